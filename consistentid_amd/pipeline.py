"""Hot-path pipelines: the denoising loops of the reference's four pipeline classes with
the reference's ``__call__`` keyword surface, running on the HIP engine.

  ConsistentIDStableDiffusionPipeline                  pipline_StableDiffusion_ConsistentID.py:33, loop :535-579
  ConsistentIDStableDiffusionXLPipeline                pipline_StableDiffusionXL_ConsistentID.py:44, loop :611-667
  StableDiffusionInpaintConsistentIDPipeline           pipelines/StableDIffusionInpaint_ConsistentID.py:94, loop :305-359
  StableDiffusionControlNetInpaintConsistentIDPipeline pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:94, :375-456

Scope: the per-step path, the ControlNet encoder (row f-1), the VAE decode (row f-2) and the VAE
encode of the inpaint pipelines (``image=`` / ``mask_image=`` with ``vae_encoder=HipVAEEncoder(...)``; the init image is
``image=`` when given, else ``input_id_images[0]``, where the reference reads it; PIL images go through image_prep.py).
Prompt strings are encoded by ``encode_prompt`` / ``_encode_prompt`` / ``encode_prompt_with_trigger_word`` on the HIP
text towers (``text_encoder=`` / ``text_encoder_2=``, clip_text.py; prompt_encode.py), the ID tokens by
``prepare_prompt_embeds``.  With ``safety_checker=`` (safety.py; ``from_pretrained`` reads ``safety_checker/``) the three
SD1.5-family pipelines (SD1.5, inpaint, ControlNet-inpaint) run the reference's ``run_safety_checker`` after the VAE
decode.  They also run the reference's whole pre-loop (``prepare_id_prompt_embeds``: the caller's FaceID app, HipBiSeNet face parsing, the facial crops, the
CLIP vision tower) for ``prompt`` + ``input_id_images``; every ``__call__`` also takes what the pre-loop produces:
``prompt_embeds`` = cat([null, augmented, text_only]) of shape [3B, 77+4, Dc] exactly as the
reference assembles it before ``.chunk(3)`` (ref :494-507, :527-531), and ``latents``.
In SDXL (whose reference ``__call__`` reads names it never defines, so there is nothing sound to mirror), and in the SD1.5
family without the pre-loop components, string prompts / ID images raise NotImplementedError naming what is missing
instead of silently doing something else; ``output_type`` other than "latent" needs the pipeline to be built with
``vae=HipVAEDecoder(...)``.

Community LoRA files (the reference scripts' ``load_lora_weights`` / ``set_adapters`` / ``fuse_lora`` block) are merged into
the packed weights of the UNet and the text towers in place (lora.py; ``_BasePipeline.load_lora_weights`` and the methods
after it).

B > 1 is this framework's extension (the reference is effectively B = 1 per call,
SURVEY.md Appendix B): B independent samples, each with its own CFG pair.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Any, List, Optional, Union

import numpy as np
import torch

from .controlnet import HipMultiControlNet, prepare_control_arguments
from .denoise import DenoiseEngine, check_eta, check_guidance_rescale, check_pag, check_sag, refuse_sag_with
from .scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, LCMScheduler,  # noqa: F401
                        PNDMScheduler)
from .unet import HipUNet


@dataclass
class StableDiffusionPipelineOutput:
    images: Any
    nsfw_content_detected: Optional[List[bool]] = None


@dataclass
class StableDiffusionXLPipelineOutput:
    images: Any


def inpaint_draws(generator, *, image_batch: int, batch_size: int, latent_channels: int, h: int, w: int,
                  unet_channels: int, latents_given: bool, strength: float, device):
    """The random draws of the inpaint pipelines' pre-loop, in diffusers 0.23's order (prepare_latents, then
    prepare_mask_latents; inpaint ref :255-292, CN :318-356), each a fp16 ``randn_tensor`` (vae.randn_tensor):
      1. the posterior eps of the init image [image_batch, L, h, w] -- only if it is encoded: a 4-channel UNet
         (return_image_latents) or no ``latents`` with ``strength`` < 1 (the add_noise start);
      2. ``noise`` [batch_size, L, h, w] -- only without ``latents`` (given latents ARE the noise);
      3. the posterior eps of the masked image [image_batch, L, h, w] -- always: the reference encodes the masked image
         even for a 4-channel UNet, which then ignores it.
    Returns (eps_image or None, noise or None, eps_masked)."""
    from .vae import randn_tensor
    enc_shape = (image_batch, latent_channels, h, w)
    eps_image = noise = None
    if unet_channels == 4 or (not latents_given and strength < 1.0):
        eps_image = randn_tensor(enc_shape, generator=generator, device=device, dtype=torch.float16)
    if not latents_given:
        noise = randn_tensor((batch_size, latent_channels, h, w), generator=generator, device=device, dtype=torch.float16)
    eps_masked = randn_tensor(enc_shape, generator=generator, device=device, dtype=torch.float16)
    return eps_image, noise, eps_masked


class _BasePipeline:
    default_guidance = 5.0
    vae_scale_factor = 8

    def __init__(self, unet: HipUNet, scheduler: Optional[DDIMScheduler] = None, use_graph: bool = True,
                 num_tokens: int = 4, lora_rank: int = 128, vae=None, vae_encoder=None, text_encoder=None, tokenizer=None,
                 text_encoder_2=None, tokenizer_2=None, safety_checker=None, feature_extractor=None):
        """``vae``: a ``consistentid_amd.vae.HipVAEDecoder`` -- enables every ``output_type`` besides "latent".
        ``vae_encoder``: a ``consistentid_amd.vae.HipVAEEncoder`` or a ``consistentid_amd.vae_tiny.HipAutoencoderTinyEncoder``
        (anything with their ``encode_inpaint``) -- lets the inpaint pipelines take ``image=`` and ``mask_image=`` (the
        reference's pre-loop VAE encode) instead of pre-computed latents.  Either encoder stands beside either decoder.
        ``text_encoder`` / ``text_encoder_2``: ``consistentid_amd.clip_text.HipCLIPTextModel`` (CLIP-L; SDXL's bigG with
        projection), ``tokenizer`` / ``tokenizer_2``: ``transformers.CLIPTokenizer`` -- let ``encode_prompt`` take strings.
        ``safety_checker``: a ``consistentid_amd.safety.HipSafetyChecker`` (or any callable with diffusers' ``(images=,
        clip_input=) -> (images, [bool])``) -- the SD1.5-family pipelines then fill ``nsfw_content_detected`` and black out
        flagged images; ``feature_extractor``: its pre-processing settings ``{"size": n}``, a preprocessor config dict or a
        transformers image processor (loader.feature_extractor_settings refuses what clip_preprocess does not do; default:
        the checker's own ``image_size``, 224 for ViT-L/14)."""
        self.unet = unet
        self.text_encoder, self.tokenizer = text_encoder, tokenizer
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2
        self.vae = vae
        self.vae_encoder = vae_encoder
        self.safety_checker = safety_checker
        self.feature_extractor = None
        if feature_extractor is not None:
            from .loader import feature_extractor_settings
            self.feature_extractor = feature_extractor_settings(feature_extractor)
        self.num_tokens = num_tokens
        self.lora_rank = lora_rank
        self.device = unet.device
        self._engine = DenoiseEngine(unet, scheduler or DDIMScheduler(), use_graph)
        # community LoRA files: adapters by name in load order ({target: modules}), active name -> weight, the multiplier of
        # fuse_lora, and the targets whose packed weights currently hold a LoRA
        self._lora_adapters, self._lora_active, self._lora_fuse, self._lora_merged = {}, {}, 1.0, set()

    def to(self, device=None, *args, **kwargs):
        """``pipe.to(device)`` of the reference scripts (infer.py:21, demo/controlnet_demo.py:60): the engines are built on
        their device by ``from_pretrained(..., device=)``; this only checks that the request names that device."""
        if device is not None and not isinstance(device, torch.dtype):
            want = torch.device(device)
            if want.type != "cuda" or (want.index is not None and want.index != (self.device.index or 0)):
                raise ValueError(f"the engine lives on {self.device} (no CPU path, weights are packed per device): "
                                 f"build the pipeline with from_pretrained(..., device={str(want)!r})")
        return self

    def _nothing_to_do(self, *args, **kwargs) -> None:
        """The memory and progress-bar switches the reference scripts call between load and generate
        (demo/controlnet_demo.py ``pipe.enable_model_cpu_offload()``): accepted and ignored.  The engine's weights are packed
        on the device at load time, so there is nothing to offload, slice or tile, the attention is the engine's own, and
        the captured loop draws no progress bar."""
        return None

    enable_model_cpu_offload = enable_sequential_cpu_offload = enable_vae_slicing = enable_vae_tiling = _nothing_to_do
    enable_xformers_memory_efficient_attention = set_progress_bar_config = _nothing_to_do

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """``pipe.enable_freeu(s1, s2, b1, b2)`` of diffusers 0.23, which the reference pipelines inherit (FreeU,
        arXiv 2309.11497): in the UNet's first two up blocks the skip features' low frequencies are scaled by s1 / s2 and the
        first half of the backbone's channels by b1 / b2 (``HipUNet.enable_freeu``, cid_freeu_f16).  All four are required,
        finite real numbers -- diffusers does not check them; a NaN there becomes a NaN image."""
        vals = (s1, s2, b1, b2)
        for name, v in zip(("s1", "s2", "b1", "b2"), vals):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"enable_freeu: {name} must be a finite number (got {v!r})")
        self.unet.enable_freeu(*(float(v) for v in vals))

    def disable_freeu(self):
        """``pipe.disable_freeu()`` of diffusers 0.23: the up blocks run as without FreeU, with no extra launch"""
        self.unet.disable_freeu()

    def enable_pag(self, pag_applied_layers="mid"):
        """Perturbed-attention guidance (arXiv 2403.17377), diffusers' ``pag_applied_layers``: a string or a list of ``"mid"``,
        ``"down.block_i"``, ``"up.block_i"``, optionally with ``".attentions_j"``, or module paths such as
        ``"down_blocks.1.attentions.0"``; every self-attention under a named module is perturbed, an id that names none raises
        ValueError.  The guidance itself is switched per call: ``pipe(..., pag_scale=3.0, pag_adaptive_scale=0.0)`` -- a call
        with ``pag_scale`` > 0 and no selection takes ``"mid"``.  Needs a UNet built with ``keep_base=True`` (RuntimeError)."""
        self.unet.enable_pag(pag_applied_layers)

    def disable_pag(self):
        """drop the selection of :meth:`enable_pag` (a later call with ``pag_scale`` > 0 selects ``"mid"`` again)"""
        self.unet.disable_pag()

    def _check_pag(self, pag_scale, pag_adaptive_scale, guidance_rescale: float = 0.0, sag_scale=0.0) -> dict:
        """the PAG keywords and ``sag_scale`` of a ``__call__``, validated -> the engine's keywords; the refusals that need no
        tensor are made here, before the pre-loop runs.  ``sag_scale`` == 0 adds no keyword: the call is the call without it."""
        pag_scale, pag_adaptive_scale = check_pag(pag_scale, pag_adaptive_scale)
        sag_scale = check_sag(sag_scale)
        refuse_sag_with(sag_scale, pag_scale, guidance_rescale)
        if sag_scale > 0.0:
            return dict(sag_scale=sag_scale)
        if pag_scale > 0.0 and guidance_rescale > 0.0:
            raise NotImplementedError("pag_scale > 0 together with guidance_rescale > 0 is not built")
        if pag_scale > 0.0 and not self.unet.pag_layers:
            self.unet.enable_pag()
        return dict(pag_scale=pag_scale, pag_adaptive_scale=pag_adaptive_scale)

    @property
    def sag_mass(self):
        """fp32 [B, H_mid * W_mid], or None: the column mass of the mid block's first self-attention map that the last
        evaluation of the last call with ``sag_scale`` > 0 thresholded at 1; a view of the engine's buffer"""
        return self._engine.sag_mass

    @property
    def scheduler(self):
        """the reference scripts replace the scheduler AFTER construction (infer.py:33
        ``pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)``, demo/controlnet_demo.py:67 with DDIM):
        the attribute is the denoise engine's scheduler, so the assignment takes effect on the next call (the per-step
        coefficients live in device buffers the captured step reads, the graphs stay valid)"""
        return self._engine.scheduler

    @scheduler.setter
    def scheduler(self, sch):
        if not (hasattr(sch, "coefficient_table") or hasattr(sch, "coefficient_rows")):
            raise TypeError(f"{type(sch).__name__}: the engine takes consistentid_amd.scheduler.DDIMScheduler / "
                            "EulerDiscreteScheduler / PNDMScheduler / DPMSolverMultistepScheduler / LCMScheduler (build one with "
                            ".from_config(diffusers_scheduler.config))")
        self._engine.scheduler = sch

    def _variance_noise(self, eta: float, generator, variance_noise, latents, num_inference_steps: int, first_step: int = 0):
        """``eta`` of the reference ``__call__``s (prepare_extra_step_kwargs -> DDIMScheduler.step(eta=, generator=)): with
        DDIM and eta > 0 every executed step adds sigma_t * randn.  The tensors are drawn here, before the loop, one
        ``randn_tensor`` [B, C, h, w] fp16 per executed step in loop order on ``generator`` -- after every pre-loop draw, so
        the generator's stream is consumed in diffusers' order -- or taken from ``variance_noise`` [steps, B, C, h, w].
        ``LCMScheduler`` (eta stays 0) noises the sample again after every executed step but the last: executed steps - 1
        tensors, drawn or taken in the same way; a single step needs none."""
        lcm = isinstance(self.scheduler, LCMScheduler)
        if (check_eta(self.scheduler, eta, variance_noise) == 0.0 and not lcm) or variance_noise is not None:
            return variance_noise       # no noise term (None), or the caller's tensors
        from .vae import randn_tensor
        self.scheduler.set_timesteps(num_inference_steps)
        n_draw = len(self.scheduler.timesteps) - first_step - (1 if lcm else 0)
        if n_draw <= 0:
            return None
        return torch.stack([randn_tensor(tuple(latents.shape), generator=generator, device=self.device, dtype=torch.float16)
                            for _ in range(n_draw)])

    # -- surface kept from the reference ------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=torch.float16, device="cuda:0", **kwargs):
        """``ConsistentIDPipeline.from_pretrained(base_model_path, torch_dtype=torch.float16)`` (infer.py:17-21): UNet and VAE
        decoder of a LOCAL diffusers model directory -> engines (loader.py); ``controlnet=`` as in demo/controlnet_demo.py:44-47.
        Follow with ``load_ConsistentID_model`` exactly like the reference."""
        from . import loader
        return loader.from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=torch_dtype, device=device, **kwargs)

    def load_ConsistentID_model(self, pretrained_model_name_or_path_or_dict, weight_name: str = "", subfolder: str = "",
                                trigger_word_ID: str = "<|image|>", trigger_word_facial: str = "<|facial|>",
                                image_encoder_path: str = "", bise_net_cp: str = "", torch_dtype=torch.float16,
                                num_tokens: int = 4, lora_rank: int = 128, face_app=None, **kwargs):
        """Reference: pipline_StableDiffusion_ConsistentID.py:36-150.  The ``adapter_modules`` entry of the checkpoint
        (dict, ``.bin`` or ``.safetensors`` path; local files only) is merged into the engine in place -- the UNet must
        have been built with ``keep_base=True``.  FacialEncoder / image_proj weights build the ID-conditioning engine
        (``prepare_prompt_embeds``, row f-3).
        ``image_encoder_path``: a local transformers CLIPVisionModelWithProjection folder (config.json + weights) ->
        ``self.image_encoder`` (HipCLIPVision, ref :54-56).  ``bise_net_cp``: a ``face_parsing.pth`` file (or its state dict)
        -> ``self.bise_net`` (HipBiSeNet, ref :67-71).  ``face_app``: the FaceID model, any object with insightface's
        ``get(np.ndarray RGB image) -> [face, ...]`` whose faces carry ``normed_embedding`` (ref :58-59, :216-226) ->
        ``self.app``.  Empty strings / None leave a component out; a path that does not exist raises FileNotFoundError
        (hub ids are never resolved)."""
        for what, path in (("image_encoder_path", image_encoder_path), ("bise_net_cp", bise_net_cp)):
            if isinstance(path, (str, os.PathLike)) and os.fspath(path) and not os.path.exists(path):
                raise FileNotFoundError(f"{what}: {os.fspath(path)!r} does not exist (local paths only, hub ids are not resolved)")
        self.image_encoder = self.bise_net = None
        if image_encoder_path:
            from . import loader
            from .clip_vision import HipCLIPVision
            cfg, sd = loader.read_component(image_encoder_path, loader.TEXT_WEIGHT_NAMES)
            self.image_encoder = HipCLIPVision(sd, num_heads=cfg["num_attention_heads"], patch_size=cfg.get("patch_size", 14),
                                               device=self.device, hidden_act=cfg.get("hidden_act", "gelu"),
                                               layer_norm_eps=cfg.get("layer_norm_eps", 1e-5))
            self.clip_image_size = int(cfg.get("image_size", 224))
        if isinstance(bise_net_cp, dict) or bise_net_cp:
            from .face_parsing import HipBiSeNet
            sd = bise_net_cp if isinstance(bise_net_cp, dict) else torch.load(bise_net_cp, map_location="cpu", weights_only=True)
            self.bise_net = HipBiSeNet(sd, n_classes=19, device=self.device)
        self.app = face_app
        from .checkpoint import load_checkpoint
        state_dict = load_checkpoint(pretrained_model_name_or_path_or_dict, weight_name, subfolder)
        self.lora_rank, self.num_tokens, self.torch_dtype = lora_rank, num_tokens, torch_dtype
        self.trigger_word_ID, self.trigger_word_facial = trigger_word_ID, trigger_word_facial
        self.unet.num_tokens = num_tokens
        self.unet.load_adapter_modules(state_dict["adapter_modules"])                  # ref :143-144 (strict)
        # once-per-image ID-conditioning modules (ProjPlusModel / FacialEncoder, ref :93-100, :141-142)
        # trigger tokens (ref :148-150): both to the tokenizer; SDXL adds only <|image|> to tokenizer_2 (ref SDXL :164-176)
        if self.tokenizer is not None:
            self.tokenizer.add_tokens([trigger_word_ID], special_tokens=True)
            self.tokenizer.add_tokens([trigger_word_facial], special_tokens=True)
        if self.tokenizer_2 is not None:
            self.tokenizer_2.add_tokens([trigger_word_ID], special_tokens=True)
        self.image_proj_state = state_dict.get("image_proj")
        self.facial_encoder_state = state_dict.get("FacialEncoder")
        self.id_conditioner = None
        if self.image_proj_state and self.facial_encoder_state:
            from .idstack import HipIDConditioner
            self.id_conditioner = HipIDConditioner(self.image_proj_state, self.facial_encoder_state, device=self.device)
        self._engine.invalidate()
        return self

    # -- community LoRA files (lora.py): infer.py's "using LoRA modules in community" block -------------------
    def _lora_engines(self):
        return {"unet": self.unet, "text_encoder": self.text_encoder, "text_encoder_2": self.text_encoder_2}

    def _apply_lora(self):
        """hand every engine its active ``(modules, weight x fuse multiplier)`` entries, in load order; engines no adapter
        ever touched are left alone.  The step graphs are forgotten as after ``load_ConsistentID_model`` (addresses do not
        change)."""
        adapters, active = self._lora_adapters, self._lora_active
        for target, engine in self._lora_engines().items():
            entries = [(adapters[n][target], active[n] * self._lora_fuse) for n in adapters if n in active and adapters[n][target]]
            if engine is not None and (entries or target in self._lora_merged):
                engine.set_lora(entries)
                if entries:
                    self._lora_merged.add(target)
                else:
                    self._lora_merged.discard(target)
        self._engine.invalidate()

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name: Optional[str] = None,
                          adapter_name: Optional[str] = None, **ignored):
        """``pipe.load_lora_weights(os.path.dirname(lora_path), weight_name=lora_model_name)`` (infer.py, infer_SDXL.py): a
        kohya or diffusers LoRA file (dict, ``.safetensors``, ``.bin`` / ``.pt``, or folder + ``weight_name``; local files
        only) is parsed and validated as a whole (lora.parse_lora), stored under ``adapter_name`` (default ``default_0``,
        ``default_1``, ...), activated at weight 1.0 and merged into the packed weights of the UNet and the text towers in
        place.  The UNet (and a tower the file addresses) must have been built with ``keep_base=True``, as ``from_pretrained``
        does.  Nothing is touched when anything is refused."""
        from . import lora
        adapters, active = self._lora_adapters, self._lora_active
        if adapter_name is None:
            adapter_name = next(f"default_{i}" for i in range(len(adapters) + 1) if f"default_{i}" not in adapters)
        if adapter_name in adapters:
            raise ValueError(f"adapter {adapter_name!r} is already loaded: pick another adapter_name or unload_lora_weights()")
        flat = lora.read_lora(pretrained_model_name_or_path_or_dict, weight_name)
        engines = self._lora_engines()
        parsed = lora.parse_lora(flat, self.unet.config, {t: getattr(e, "spec", None) for t, e in engines.items() if t != "unet"})
        for target, modules in parsed.items():
            if modules:
                engines[target].require_base()
        adapters[adapter_name] = parsed
        active[adapter_name] = 1.0
        self._apply_lora()
        return self

    def set_adapters(self, adapter_names, adapter_weights=None):
        """``pipe.set_adapters([...], adapter_weights=[...])``: the listed adapters become active with those weights (a float
        for all, a list, or None = 1.0), every other adapter inactive"""
        adapters, active = self._lora_adapters, self._lora_active
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if adapter_weights is None or isinstance(adapter_weights, (int, float)):
            weights = [1.0 if adapter_weights is None else float(adapter_weights)] * len(names)
        else:
            weights = [1.0 if w is None else float(w) for w in adapter_weights]
        if len(weights) != len(names):
            raise ValueError(f"{len(names)} adapter names with {len(weights)} adapter weights")
        unknown = [n for n in names if n not in adapters]
        if unknown or len(set(names)) != len(names):
            raise ValueError(f"set_adapters: unknown or repeated adapter name(s) {unknown or names}; loaded: {list(adapters)}")
        active.clear()
        active.update(zip(names, weights))
        self._apply_lora()
        return self

    def fuse_lora(self, lora_scale: float = 1.0, **ignored):
        """``pipe.fuse_lora()``: the engine's weights are always merged, so this only sets one multiplier on all active
        adapters; ``unfuse_lora`` resets it and the adapters are active at their own weights again, as in diffusers"""
        self._lora_fuse = float(lora_scale)
        self._apply_lora()
        return self

    def unfuse_lora(self, **ignored):
        return self.fuse_lora(1.0)

    def unload_lora_weights(self):
        """drop every adapter; the packed weights return to the base (with the ConsistentID adapter, if loaded) bit for bit"""
        adapters, active = self._lora_adapters, self._lora_active
        adapters.clear()
        active.clear()
        self._lora_fuse = 1.0
        self._apply_lora()
        return self

    def get_active_adapters(self) -> List[str]:
        adapters, active = self._lora_adapters, self._lora_active
        return [n for n in adapters if n in active]

    def get_list_adapters(self) -> List[str]:
        return list(self._lora_adapters)

    def prepare_prompt_embeds(self, **encoder_outputs) -> torch.Tensor:
        """``prompt_embeds`` = cat([null, augmented, text_only]) from the upstream encoders' outputs (what ref :479-507
        computes between the CLIP / FaceID / text encoders and the loop): see ``idstack.HipIDConditioner.__call__`` for
        the keywords.  Needs a checkpoint with ``image_proj`` and ``FacialEncoder`` loaded (``load_ConsistentID_model``)."""
        if getattr(self, "id_conditioner", None) is None:
            raise RuntimeError("no ID-conditioning weights: load_ConsistentID_model(checkpoint with image_proj + FacialEncoder)")
        return self.id_conditioner(**encoder_outputs)

    def _check_hot_path_inputs(self, prompt, input_id_images, prompt_embeds, latents, output_type):
        if prompt is not None or input_id_images is not None:
            raise NotImplementedError(
                f"{type(self).__name__}.__call__(prompt=..., input_id_images=...) is built for the SD1.5 pipeline only "
                "(ConsistentIDStableDiffusionPipeline): encode the text with encode_prompt_with_trigger_word / "
                "encode_prompt, build prompt_embeds with prepare_prompt_embeds and pass it with latents")
        if prompt_embeds is None or latents is None:
            raise ValueError("prompt_embeds (cat([null, augmented, text_only])) and latents are required")
        if output_type != "latent" and self.vae is None:
            raise ValueError("output_type other than 'latent' needs a VAE decoder: build the pipeline with "
                             "vae=HipVAEDecoder(...)")

    @staticmethod
    def _numpy_to_pil(arr: np.ndarray):
        """NHWC float in [0, 1] -> PIL images (diffusers numpy_to_pil)"""
        from PIL import Image
        return [Image.fromarray(a) for a in (arr * 255).round().astype("uint8")]

    def run_safety_checker(self, image, device=None, dtype=None):
        """D: StableDiffusionPipeline.run_safety_checker (ref :589-602, inpaint :371, CN :468) -> (image, has_nsfw_concept).
        ``image``: NHWC numpy in [0, 1] (the SD1.5 pipeline checks after decode_latents) or the decoded [B, 3, H, W] device
        tensor in [0, 1] (the inpaint pipelines check the tensor).  Either becomes PIL images as ``_postprocess`` builds
        them, those go through ``face_prep.clip_preprocess`` (the feature extractor) and the checker; flagged images come
        back black -- a tensor is zeroed in place on the device.  Without a checker: (image, None), as in diffusers.
        ``device`` / ``dtype`` are the reference's arguments; the engine has one device and computes in fp16."""
        if self.safety_checker is None:
            return image, None
        from .face_prep import clip_preprocess
        arr = image.float().permute(0, 2, 3, 1).cpu().numpy() if torch.is_tensor(image) else image
        size = (self.feature_extractor or {}).get("size") or getattr(self.safety_checker, "image_size", 224)
        clip_input = torch.from_numpy(np.stack([clip_preprocess(im, size) for im in self._numpy_to_pil(arr)]))
        return self.safety_checker(images=image, clip_input=clip_input)

    def _postprocess(self, latents: torch.Tensor, output_type: str, legacy_numpy: bool = False):
        """``_postprocess_checked`` without the safety checker: the images only (SDXL :676-684 has no checker)"""
        return self._postprocess_checked(latents, output_type, legacy_numpy, check=False)[0]

    def _postprocess_checked(self, latents: torch.Tensor, output_type: str, legacy_numpy: bool = False, check: bool = True):
        """-> (images, has_nsfw_concept).  SD1.5 (ref :581-602): decode_latents -> NHWC float32 numpy in [0, 1] ->
        run_safety_checker on the numpy array (-> PIL for "pil"); any other non-latent output_type also yields numpy there
        (``legacy_numpy``).  The image_processor-based pipelines (SDXL :676-684, inpaint :367-381) check the decoded tensor
        and additionally know "pt" (the [B, 3, H, W] tensor in [0, 1]).  "latent" is never checked."""
        if output_type == "latent":
            return latents, None
        img = self.vae.decode_latents(latents)
        nsfw = None
        if check and not legacy_numpy:
            img, nsfw = self.run_safety_checker(img)
        if output_type == "pt" and not legacy_numpy:
            return img, nsfw
        arr = img.float().permute(0, 2, 3, 1).cpu().numpy()
        if check and legacy_numpy:
            arr, nsfw = self.run_safety_checker(arr)
        if output_type == "pil":
            return self._numpy_to_pil(arr), nsfw
        return arr, nsfw

    @staticmethod
    def _output(out, return_dict: bool, has_nsfw_concept: Optional[List[bool]] = None):
        """the SD1.5-family tail (ref :608-613); ``has_nsfw_concept`` is None without a safety checker and for latents"""
        if not return_dict:
            return (out, has_nsfw_concept)
        return StableDiffusionPipelineOutput(images=out, nsfw_content_detected=has_nsfw_concept)

    def _split(self, prompt_embeds):
        assert prompt_embeds.shape[0] % 3 == 0
        return prompt_embeds.chunk(3)   # null, augmented, text-only (ref :527-531)


class _SD15PromptEncoding:
    """Prompt encoding of the SD1.5-family pipelines (SD1.5, inpaint, ControlNet-inpaint): D: encode_prompt /
    _encode_prompt of diffusers 0.23 on ``self.text_encoder`` (prompt_encode.py), and the reference's
    ``encode_prompt_with_trigger_word`` (prompt_utils.py) on ``self.tokenizer``."""

    def encode_prompt(self, prompt, device=None, num_images_per_prompt: int = 1, do_classifier_free_guidance: bool = True,
                      negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None,
                      clip_skip=None, max_embeddings_multiples: int = 1):
        """-> (prompt_embeds, negative_prompt_embeds), fp16 on the engine's device.  ``max_embeddings_multiples`` >= 2: long
        weighted prompts (prompt_weighting.py): ``(word)``, ``[word]``, ``(word:1.3)`` are parsed and the texts encoded in up
        to that many chunks of 75 tokens, [B, 77 m, Dc]; 1 (default): diffusers' path, brackets literal, cut at 77."""
        from .prompt_encode import encode_prompt
        return encode_prompt(self.tokenizer, self.text_encoder, prompt, device or self.device, num_images_per_prompt,
                             do_classifier_free_guidance, negative_prompt, prompt_embeds, negative_prompt_embeds, lora_scale,
                             clip_skip, max_embeddings_multiples=max_embeddings_multiples)

    def _encode_prompt(self, prompt, device=None, num_images_per_prompt: int = 1, do_classifier_free_guidance: bool = True,
                       negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None,
                       max_embeddings_multiples: int = 1):
        """legacy form the reference calls (ref :469-475, :494-501): cat([negative, prompt])"""
        from .prompt_encode import encode_prompt_legacy
        return encode_prompt_legacy(self.tokenizer, self.text_encoder, prompt, device or self.device, num_images_per_prompt,
                                    do_classifier_free_guidance, negative_prompt, prompt_embeds, negative_prompt_embeds,
                                    lora_scale, max_embeddings_multiples=max_embeddings_multiples)

    def encode_prompt_with_trigger_word(self, prompt: str, face_caption: str, key_parsing_mask_list=None,
                                        image_token: str = "<|image|>", facial_token: str = "<|facial|>",
                                        max_num_facials: int = 5, num_id_images: int = 1, device=None):
        """ref :311-347 -> (prompt_text_only, clean_input_id, key_parsing_mask_list_align, facial_token_mask,
        facial_token_idx, facial_token_idx_mask)"""
        from .prompt_utils import encode_prompt_with_trigger_word
        if self.tokenizer is None:
            raise ValueError("no tokenizer: build the pipeline with tokenizer= (from_pretrained reads tokenizer/)")
        return encode_prompt_with_trigger_word(self.tokenizer, prompt, face_caption,
                                               {} if key_parsing_mask_list is None else key_parsing_mask_list, image_token,
                                               facial_token, max_num_facials, num_id_images)


class _IDPreLoop:
    """The SD1.5 reference's pre-loop (pipline_StableDiffusion_ConsistentID.py:177-376, :437-507): FaceID (the caller's
    ``face_app``), face parsing (HipBiSeNet), the facial crops and the CLIP vision tower (HipCLIPVision), then the
    ID-conditioning modules (HipIDConditioner).  Public methods keep the reference's names and return values."""

    FACE_CAPTION = "The person has one face, one nose, two eyes, two ears, and one mouth."   # ref :283
    PARSE_SIZE = 512

    def _missing_id_components(self) -> List[str]:
        need = (("FaceID app (load_ConsistentID_model(face_app=...))", getattr(self, "app", None)),
                ("BiSeNet (bise_net_cp=)", getattr(self, "bise_net", None)),
                ("image encoder (image_encoder_path=)", getattr(self, "image_encoder", None)),
                ("ID weights (image_proj + FacialEncoder)", getattr(self, "id_conditioner", None)),
                ("text encoder", self.text_encoder), ("tokenizer", self.tokenizer))
        return [name for name, v in need if v is None]

    def _takes_id_pre_loop(self, prompt, input_id_images, prompt_embeds) -> bool:
        """The argument checks the SD1.5-family ``__call__``s share: True when the call goes through the pre-loop (``prompt`` +
        ``input_id_images``), False when it brings its own ``prompt_embeds``."""
        if prompt is None and input_id_images is None:
            return False
        missing = self._missing_id_components()
        if missing:
            raise NotImplementedError("__call__(prompt=..., input_id_images=...) needs: " + ", ".join(missing)
                                      + "; or build prompt_embeds with prepare_prompt_embeds and pass it with latents")
        if prompt is None or input_id_images is None:
            raise ValueError("prompt and input_id_images go together (ref :434-438)")
        if prompt_embeds is not None:
            raise ValueError("give either prompt + input_id_images or prompt_embeds, not both")
        return True

    def _id_call_prompt_embeds(self, prompt, input_id_images, negative_prompt, num_images_per_prompt,
                               max_embeddings_multiples: int = 1) -> torch.Tensor:
        """``prompt_embeds`` [3n, 77 m + num_tokens, Dc] of a pre-loop call (m = 1 unless ``max_embeddings_multiples`` >= 2 and
        the negative prompt needs more chunks): the pre-loop runs once and each of its three row
        groups is repeated ``num_images_per_prompt`` = n times, which is diffusers' meaning of the argument (the reference
        itself breaks on n > 1)."""
        n = 1 if num_images_per_prompt is None else int(num_images_per_prompt)
        if n < 1:
            raise ValueError(f"num_images_per_prompt must be at least 1, got {num_images_per_prompt}")
        pe = self.prepare_id_prompt_embeds(prompt, input_id_images, negative_prompt, max_embeddings_multiples)
        return pe if n == 1 else torch.cat([rows.repeat(n, 1, 1) for rows in pe.chunk(3)])

    def get_prepare_faceid(self, face_image) -> torch.Tensor:
        """ref :216-226: the first face's ``normed_embedding`` [1, 512], zeros when the app finds no face"""
        faces = self.app.get(np.array(face_image))
        if len(faces) == 0:
            return torch.zeros(1, 512)
        return torch.from_numpy(np.asarray(faces[0].normed_embedding)).unsqueeze(0)

    def get_prepare_llva_caption(self, input_image_file, model_path=None, prompt=None) -> str:
        """ref :265-287: the reference's built-in template (its LLaVA call is commented out)"""
        return self.FACE_CAPTION

    def parsing_face_mask(self, raw_image_refer):
        """ref :229-262 -> (colour overlay uint8 [512, 512, 3] (BGR blend), label map uint8 [512, 512])"""
        from PIL import Image
        from .face_prep import parsing_overlay
        image = raw_image_refer.convert("RGB").resize((self.PARSE_SIZE, self.PARSE_SIZE), Image.BILINEAR)
        labels = self.bise_net(image, size=None)[0].cpu().numpy()
        return parsing_overlay(np.asarray(image), labels), labels

    def get_prepare_facemask(self, input_image_file):
        """ref :289-309 -> (key_parsing_mask_list, colour overlay)"""
        from .face_prep import masks_for_unique_values, select_face_masks
        overlay, labels = self.parsing_face_mask(input_image_file)
        return select_face_masks(masks_for_unique_values(labels)), overlay

    def get_prepare_clip_image(self, input_image_file, key_parsing_mask_list, image_size: int = 512,
                               max_num_facials: int = 5, change_facial: bool = True):
        """ref :350-376 -> (facial_clip_image [max_num_facials, 3, 224, 224] fp32, facial_mask [max_num_facials, S, S]); the
        part masks come from the 512 x 512 label map, so the reference's CenterCrop(image_size) keeps them whole"""
        from .face_prep import clip_preprocess, fetch_mask_raw_image
        clips, masks = [], []
        for key in key_parsing_mask_list:
            m = key_parsing_mask_list[key]
            a = np.asarray(m, dtype=np.float32) / 255
            if a.shape != (image_size, image_size):
                raise ValueError(f"facial mask {key!r} is {a.shape}, expected {image_size} x {image_size}")
            masks.append(torch.from_numpy(a))
            clips.append(torch.from_numpy(clip_preprocess(fetch_mask_raw_image(input_image_file, m))))
        n = len(clips)
        clips += [torch.zeros(3, 224, 224) for _ in range(max_num_facials - n)]
        masks += [torch.zeros(image_size, image_size) for _ in range(max_num_facials - n)]
        return torch.stack(clips), torch.stack(masks)

    def _clip_hidden(self, pixel_values: torch.Tensor) -> torch.Tensor:
        return self.image_encoder.hidden_states(pixel_values.to(self.device, torch.float16), -2)

    def get_image_embeds(self, faceid_embeds, face_image, s_scale: float, shortcut: bool = False):
        """ref :197-209 -> (prompt tokens, uncond prompt tokens) of ProjPlusModel"""
        from .face_prep import clip_preprocess
        pix = torch.from_numpy(clip_preprocess(face_image))[None]
        hs = self._clip_hidden(torch.cat([pix, torch.zeros_like(pix)]))
        ip = self.id_conditioner.image_proj_model
        fid = faceid_embeds.to(self.device, torch.float16)
        return (ip(fid, hs[:1], shortcut=shortcut, scale=s_scale),
                ip(torch.zeros_like(fid), hs[1:], shortcut=shortcut, scale=s_scale))

    def get_facial_embeds(self, prompt_embeds, negative_prompt_embeds, facial_clip_images, facial_token_masks,
                          valid_facial_token_idx_mask):
        """ref :177-195 -> (facial prompt embeds, uncond facial prompt embeds); facial_clip_images [B, n, 3, 224, 224]"""
        B, n = facial_clip_images.shape[:2]
        hs = self._clip_hidden(torch.cat([facial_clip_images.reshape(B * n, *facial_clip_images.shape[2:]),
                                          torch.zeros_like(facial_clip_images[0, :1])]))
        emb = hs[:B * n].reshape(B, n, *hs.shape[1:])
        uncond = hs[B * n:].expand(B * n, *hs.shape[1:]).reshape(B, n, *hs.shape[1:])
        fe = self.id_conditioner.FacialEncoder
        return (fe(prompt_embeds, emb, facial_token_masks, valid_facial_token_idx_mask),
                fe(negative_prompt_embeds, uncond, facial_token_masks, valid_facial_token_idx_mask))

    def prepare_id_prompt_embeds(self, prompt: str, input_id_images, negative_prompt=None,
                                 max_embeddings_multiples: int = 1) -> torch.Tensor:
        """``prompt_embeds`` [3, 77 + num_tokens, Dc] = cat([null, augmented, text_only]) of ONE prompt and its ID images,
        assembled as ref :437-507 does.  The CLIP tower runs each distinct image once: the face, its real crops and one zero
        image, whose hidden states stand for every padded crop and every uncond input.
        ``max_embeddings_multiples`` >= 2 (prompt_weighting.py): the NEGATIVE prompt is parsed for emphasis, weighted and
        encoded in the m <= max_embeddings_multiples chunks it needs.  The trigger-word machinery is the reference's and is
        defined on the 77 window, so the prompt (with the trigger word and the facial caption) is tokenised as always, its
        brackets literal; both positive sets are continued to 77 m rows with the tower's output for the empty chunk
        [bos, pad x 75, eos] and the facial token mask with zeros -> [3, 77 m + num_tokens, Dc].  Emphasis in the positive
        prompt of an ID call: ``encode_prompt(..., max_embeddings_multiples=)`` + ``prepare_prompt_embeds``."""
        from .prompt_weighting import check_multiples
        check_multiples(max_embeddings_multiples)
        missing = self._missing_id_components()
        if missing:
            raise NotImplementedError("prompt + input_id_images need: " + ", ".join(missing))
        if not isinstance(prompt, str):
            raise NotImplementedError("one prompt string per call (the reference breaks on lists, SURVEY.md Appendix B)")
        images = input_id_images if isinstance(input_id_images, list) else [input_id_images]
        img = images[0]                                                                    # ref :436
        dev = self.device
        faceid = self.get_prepare_faceid(img)                                              # :438
        caption = self.get_prepare_llva_caption(img)
        masks, _ = self.get_prepare_facemask(img)
        text_only, clean_ids, masks_align, fmask, _, fidx_mask = self.encode_prompt_with_trigger_word(
            prompt, caption, masks, max_num_facials=5, num_id_images=len(images))           # :445-458
        text_embeds = self.text_encoder(clean_ids.to(dev))[0]                               # :467
        if max_embeddings_multiples == 1:
            both = self._encode_prompt(text_only, dev, 1, True, negative_prompt)           # :469-477
            neg, pos = both[:1], both[1:]
        else:
            from . import prompt_weighting as pw
            from .prompt_encode import _uncond_tokens
            pos = self.encode_prompt(text_only, dev, 1, False)[0]
            neg, _, m = pw.encode_weighted(self.tokenizer, self.text_encoder, _uncond_tokens(text_only, negative_prompt, 1),
                                           None, max_embeddings_multiples, dev)
            neg = neg.to(device=dev, dtype=torch.float16)
            pos = pw.extend_with_empty_chunks(self.text_encoder, self.tokenizer, pos, m, dev)
            text_embeds = pw.extend_with_empty_chunks(self.text_encoder, self.tokenizer, text_embeds, m, dev)
            fmask = torch.nn.functional.pad(fmask, (0, pw.WINDOW * (m - 1)))
        from .face_prep import clip_preprocess
        crops, _ = self.get_prepare_clip_image(img, masks_align, image_size=512, max_num_facials=5)    # :482
        n = len(masks_align)
        pix = torch.cat([torch.from_numpy(clip_preprocess(img))[None], crops[:n], torch.zeros(1, 3, 224, 224)])
        hs = self._clip_hidden(pix)
        face_hs, crop_hs, zero_hs = hs[:1], hs[1:1 + n], hs[1 + n:]
        facial = torch.cat([crop_hs, zero_hs.expand(5 - n, *zero_hs.shape[1:])])[None]
        return self.id_conditioner(
            text_embeds=text_embeds, negative_embeds=neg, text_only_embeds=pos, faceid_embeds=faceid,
            clip_embeds=face_hs, uncond_clip_embeds=zero_hs, facial_embeds=facial,
            uncond_facial_embeds=zero_hs.expand(5, *zero_hs.shape[1:])[None], facial_token_mask=fmask.to(dev),
            valid_facial_mask=fidx_mask.to(dev))


class ConsistentIDStableDiffusionPipeline(_IDPreLoop, _SD15PromptEncoding, _BasePipeline):
    def __call__(self, prompt=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 5.0, negative_prompt=None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
                 negative_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 cross_attention_kwargs=None, original_size=None, target_size=None, callback=None,
                 callback_steps: int = 1, input_id_images=None, start_merge_step: int = 0,
                 class_tokens_mask=None, prompt_embeds_text_only=None, variance_noise: Optional[torch.Tensor] = None,
                 max_embeddings_multiples: int = 1, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 sag_scale: float = 0.0, guidance_rescale: float = 0.0):
        """``guidance_rescale`` (diffusers 0.23 StableDiffusionPipeline; rescale_noise_cfg's phi): > 0 rescales the guided
        prediction to the conditional one's standard deviation, per sample and step.
        ``pag_scale`` / ``pag_adaptive_scale``: perturbed-attention guidance as diffusers' PAG pipelines spell it (``enable_pag``;
        DESIGN.md 4.28); 0 = off, not together with ``guidance_rescale``.
        ``sag_scale``: self-attention guidance as diffusers' StableDiffusionSAGPipeline spells it; 0 = off, not
        together with ``pag_scale`` or ``guidance_rescale``.
        ``max_embeddings_multiples`` >= 2: the negative prompt of a pre-loop call is a long weighted prompt
        (prepare_id_prompt_embeds).  ``prompt_embeds`` may have any [3B, T + num_tokens, Dc] the
        cross-attention kernels take (T <= 1024 text rows).
        ``pipe(prompt, input_id_images=[face], ...)`` runs the reference's pre-loop (prepare_id_prompt_embeds) and, without
        ``latents``, draws them like diffusers' prepare_latents (randn_tensor on the generator's device); or pass
        ``prompt_embeds`` (cat([null, augmented, text_only])) and ``latents`` directly.  ``num_images_per_prompt`` = n on the
        prompt path: n samples of the one identity -- the embeds repeated n times, the latents one draw of [n, C, h, w]."""
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        pag_kw = self._check_pag(pag_scale, pag_adaptive_scale, guidance_rescale, sag_scale)
        if self._takes_id_pre_loop(prompt, input_id_images, prompt_embeds):
            prompt_embeds = self._id_call_prompt_embeds(prompt, input_id_images, negative_prompt, num_images_per_prompt,
                                                        max_embeddings_multiples)
            n = prompt_embeds.shape[0] // 3
            if latents is None:
                from .vae import randn_tensor
                height = height or self.unet.config.sample_size * self.vae_scale_factor
                width = width or self.unet.config.sample_size * self.vae_scale_factor
                shape = (n, self.unet.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
                latents = randn_tensor(shape, generator=generator, device=self.device, dtype=torch.float16)   # ref :517-526
            elif latents.shape[0] != n:
                raise ValueError(f"latents of batch {latents.shape[0]} with num_images_per_prompt = {n}")
            prompt = input_id_images = None
        self._check_hot_path_inputs(prompt, input_id_images, prompt_embeds, latents, output_type)
        assert guidance_scale >= 1.0, "the reference asserts classifier-free guidance (ref :434,:441)"
        variance_noise = self._variance_noise(eta, generator, variance_noise, latents, num_inference_steps)
        null_e, aug_e, text_e = self._split(prompt_embeds)
        out = self._engine.run(latents, null_e, aug_e, text_e, num_inference_steps=num_inference_steps,
                               guidance_scale=guidance_scale, start_merge_step=start_merge_step,
                               callback=callback, callback_steps=callback_steps, eta=eta, variance_noise=variance_noise,
                               guidance_rescale=guidance_rescale, **pag_kw)
        out, has_nsfw_concept = self._postprocess_checked(out, output_type, legacy_numpy=True)
        return self._output(out, return_dict, has_nsfw_concept)


class ConsistentIDStableDiffusionXLPipeline(_BasePipeline):
    default_guidance = 7.5

    def __init__(self, unet: HipUNet, scheduler: Optional[DDIMScheduler] = None, force_zeros_for_empty_prompt: bool = True,
                 **kw):
        """``force_zeros_for_empty_prompt``: the SDXL pipeline config flag (model_index.json; diffusers' default True) --
        ``encode_prompt`` gives zero negative embeds when no negative prompt is given"""
        super().__init__(unet, scheduler, **kw)
        self.force_zeros_for_empty_prompt = force_zeros_for_empty_prompt

    def encode_prompt(self, prompt, prompt_2=None, device=None, num_images_per_prompt: int = 1,
                      do_classifier_free_guidance: bool = True, negative_prompt=None, negative_prompt_2=None,
                      prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                      negative_pooled_prompt_embeds=None, lora_scale=None):
        """D: StableDiffusionXLPipeline.encode_prompt (ref SDXL :552-565) on the two HIP towers -> (prompt_embeds,
        negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds).  No ``max_embeddings_multiples`` here:
        strings are cut at 77 tokens and their brackets are literal; the SDXL pipeline takes long prompts only as
        ``prompt_embeds`` / ``negative_prompt_embeds`` of T + num_tokens rows (T <= 1024) built elsewhere."""
        from .prompt_encode import encode_prompt_sdxl
        toks, encs = [self.tokenizer, self.tokenizer_2], [self.text_encoder, self.text_encoder_2]
        if self.text_encoder is None:
            toks, encs = toks[1:], encs[1:]
        return encode_prompt_sdxl(toks, encs, prompt, prompt_2, device or self.device, num_images_per_prompt,
                                  do_classifier_free_guidance, negative_prompt, negative_prompt_2, prompt_embeds,
                                  negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, lora_scale,
                                  self.force_zeros_for_empty_prompt)

    def encode_prompt_with_trigger_word(self, prompt: str, face_caption: str, key_parsing_mask_list=None,
                                        image_token: str = "<|image|>", facial_token: str = "<|facial|>",
                                        max_num_facials: int = 5, num_id_images: int = 1, device=None):
        """ref SDXL :338-391 -> (prompt_text_only, clean_input_id, clean_input_id2, key_parsing_mask_list_align,
        facial_token_mask, facial_token_idx, facial_token_idx_mask); see prompt_encode.encode_prompt_with_trigger_word_sdxl
        for the tokenizer-2 quirk it keeps"""
        from .prompt_encode import encode_prompt_with_trigger_word_sdxl
        if self.tokenizer is None or self.tokenizer_2 is None:
            raise ValueError("the SDXL trigger-word encoding needs tokenizer and tokenizer_2")
        return encode_prompt_with_trigger_word_sdxl(self.tokenizer, self.tokenizer_2, prompt, face_caption,
                                                    {} if key_parsing_mask_list is None else key_parsing_mask_list,
                                                    image_token, facial_token, max_num_facials, num_id_images)

    def __call__(self, prompt=None, prompt_2=None, height=None, width=None, num_inference_steps: int = 50,
                 denoising_end=None, guidance_scale: float = 7.5, negative_prompt=None, negative_prompt_2=None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback=None, callback_steps: int = 1, cross_attention_kwargs=None, guidance_rescale: float = 0.0,
                 original_size=None, crops_coords_top_left=(0, 0), target_size=None, input_id_images=None,
                 start_merge_step: int = 0, class_tokens_mask=None, prompt_embeds_text_only=None,
                 pooled_prompt_embeds_text_only=None, add_time_ids: Optional[torch.Tensor] = None,
                 negative_prompt_embeds_facial: Optional[torch.Tensor] = None,
                 variance_noise: Optional[torch.Tensor] = None, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 sag_scale: float = 0.0):
        """``pag_scale`` / ``pag_adaptive_scale``: perturbed-attention guidance (``enable_pag``) -- the perturbed
        rows take the conditional rows' pooled embeds and time ids.
        ``sag_scale``: self-attention guidance -- the second evaluation takes the unconditional rows' context
        (the post-merge null set once merged), pooled embeds and time ids.
        pooled_prompt_embeds = pooled embeds used AFTER the merge step, pooled_prompt_embeds_text_only
        BEFORE it, negative_pooled_prompt_embeds for the unconditional half (ref SDXL :620-631);
        add_time_ids [2B, 6] (ref :531-539).  ``guidance_rescale``: diffusers' rescale_noise_cfg, which the reference's loop
        has commented out (ref SDXL :652-654); honoured here, 0 = the reference's behaviour."""
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        pag_kw = self._check_pag(pag_scale, pag_adaptive_scale, guidance_rescale, sag_scale)
        self._check_hot_path_inputs(prompt, input_id_images, prompt_embeds, latents, output_type)
        assert guidance_scale >= 1.0
        variance_noise = self._variance_noise(eta, generator, variance_noise, latents, num_inference_steps)
        # The SDXL loop has TWO unconditional sets (ref SDXL :586-590, :620-631): cat([negative text embeds, uncond ID
        # tokens]) up to start_merge_step, cat([FacialEncoder(negative embeds), uncond ID tokens]) afterwards.
        # prompt_embeds = cat([null_text_only, augmented, text_only, null_facial]) (4B rows); with 3B rows the one null
        # serves both phases (the SD1.5 convention).  negative_prompt_embeds_facial overrides / supplies the second one.
        null_post = negative_prompt_embeds_facial
        if prompt_embeds.shape[0] % 4 == 0 and prompt_embeds.shape[0] // 4 == latents.shape[0]:
            null_e, aug_e, text_e, null_post4 = prompt_embeds.chunk(4)
            null_post = null_post if null_post is not None else null_post4
        else:
            null_e, aug_e, text_e = self._split(prompt_embeds)
        if negative_prompt_embeds is not None:
            # ref SDXL :586-590: negative_prompt_embeds_text_only = cat([negative_prompt_embeds, uncond_prompt_tokens_faceid],
            # dim=1) is the unconditional set up to start_merge_step.  Raw [B, 77, Dc] negative embeds get the unconditional
            # ID tokens appended here -- the trailing num_tokens rows of the null set in prompt_embeds ARE those tokens
            # (ref :582-583: every unconditional set ends with uncond_prompt_tokens_faceid); [B, 77 + 4, Dc] is taken as is.
            neg = negative_prompt_embeds.to(null_e.device, null_e.dtype)
            nt = self.num_tokens
            if neg.shape[1] == null_e.shape[1] - nt:
                neg = torch.cat([neg, null_e[:, -nt:]], dim=1)
            if neg.shape != null_e.shape:
                raise ValueError(f"negative_prompt_embeds {tuple(negative_prompt_embeds.shape)}: expected [B, {null_e.shape[1] - nt}"
                                 f" or {null_e.shape[1]}, {null_e.shape[2]}]")
            if null_post is None:
                null_post = null_e      # after the merge the reference keeps FacialEncoder(negative): the assembled null set
            null_e = neg
        if add_time_ids is None:
            H, W = latents.shape[-2] * 8, latents.shape[-1] * 8
            add_time_ids = torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32).repeat(2 * latents.shape[0], 1)
        out = self._engine.run(latents, null_e, aug_e, text_e, num_inference_steps=num_inference_steps,
                               guidance_scale=guidance_scale, start_merge_step=start_merge_step, null_embeds_post=null_post,
                               pooled=(negative_pooled_prompt_embeds, pooled_prompt_embeds_text_only,
                                       pooled_prompt_embeds), time_ids=add_time_ids,
                               callback=callback, callback_steps=callback_steps, eta=eta, variance_noise=variance_noise,
                               guidance_rescale=guidance_rescale, **pag_kw)
        out = self._postprocess(out, output_type)
        if not return_dict:
            return (out,)
        return StableDiffusionXLPipelineOutput(images=out)


class StableDiffusionInpaintConsistentIDPipeline(_IDPreLoop, _SD15PromptEncoding, _BasePipeline):
    default_guidance = 7.5

    def _call_inputs(self, prompt, input_id_images, prompt_embeds, negative_prompt, num_images_per_prompt, image, mask_image,
                     height, width, max_embeddings_multiples: int = 1):
        """What the reference does between its arguments and the VAE encode (inpaint ref :127-239, CN :180-265): the ID
        pre-loop on ``input_id_images[0]`` for ``prompt`` + ``input_id_images``, and image_prep.py for PIL images.  The init
        image is ``image`` when given, else ``input_id_images[0]`` (ref :157, :232-234); PIL inputs are brought to ``height``
        x ``width`` -- by default the size of a tensor given beside them, else ``unet.config.sample_size * 8`` (ref
        :127-128).  Float tensors pass through untouched.  Returns (prompt_embeds, image, mask_image, height, width,
        normalize): ``normalize`` is False for an image that image_prep already put in [-1, 1], None for a tensor."""
        from . import image_prep
        id_call = self._takes_id_pre_loop(prompt, input_id_images, prompt_embeds)
        if id_call and image is None and mask_image is not None:
            image = input_id_images[0] if isinstance(input_id_images, (list, tuple)) else input_id_images
        normalize = None
        if image_prep.is_pil(image) or image_prep.is_pil(mask_image):
            given = [t for t in (image, mask_image) if torch.is_tensor(t)]
            side = self.unet.config.sample_size * self.vae_scale_factor
            height = height or (given[0].shape[-2] if given else side)
            width = width or (given[0].shape[-1] if given else side)
            if image_prep.is_pil(image):
                image, normalize = image_prep.preprocess_image(image, height, width), False
            if image_prep.is_pil(mask_image):
                mask_image = image_prep.preprocess_mask(mask_image, height, width)
            height, width = (image if torch.is_tensor(image) else mask_image).shape[-2:]
        if id_call:
            prompt_embeds = self._id_call_prompt_embeds(prompt, input_id_images, negative_prompt, num_images_per_prompt,
                                                        max_embeddings_multiples)
        return prompt_embeds, image, mask_image, height, width, normalize

    def _strength_window(self, strength: float, num_inference_steps: int, latents, image_latents, noise):
        """get_timesteps + prepare_latents of the inpaint pipelines (inpaint ref :246-252, :258-275; diffusers 0.23):
        the loop runs the LAST int(S * strength) schedule entries; user-supplied ``latents`` are the initial noise
        (x init_noise_sigma) whatever the strength, without them the start is pure noise at strength 1 and
        add_noise(image_latents, noise, first timestep) below it.  Returns (first_step, initial latents, scale flag)."""
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength must be in (0, 1], got {strength}")
        S = num_inference_steps
        first = max(S - min(int(S * strength), S), 0)
        if first >= S:      # diffusers: "After adjusting the num_inference_steps by strength parameter: ... < 1"
            raise ValueError(f"strength {strength} with {S} inference steps leaves no denoising step")
        if latents is not None:
            return first, latents, True
        if noise is not None and strength == 1.0:
            return first, noise, True          # pure noise: no image latents needed (a 9-channel UNet has none here)
        if noise is None or image_latents is None:
            raise ValueError("without latents the inpaint pipelines need image_latents and noise")
        self.scheduler.set_timesteps(S)
        ca, cn_ = self.scheduler.add_noise_coefficients(self.scheduler.timesteps[first])
        return first, ca * image_latents.float() + cn_ * noise.float(), False

    def _encode_images(self, image, mask_image, height, width, latents, strength, generator, prompt_embeds, explicit,
                       normalize=None):
        """``image=`` / ``mask_image=`` -> (image_latents, noise, mask_latents, masked_image_latents): the pre-loop of inpaint ref
        :231-295 (CN :254-356) on the HIP encoder.  The mask is binarised at 0.5, masked_image = image * (mask < 0.5); the
        image is normalised (2x - 1) unless ``image.min() < 0`` (diffusers VaeImageProcessor) or ``normalize`` says whether
        it still has to be (False for what image_prep.preprocess_image returns); both images go through ONE
        encoder pass; latents = scaling_factor * latent_dist.sample(generator) with the draws of ``inpaint_draws``; image /
        mask latents are repeated to the batch like diffusers does.  Given ``latents`` are also the blend noise (diffusers
        prepare_latents: ``noise = latents``)."""
        if any(v is not None for v in explicit.values()):
            raise ValueError(f"pass either image / mask_image or pre-computed {sorted(k for k, v in explicit.items() if v is not None)}, "
                             "not both")
        if image is None or mask_image is None:
            raise ValueError("image= (the init image) and mask_image= come together")
        if not (torch.is_tensor(image) and torch.is_tensor(mask_image)):
            raise NotImplementedError("image / mask_image: PIL images (resized by image_prep.py) or float tensors image "
                                      "[B, 3, H, W] and mask_image [B, 1, H, W]; numpy arrays are not taken")
        if self.vae_encoder is None:
            raise ValueError("image= / mask_image= need a VAE encoder: build the pipeline with vae_encoder=HipVAEEncoder(...) "
                             "or HipAutoencoderTinyEncoder(...), or set pipe.vae_encoder (from_pretrained builds one when "
                             "vae/ holds encoder weights)")
        enc = self.vae_encoder
        img = image.unsqueeze(0) if image.dim() == 3 else image
        msk = mask_image
        while msk.dim() < 4:
            msk = msk.unsqueeze(0)
        if img.dim() != 4 or img.shape[1] != 3 or not img.is_floating_point():
            raise ValueError(f"image must be a float tensor [B, 3, H, W] or [3, H, W], got {tuple(image.shape)} {image.dtype}")
        if msk.dim() != 4 or msk.shape[1] != 1:
            raise ValueError(f"mask_image must be [B, 1, H, W], [1, H, W] or [H, W], got {tuple(mask_image.shape)}")
        H, W = img.shape[-2:]
        height, width = height or H, width or W
        if (height, width) != (H, W) or tuple(msk.shape[-2:]) != (H, W):
            raise ValueError(f"image {tuple(img.shape[-2:])}, mask {tuple(msk.shape[-2:])} and height x width {(height, width)} "
                             "must agree: images are not resized here")
        Bi = img.shape[0]
        if msk.shape[0] not in (1, Bi):
            raise ValueError(f"mask batch {msk.shape[0]} must be 1 or the image batch {Bi}")
        B = prompt_embeds.shape[0] // 3 if prompt_embeds is not None else Bi
        if B % Bi or B % msk.shape[0]:
            raise ValueError(f"batch {B} is not a multiple of the image batch {Bi} / mask batch {msk.shape[0]}")
        cin = getattr(self.unet.config, "in_channels", 4)
        L = enc.config.latent_channels
        if normalize is None:
            normalize = not bool(img.min() < 0)                 # diffusers: "already in [-1, 1]" tensors are left alone
        eps_img, noise, eps_msk = inpaint_draws(generator, image_batch=Bi, batch_size=B, latent_channels=L, h=H // 8,
                                                w=W // 8, unet_channels=cin, latents_given=latents is not None,
                                                strength=strength, device=self.device)
        enc_img = eps_img is not None
        enc_msk = cin != 4                     # a 4-channel UNet ignores the masked image: its draw is consumed, no encode
        r = enc.encode_inpaint(img, msk.float(), normalize=normalize, encode_image=enc_img, encode_masked=enc_msk,
                               eps_image=eps_img, eps_masked=eps_msk if enc_msk else None)
        rep = lambda t: None if t is None else t.repeat(B // t.shape[0], 1, 1, 1)
        if latents is not None:
            noise = latents
        return rep(r["image_latents"]), noise, rep(r["mask_latents"]), rep(r["masked_image_latents"])

    def _unet_extra(self, latents, mask_latents, masked_image_latents):
        """9-channel inpainting UNets (``unet.config.in_channels == 9``): the per-step
        ``torch.cat([latent_model_input, mask, masked_image_latents], dim=1)`` (inpaint ref :320-321, CN :415-416).  Returns
        cat([mask, masked_image_latents]) [B, 5, h, w] for conv_in's second source, None for 4-channel UNets (which ignore
        masked_image_latents like the reference does)."""
        cin = getattr(self.unet.config, "in_channels", 4)
        if cin == 4:
            return None
        if cin != 9:
            raise ValueError(f"inpainting UNets have 4 or 9 input channels, this one has {cin}")
        if mask_latents is None or masked_image_latents is None:
            raise ValueError("a 9-channel inpainting UNet needs mask_latents [B,1,h,w] and masked_image_latents [B,4,h,w]")
        B = latents.shape[0]
        m = mask_latents.to(self.device, torch.float16).expand(B, 1, *latents.shape[-2:])
        mi = masked_image_latents.to(self.device, torch.float16).expand(B, -1, -1, -1)
        if m.shape[1] + mi.shape[1] + latents.shape[1] != cin:    # the reference's check (inpaint ref :285-293)
            raise ValueError(f"latents {latents.shape[1]} + mask {m.shape[1]} + masked image {mi.shape[1]} channels != {cin}")
        return torch.cat([m, mi], dim=1).contiguous()

    @staticmethod
    def _blend_inputs(extra, mask_latents, image_latents, noise):
        """The per-step ``latents = (1 - mask) * noised_init + mask * latents`` exists only for 4-channel UNets:
        ``if num_channels_unet == 4`` (inpaint ref :340-353, CN :437-449) and ``return_image_latents = num_channels_unet
        == 4`` (inpaint ref :258, CN :319) -- a 9-channel UNet sees the mask through its input channels and its loop
        neither blends nor has image latents.  Returns the engine's (inpaint_mask, inpaint_init, inpaint_noise)."""
        if extra is not None or mask_latents is None:
            return None, None, None
        if image_latents is None or noise is None:
            raise ValueError("inpainting with a 4-channel UNet blends every step (inpaint ref :340-353): image_latents and "
                             "noise are required beside mask_latents")
        return mask_latents, image_latents, noise

    def __call__(self, prompt=None, image=None, mask_image=None, masked_image_latents=None, height=None, width=None,
                 strength: float = 1.0, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt=None, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents=None, prompt_embeds=None, negative_prompt_embeds=None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, callback=None, callback_steps: int = 1, cross_attention_kwargs=None,
                 input_id_images=None, start_merge_step: int = 0, class_tokens_mask=None,
                 prompt_embeds_text_only=None, image_latents: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None, mask_latents: Optional[torch.Tensor] = None,
                 down_block_res_samples=None, mid_block_res_sample=None, variance_noise: Optional[torch.Tensor] = None,
                 max_embeddings_multiples: int = 1, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 sag_scale: float = 0.0, guidance_rescale: float = 0.0):
        """``pag_scale`` / ``pag_adaptive_scale``: perturbed-attention guidance (``enable_pag``), not together
        with precomputed ControlNet residuals.  ``sag_scale``: self-attention guidance, under the same condition.
        ``guidance_rescale`` / ``max_embeddings_multiples``: engine extensions here (diffusers' inpaint pipelines do not take
        them), as in ConsistentIDStableDiffusionPipeline.__call__.  The reference's call, ``pipe(prompt, input_id_images=face, mask_image=mask, height=, width=, ...)``, runs its whole
        pre-loop: the ID pre-loop on ``input_id_images[0]`` (prepare_id_prompt_embeds; ref :157-229), image_prep.py on the
        PIL init image and mask (ref :232-239), the VAE encode on ``vae_encoder`` (ref :255-291).  ``prompt_embeds``
        (cat([null, augmented, text_only])) replaces the first part; the pre-computed ``image_latents`` (init latents),
        ``noise``, ``mask_latents`` [B,1,h,w] (1 = repaint) and ``masked_image_latents`` replace the rest.
        The INIT image is ``image`` when given, else ``input_id_images[0]``, where the reference reads it (ref :157,
        :232-235; it ignores its own ``image`` argument).  PIL images (one, or a list) are converted to RGB / L and resized
        to ``height`` x ``width`` (default ``unet.config.sample_size * 8``, each rounded down to a multiple of 8).  Float
        tensors are taken as they are, without resizing: ``image`` [B, 3, H, W] / [3, H, W] in [0, 1] (or already in
        [-1, 1]), ``mask_image`` [B, 1, H, W] / [1, H, W] / [H, W], binarised at 0.5 (1 = repaint), H, W = height, width.
        ``generator`` seeds the posterior samples and the noise in diffusers' order.  ``num_images_per_prompt`` = n on the
        prompt path: n samples of the one identity (embeds and image latents repeated, noise one draw of [n, C, h, w])."""
        return self._inpaint(prompt=prompt, image=image, mask_image=mask_image, masked_image_latents=masked_image_latents,
                             height=height, width=width, strength=strength, num_inference_steps=num_inference_steps,
                             guidance_scale=guidance_scale, negative_prompt=negative_prompt,
                             num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator, latents=latents,
                             prompt_embeds=prompt_embeds, output_type=output_type, return_dict=return_dict,
                             callback=callback, callback_steps=callback_steps, input_id_images=input_id_images,
                             start_merge_step=start_merge_step, image_latents=image_latents, noise=noise,
                             mask_latents=mask_latents, down_block_res_samples=down_block_res_samples,
                             mid_block_res_sample=mid_block_res_sample, variance_noise=variance_noise,
                             guidance_rescale=guidance_rescale, max_embeddings_multiples=max_embeddings_multiples,
                             pag_scale=pag_scale, pag_adaptive_scale=pag_adaptive_scale, sag_scale=sag_scale)

    def _inpaint(self, *, prompt, image, mask_image, masked_image_latents, height, width, strength, num_inference_steps,
                 guidance_scale, negative_prompt, num_images_per_prompt, eta, generator, latents, prompt_embeds,
                 output_type, return_dict, callback, callback_steps, input_id_images, start_merge_step, image_latents,
                 noise, mask_latents, down_block_res_samples, mid_block_res_sample, variance_noise, control=None,
                 max_embeddings_multiples: int = 1, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 sag_scale: float = 0.0, guidance_rescale: float = 0.0):
        """The body both inpaint ``__call__``s share (inpaint ref :127-359, CN :180-456).  ``control``: the ControlNet
        pipeline's (control_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end)."""
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        if check_pag(pag_scale, pag_adaptive_scale)[0] > 0.0 and (control is not None or down_block_res_samples is not None
                                                                  or mid_block_res_sample is not None):
            raise NotImplementedError("PAG with ControlNet residuals is not built: the ControlNet-inpaint pipeline and "
                                      "precomputed residuals take pag_scale = 0")
        refuse_sag_with(check_sag(sag_scale), residuals=control is not None or down_block_res_samples is not None
                        or mid_block_res_sample is not None)
        pag_kw = self._check_pag(pag_scale, pag_adaptive_scale, guidance_rescale, sag_scale)
        prompt_embeds, image, mask_image, height, width, normalize = self._call_inputs(
            prompt, input_id_images, prompt_embeds, negative_prompt, num_images_per_prompt, image, mask_image, height, width,
            max_embeddings_multiples)
        if image is not None or mask_image is not None:
            image_latents, noise, mask_latents, masked_image_latents = self._encode_images(
                image, mask_image, height, width, latents, strength, generator, prompt_embeds,
                dict(image_latents=image_latents, noise=noise, mask_latents=mask_latents,
                     masked_image_latents=masked_image_latents), normalize)
        first, latents, scaled = self._strength_window(strength, num_inference_steps, latents, image_latents, noise)
        self._check_hot_path_inputs(None, None, prompt_embeds, latents, output_type)    # (_call_inputs took prompt / ID images)
        extra = self._unet_extra(latents, mask_latents, masked_image_latents)
        cn_kw = {}
        if control is not None:
            if control[0] is not None and self.controlnet is not None and down_block_res_samples is not None:
                raise ValueError("pass either control_image (native ControlNet) or precomputed residuals")
            cn_kw = prepare_control_arguments(self.controlnet, *control, [n * self.vae_scale_factor for n in latents.shape[-2:]])
        null_e, aug_e, text_e = self._split(prompt_embeds)
        b_mask, b_init, b_noise = self._blend_inputs(extra, mask_latents, image_latents, noise)
        variance_noise = self._variance_noise(eta, generator, variance_noise, latents, num_inference_steps, first)
        out = self._engine.run(latents, null_e, aug_e, text_e, num_inference_steps=num_inference_steps,
                               guidance_scale=guidance_scale, start_merge_step=start_merge_step,
                               down_residuals=down_block_res_samples, mid_residual=mid_block_res_sample,
                               inpaint_mask=b_mask, inpaint_init=b_init, inpaint_noise=b_noise,
                               callback=callback, callback_steps=callback_steps, first_step=first, scale_initial=scaled,
                               unet_extra=extra, eta=eta, variance_noise=variance_noise, guidance_rescale=guidance_rescale,
                               **pag_kw, **cn_kw)
        out, has_nsfw_concept = self._postprocess_checked(out, output_type)
        return self._output(out, return_dict, has_nsfw_concept)


class StableDiffusionControlNetInpaintConsistentIDPipeline(StableDiffusionInpaintConsistentIDPipeline):
    """ControlNet-inpaint loop (pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:375-456).

    With a ``controlnet`` (``consistentid_amd.controlnet.HipControlNet``) and a ``control_image`` [B, 3, 8h, 8w] the
    ControlNet encoder runs natively inside every captured step: on the B conditional latents, with the conditional
    embeds of the step (text-only up to ``start_merge_step``, augmented afterwards) seen through default attention
    (CN :389-396, :405-412), residuals scaled by ``controlnet_conditioning_scale`` x the keep window (CN :364-371).
    Precomputed residuals (``down_block_res_samples`` token-major [B, HW_i, C_i] x 12, ``mid_block_res_sample``) are
    still accepted instead.  Either way the reference adds batch-B residuals to the batch-2B UNet by broadcasting at
    B = 1 (CN :418-425) -- the SAME residual for the uncond and cond halves; cid_add_inplace_f16 reproduces that as
    y[i] += a[i mod len(a)]."""

    def __init__(self, unet: HipUNet, controlnet=None, scheduler: Optional[DDIMScheduler] = None, **kw):
        """``controlnet``: a ``HipControlNet``, a ``HipMultiControlNet``, or a list / tuple of 1..4 ``HipControlNet``s, which
        becomes a ``HipMultiControlNet`` (as diffusers wraps a list in a MultiControlNetModel)"""
        super().__init__(unet, scheduler, **kw)
        if isinstance(controlnet, (list, tuple)):
            controlnet = HipMultiControlNet(controlnet)
        self.controlnet = controlnet

    def __call__(self, prompt=None, image=None, mask_image=None, control_image=None, height=None, width=None,
                 strength: float = 1.0, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt=None, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents=None, prompt_embeds=None, negative_prompt_embeds=None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, cross_attention_kwargs=None, original_size=None, target_size=None,
                 callback=None, callback_steps: int = 1,
                 controlnet_conditioning_scale: Union[float, List[float]] = 0.5, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0,
                 control_guidance_end: Union[float, List[float]] = 1.0,
                 input_id_images=None, start_merge_step: int = 0, class_tokens_mask=None, prompt_embeds_text_only=None,
                 image_latents: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                 mask_latents: Optional[torch.Tensor] = None, down_block_res_samples=None, mid_block_res_sample=None,
                 masked_image_latents: Optional[torch.Tensor] = None, variance_noise: Optional[torch.Tensor] = None,
                 max_embeddings_multiples: int = 1, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 sag_scale: float = 0.0, guidance_rescale: float = 0.0):
        """``pag_scale`` > 0 and ``sag_scale`` > 0 are refused here (NotImplementedError): neither is built with ControlNet residuals.
        ``prompt`` / ``input_id_images`` / ``image`` / ``mask_image`` / ``guidance_rescale`` / ``max_embeddings_multiples``: as in
        StableDiffusionInpaintConsistentIDPipeline.__call__ (CN :180-265).  ``control_image``: a float tensor [B, 3, 8h, 8w]
        in [0, 1], or one PIL image (or a list of one), converted to RGB and resized to the final height x width by
        image_prep.preprocess_control (CN :267-280).
        Built with a list of ControlNets (``controlnet=HipMultiControlNet([...])``, or a list given to ``from_pretrained``),
        the pipeline takes the reference's MultiControlNet arguments (CN :139-149, :281-301, :363-370, :397-398):
        ``control_image`` is a list with one item per net, each a PIL image, a list of one PIL image or a float tensor
        [B or 1, 3, 8h, 8w]; ``controlnet_conditioning_scale`` a list of N floats, or one float for all nets as in diffusers'
        own ControlNet pipelines (the reference itself would fail on a float there: its ``zip`` at CN :398 needs a list);
        ``control_guidance_start`` / ``control_guidance_end`` floats or lists of N, aligned as CN :139-149.  A net runs only in
        the steps of its window.  Mismatched lengths raise ValueError.  A pipeline built with ONE ControlNet refuses several
        control images (NotImplementedError).  ``guess_mode`` is not forwarded, as in the reference."""
        return self._inpaint(prompt=prompt, image=image, mask_image=mask_image, masked_image_latents=masked_image_latents,
                             height=height, width=width, strength=strength, num_inference_steps=num_inference_steps,
                             guidance_scale=guidance_scale, negative_prompt=negative_prompt,
                             num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator, latents=latents,
                             prompt_embeds=prompt_embeds, output_type=output_type, return_dict=return_dict,
                             callback=callback, callback_steps=callback_steps, input_id_images=input_id_images,
                             start_merge_step=start_merge_step, image_latents=image_latents, noise=noise,
                             mask_latents=mask_latents, down_block_res_samples=down_block_res_samples,
                             mid_block_res_sample=mid_block_res_sample, variance_noise=variance_noise,
                             control=(control_image, controlnet_conditioning_scale, control_guidance_start,
                             control_guidance_end), guidance_rescale=guidance_rescale,
                             max_embeddings_multiples=max_embeddings_multiples, pag_scale=pag_scale,
                             pag_adaptive_scale=pag_adaptive_scale, sag_scale=sag_scale)
