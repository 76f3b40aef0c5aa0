"""Base-model loader: a diffusers model directory on disk -> the HIP engines.

The reference builds its pipelines with ``ConsistentIDPipeline.from_pretrained(base_model_path, torch_dtype=torch.float16)``
(/root/reference/infer.py:17-21, infer_SDXL.py:19-25) -- diffusers' loader reading ``model_index.json`` and one
sub-folder per component.  This module reads the components the hot path needs, straight from their files:

    <root>/unet/config.json + diffusion_pytorch_model.{safetensors,bin}     -> HipUNet      (required)
    <root>/vae/config.json  + diffusion_pytorch_model.{safetensors,bin}     -> HipVAEDecoder (optional; + HipVAEEncoder for the
                                                                             inpaint pipelines when encoder.* weights are there);
                                                                             a config whose _class_name is AutoencoderTiny
                                                                             -> HipAutoencoderTiny (the decoder; +
                                                                             HipAutoencoderTinyEncoder for the inpaint
                                                                             pipelines when encoder.* weights are there)
    <taesd dir>/config.json + diffusion_pytorch_model.{safetensors,bin}     -> HipAutoencoderTiny (load_tiny_vae: the local
                                                                             AutoencoderTiny.from_pretrained(path)) and
                                                                             HipAutoencoderTinyEncoder (load_tiny_vae_encoder:
                                                                             its encode half, for pipe.vae_encoder)
    <controlnet dir>/config.json + diffusion_pytorch_model.{safetensors,bin} -> HipControlNet (separate call, like the
                                                                                reference: demo/controlnet_demo.py:44-47)
    <root>/text_encoder{,_2}/config.json + model{.fp16,}.safetensors | pytorch_model{.fp16,}.bin
                                                                          -> HipCLIPTextModel (optional; transformers names)
    <root>/tokenizer{,_2}/                                                -> transformers.CLIPTokenizer (optional)
    <root>/safety_checker/config.json + model{.fp16,}.safetensors | pytorch_model{.fp16,}.bin
                                                                          -> HipSafetyChecker (optional; SD1.5 family only)
    <root>/feature_extractor/preprocessor_config.json                     -> settings of face_prep.clip_preprocess (optional)

Local files only (there is no hub access in the engine), ``.fp16`` variants are picked up, sharded checkpoints are
not.
``scheduler/scheduler_config.json`` is read for its betas / steps_offset / timestep spacing (the engine carries its own
DDIM / Euler coefficient tables, scheduler.py; the base model's sampler class itself is not built).

Host Python + file IO; the tensors go to the GPU inside the engines' weight packers.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from .unet_spec import UNetConfig
from .vae_spec import VAEConfig

WEIGHT_NAMES = ("diffusion_pytorch_model.fp16.safetensors", "diffusion_pytorch_model.safetensors",
                "diffusion_pytorch_model.fp16.bin", "diffusion_pytorch_model.bin")


# transformers' file names (text_encoder/, text_encoder_2/), not diffusers' WEIGHT_NAMES
TEXT_WEIGHT_NAMES = ("model.fp16.safetensors", "model.safetensors", "pytorch_model.fp16.bin", "pytorch_model.bin")
TEXT_COMPONENTS = ("text_encoder", "tokenizer", "text_encoder_2", "tokenizer_2")


def _tup(v, n) -> Tuple[int, ...]:
    return tuple(v) if isinstance(v, (list, tuple)) else (int(v),) * n


def unet_config_from_diffusers(cfg: Dict) -> UNetConfig:
    """``unet/config.json`` (diffusers UNet2DConditionModel / ControlNetModel) -> UNetConfig.

    diffusers 0.23 quirk kept: ``num_attention_heads = num_attention_heads or attention_head_dim`` -- for the SD1.5 and
    SDXL checkpoints the field called attention_head_dim holds the head COUNT per level (8 / [5, 10, 20])."""
    boc = tuple(cfg["block_out_channels"])
    n = len(boc)
    heads = cfg.get("num_attention_heads") or cfg.get("attention_head_dim", 8)
    down = tuple(cfg.get("down_block_types", ("CrossAttnDownBlock2D",) * (n - 1) + ("DownBlock2D",)))
    up = cfg.get("up_block_types")
    if up is None:      # ControlNet configs have no decoder: mirror the encoder so that the shared topology walk works
        up = tuple("CrossAttnUpBlock2D" if t.startswith("CrossAttn") else "UpBlock2D" for t in reversed(down))
    for t in tuple(down) + tuple(up):
        if t not in ("CrossAttnDownBlock2D", "DownBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"):
            raise NotImplementedError(f"block type {t}: only the SD1.5 / SDXL UNet topologies are built")
    if cfg.get("mid_block_type", "UNetMidBlock2DCrossAttn") != "UNetMidBlock2DCrossAttn":
        raise NotImplementedError(f"mid block {cfg['mid_block_type']}")
    expected = {"class_embed_type": (None,), "encoder_hid_dim": (None,), "only_cross_attention": (False, None),
                "dual_cross_attention": (False, None), "upcast_attention": (False, None),
                "resnet_time_scale_shift": ("default", None), "time_embedding_type": ("positional", None),
                "act_fn": ("silu", None), "class_embeddings_concat": (False, None), "conv_in_kernel": (3, None),
                "conv_out_kernel": (3, None), "flip_sin_to_cos": (True, None), "freq_shift": (0, None)}
    for key, ok in expected.items():
        if cfg.get(key) not in ok:
            raise NotImplementedError(f"UNet config {key}={cfg[key]!r} is outside the SD1.5 / SDXL geometry the engine builds")
    add = cfg.get("addition_embed_type")
    if add not in (None, "text_time"):
        raise NotImplementedError(f"addition_embed_type {add!r}")
    return UNetConfig(
        sample_size=int(cfg.get("sample_size", 64)), in_channels=int(cfg.get("in_channels", 4)),
        out_channels=int(cfg.get("out_channels", 4)), block_out_channels=boc, down_block_types=down, up_block_types=tuple(up),
        layers_per_block=int(cfg.get("layers_per_block", 2)),
        transformer_layers_per_block=_tup(cfg.get("transformer_layers_per_block", 1), n),
        num_attention_heads=_tup(heads, n), cross_attention_dim=int(cfg.get("cross_attention_dim", 768)),
        norm_num_groups=int(cfg.get("norm_num_groups", 32)), norm_eps=float(cfg.get("norm_eps", 1e-5)),
        use_linear_projection=bool(cfg.get("use_linear_projection", False)), addition_embed_type=add,
        addition_time_embed_dim=cfg.get("addition_time_embed_dim"),
        projection_class_embeddings_input_dim=cfg.get("projection_class_embeddings_input_dim"),
        time_cond_proj_dim=None if cfg.get("time_cond_proj_dim") is None else int(cfg["time_cond_proj_dim"]),
        family="sdxl" if add == "text_time" else "sd15")


def vae_config_from_diffusers(cfg: Dict) -> VAEConfig:
    return VAEConfig(in_channels=int(cfg.get("in_channels", 3)), out_channels=int(cfg.get("out_channels", 3)),
                     latent_channels=int(cfg.get("latent_channels", 4)), block_out_channels=tuple(cfg["block_out_channels"]),
                     layers_per_block=int(cfg.get("layers_per_block", 2)), norm_num_groups=int(cfg.get("norm_num_groups", 32)),
                     scaling_factor=float(cfg.get("scaling_factor", 0.18215)), force_upcast=bool(cfg.get("force_upcast", False)))


def read_component(folder: Union[str, os.PathLike], weight_names: Sequence[str] = WEIGHT_NAMES
                   ) -> Tuple[Dict, Dict[str, torch.Tensor]]:
    """(config.json as dict, state_dict on the CPU) of one diffusers component folder (``weight_names``: the files
    tried in order; TEXT_WEIGHT_NAMES for the transformers text encoders)"""
    folder = os.fspath(folder)
    cpath = os.path.join(folder, "config.json")
    if not os.path.isfile(cpath):
        raise FileNotFoundError(f"{cpath}: not a diffusers component folder (the engine reads local files only)")
    with open(cpath) as f:
        cfg = json.load(f)
    for name in weight_names:
        wpath = os.path.join(folder, name)
        if os.path.isfile(wpath):
            break
    else:
        if os.path.isfile(os.path.join(folder, weight_names[1] + ".index.json")):     # (the plain .safetensors name)
            raise NotImplementedError(f"{folder}: sharded checkpoints are not read; merge the shards first")
        raise FileNotFoundError(f"{folder}: none of {tuple(weight_names)}")
    if wpath.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(wpath, device="cpu")
    else:
        sd = torch.load(wpath, map_location="cpu", weights_only=True)
    return cfg, sd


def load_unet(root: Union[str, os.PathLike], device="cuda:0", subfolder: str = "unet", keep_base: bool = True, **kw):
    """-> HipUNet.  ``keep_base`` keeps the un-merged attention weights so that ``load_ConsistentID_model`` can merge a
    ConsistentID checkpoint afterwards (the reference's order: from_pretrained, then load_ConsistentID_model)."""
    from .unet import HipUNet
    cfg, sd = read_component(os.path.join(os.fspath(root), subfolder) if subfolder else root)
    return HipUNet(unet_config_from_diffusers(cfg), sd, None, device=device, keep_base=keep_base, **kw)


def load_controlnet(folder, device="cuda:0"):
    """a ControlNetModel folder -> HipControlNet; a list / tuple of folders and / or HipControlNets -> HipMultiControlNet
    (diffusers wraps a list of ControlNets in a MultiControlNetModel in the same way)"""
    from .controlnet import HipControlNet, HipMultiControlNet, check_controlnet_count
    if isinstance(folder, (list, tuple)):
        check_controlnet_count(len(folder))         # before anything is read
        return HipMultiControlNet([load_controlnet(f, device=device) if isinstance(f, (str, os.PathLike)) else f
                                   for f in folder])
    cfg, sd = read_component(folder)
    return HipControlNet(unet_config_from_diffusers(cfg), sd, device=device)


def is_tiny_vae(cfg: Dict) -> bool:
    """a ``vae/config.json`` of diffusers' AutoencoderTiny (TAESD / taesdxl) rather than AutoencoderKL"""
    return cfg.get("_class_name") == "AutoencoderTiny"


def _make_decoder(cfg: Dict, sd, device):
    """the decoder engine for a ``vae/`` folder, by the config's ``_class_name``"""
    if is_tiny_vae(cfg):
        from .vae_tiny import HipAutoencoderTiny
        return HipAutoencoderTiny(cfg, sd, device=device)
    from .vae import make_vae_decoder
    return make_vae_decoder(vae_config_from_diffusers(cfg), sd, device=device)      # fp32 engine for force_upcast (SDXL)


def load_vae(root: Union[str, os.PathLike], device="cuda:0", subfolder: str = "vae"):
    cfg, sd = read_component(os.path.join(os.fspath(root), subfolder) if subfolder else root)
    return _make_decoder(cfg, sd, device)


def load_tiny_vae(folder: Union[str, os.PathLike], device="cuda:0"):
    """The local ``AutoencoderTiny.from_pretrained(path)``: a stand-alone TAESD / taesdxl folder (``config.json`` + weights,
    as ``madebyollin/taesd`` is laid out) -> HipAutoencoderTiny, for ``pipe.vae = load_tiny_vae(path)`` on any pipeline.
    Hub ids are not resolved."""
    from .vae_tiny import HipAutoencoderTiny
    cfg, sd = read_component(folder)
    if cfg.get("_class_name", "AutoencoderTiny") != "AutoencoderTiny":
        raise NotImplementedError(f"{os.fspath(folder)}: _class_name={cfg['_class_name']!r} is not AutoencoderTiny "
                                  "(load_vae reads AutoencoderKL folders)")
    return HipAutoencoderTiny(cfg, sd, device=device)


def load_tiny_vae_encoder(folder: Union[str, os.PathLike], device="cuda:0"):
    """The encode half of the same stand-alone TAESD / taesdxl folder -> HipAutoencoderTinyEncoder, for
    ``pipe.vae_encoder = load_tiny_vae_encoder(path)`` on the inpaint pipelines (beside ``pipe.vae = load_tiny_vae(path)`` or
    a KL decoder: they share a latent space).  Hub ids are not resolved."""
    from .vae_tiny import HipAutoencoderTinyEncoder
    cfg, sd = read_component(folder)
    if cfg.get("_class_name", "AutoencoderTiny") != "AutoencoderTiny":
        raise NotImplementedError(f"{os.fspath(folder)}: _class_name={cfg['_class_name']!r} is not AutoencoderTiny "
                                  "(load_vae_encoder reads AutoencoderKL folders)")
    if not _has_encoder(sd):
        raise NotImplementedError(f"{os.fspath(folder)}: the weights hold no encoder.* keys (a decoder-only AutoencoderTiny "
                                  "export); load_tiny_vae reads its decoder")
    return HipAutoencoderTinyEncoder(cfg, sd, device=device)


def load_vae_encoder(root: Union[str, os.PathLike], device="cuda:0", subfolder: str = "vae"):
    """-> HipVAEEncoder (``vae.encode`` of the inpaint pipelines' pre-loop) from the same ``vae/`` folder as the decoder."""
    from .vae import HipVAEEncoder
    cfg, sd = read_component(os.path.join(os.fspath(root), subfolder) if subfolder else root)
    return HipVAEEncoder(vae_config_from_diffusers(cfg), sd, device=device)


def load_text_encoder(folder: Union[str, os.PathLike], device="cuda:0"):
    """``text_encoder/`` or ``text_encoder_2/`` (transformers CLIPTextModel / CLIPTextModelWithProjection) -> HipCLIPTextModel,
    with the base weights kept on the host so that ``load_lora_weights`` can merge text-encoder LoRA later"""
    from .clip_text import HipCLIPTextModel
    cfg, sd = read_component(folder, TEXT_WEIGHT_NAMES)
    return HipCLIPTextModel(sd, cfg, device=device, keep_base=True)


def load_tokenizer(folder: Union[str, os.PathLike]):
    """``tokenizer/`` or ``tokenizer_2/`` -> transformers.CLIPTokenizer (local files only; transformers is imported here,
    not by the engine)"""
    from transformers import CLIPTokenizer
    return CLIPTokenizer.from_pretrained(os.fspath(folder), local_files_only=True)


def read_force_zeros(root: Union[str, os.PathLike]) -> bool:
    """SDXL's ``force_zeros_for_empty_prompt`` from ``model_index.json`` (diffusers' default True when absent)"""
    path = os.path.join(os.fspath(root), "model_index.json")
    if not os.path.isfile(path):
        return True
    with open(path) as f:
        return bool(json.load(f).get("force_zeros_for_empty_prompt", True))


def read_text_components(root: Union[str, os.PathLike], device="cuda:0", given: Optional[Dict] = None) -> Dict:
    """The text encoders and tokenizers of a model directory, by keyword: a component passed in ``given`` is kept as it
    is (None skips it, as in diffusers); the others are read from their folder when it exists."""
    given = given or {}
    out = {}
    for name in TEXT_COMPONENTS:
        if name in given:
            out[name] = given[name]
            continue
        folder = os.path.join(os.fspath(root), name)
        if os.path.isdir(folder):
            out[name] = load_tokenizer(folder) if name.startswith("tokenizer") else load_text_encoder(folder, device=device)
    return out


SAFETY_COMPONENTS = ("safety_checker", "feature_extractor")


def _edge(v, keys, what: str) -> int:
    """an image-processor size: an int, [h, w] or a dict ({"shortest_edge": n} / {"height": n, "width": n}) -> n"""
    if isinstance(v, dict):
        vals = [v[k] for k in keys if k in v]
        if not vals:
            raise NotImplementedError(f"{what}={v!r}: expected one of {keys}")
    else:
        vals = list(v) if isinstance(v, (list, tuple)) else [v]
    if len(set(int(x) for x in vals)) != 1:
        raise NotImplementedError(f"{what}={v!r}: clip_preprocess crops a square")
    return int(vals[0])


def preprocessor_settings(cfg: Dict) -> Dict:
    """A CLIPImageProcessor / CLIPFeatureExtractor config (``preprocessor_config.json``) -> {"size": n}, the one setting
    ``face_prep.clip_preprocess`` takes.  Everything else has to BE what clip_preprocess does -- shortest edge to n with
    bicubic resampling, centre crop n x n, rescale by 1 / 255, OpenAI CLIP mean / std -- or the key is named in a
    NotImplementedError.  Absent keys take transformers' CLIPImageProcessor defaults, which are exactly that (an absent
    crop_size follows size, so that the settings this function returns pass through it unchanged)."""
    from .face_prep import CLIP_MEAN, CLIP_SIZE, CLIP_STD
    for key in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if not cfg.get(key, True):
            raise NotImplementedError(f"preprocessor {key}={cfg[key]!r}: clip_preprocess always resizes, centre-crops, "
                                      "rescales and normalises")
    if cfg.get("resample", 3) != 3:
        raise NotImplementedError(f"preprocessor resample={cfg['resample']!r}: clip_preprocess resamples bicubic (3)")
    if abs(float(cfg.get("rescale_factor", 1 / 255)) - 1 / 255) > 1e-9:
        raise NotImplementedError(f"preprocessor rescale_factor={cfg['rescale_factor']!r}: clip_preprocess rescales by 1 / 255")
    for key, want in (("image_mean", CLIP_MEAN), ("image_std", CLIP_STD)):
        got = cfg.get(key, want)
        if len(got) != 3 or any(abs(float(a) - b) > 1e-6 for a, b in zip(got, want)):
            raise NotImplementedError(f"preprocessor {key}={got!r}: clip_preprocess normalises with the CLIP values {want}")
    size = _edge(cfg.get("size", CLIP_SIZE), ("shortest_edge", "height", "width"), "preprocessor size")
    crop = size if "crop_size" not in cfg else _edge(cfg["crop_size"], ("height", "width"), "preprocessor crop_size")
    if size != crop:
        raise NotImplementedError(f"preprocessor size={cfg.get('size')!r} with crop_size={cfg.get('crop_size')!r}: "
                                  "clip_preprocess crops to the size it resized the shorter edge to")
    return {"size": size}


def feature_extractor_settings(fe) -> Dict:
    """a ready ``feature_extractor=``: settings ({"size": n}), a preprocessor config dict, or a transformers image
    processor (anything with ``to_dict()``) -> ``preprocessor_settings``"""
    return preprocessor_settings(fe.to_dict() if hasattr(fe, "to_dict") else dict(fe))


def read_feature_extractor(folder: Union[str, os.PathLike]) -> Dict:
    """``feature_extractor/preprocessor_config.json`` -> ``preprocessor_settings`` (settings only: no processor is built)"""
    path = os.path.join(os.fspath(folder), "preprocessor_config.json")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: not a feature extractor folder")
    with open(path) as f:
        return preprocessor_settings(json.load(f))


def load_safety_checker(folder: Union[str, os.PathLike], device="cuda:0"):
    """``safety_checker/`` (diffusers StableDiffusionSafetyChecker, saved by transformers) -> HipSafetyChecker"""
    from .safety import HipSafetyChecker
    cfg, sd = read_component(folder, TEXT_WEIGHT_NAMES)
    return HipSafetyChecker(cfg, sd, device=device)


def read_safety_components(root: Union[str, os.PathLike], device="cuda:0", given: Optional[Dict] = None) -> Dict:
    """The safety checker and its pre-processing settings with diffusers' meaning of the keywords: a component passed in
    ``given`` is kept (None: not loaded, which is how the reference's SDXL script switches the checker off); otherwise it
    is read when its folder exists.  Without a checker the feature extractor is not read either.  A ready
    ``feature_extractor`` may be settings ({"size": n}), a preprocessor config dict, or a transformers image processor."""
    given = given or {}
    out = {}
    folder = os.path.join(os.fspath(root), "safety_checker")
    if "safety_checker" in given:
        out["safety_checker"] = given["safety_checker"]
    elif os.path.isdir(folder):
        out["safety_checker"] = load_safety_checker(folder, device=device)
    if out.get("safety_checker") is None:
        return {}
    fe = given.get("feature_extractor")
    folder = os.path.join(os.fspath(root), "feature_extractor")
    if fe is not None:
        out["feature_extractor"] = feature_extractor_settings(fe)
    elif "feature_extractor" not in given and os.path.isdir(folder):
        out["feature_extractor"] = read_feature_extractor(folder)
    return out


def _has_encoder(sd) -> bool:
    return any(k.startswith("encoder.") for k in sd)


def read_scheduler(root: Union[str, os.PathLike]):
    """``<root>/scheduler/scheduler_config.json`` -> the engine's DDIMScheduler on that config (None without the file).
    The base model's own sampler class (PNDM for SD1.5) is not built; its CONFIG is kept, so that the reference scripts' next
    line -- ``pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)`` (infer.py:33) -- sees the base
    model's betas / steps_offset / timestep spacing.  Until then the engine's DDIM runs on that config."""
    spath = os.path.join(os.fspath(root), "scheduler", "scheduler_config.json")
    if not os.path.isfile(spath):
        return None
    import warnings
    from .scheduler import DDIMScheduler, EulerDiscreteScheduler, LCMScheduler
    with open(spath) as f:
        cfg = json.load(f)
    # the base model's sampler class: SDXL base ships EulerDiscrete (built), SD1.5 PNDM (not built: DDIM on its config)
    name = cfg.get("_class_name", "DDIMScheduler")
    # a distilled latent-consistency model directory names LCMScheduler (built: few-step sampling)
    cls = {"EulerDiscreteScheduler": EulerDiscreteScheduler, "LCMScheduler": LCMScheduler}.get(name, DDIMScheduler)
    if name not in ("EulerDiscreteScheduler", "DDIMScheduler", "LCMScheduler"):
        warnings.warn(f"{name} is not built: the engine samples with DDIM on its config until pipe.scheduler is replaced "
                      "(infer.py:33 / demo/controlnet_demo.py:67 do that on the next line)")
    def make(c):
        # a v-prediction model: the saved prediction type goes on as the explicit keyword from_config asks for (a raw
        # config alone is refused there); said once, because X.from_config(<this json>) elsewhere needs the same keyword
        if c.get("prediction_type") == "v_prediction":
            sch = cls.from_config(c, prediction_type="v_prediction")
            warnings.warn(f"{spath}: a v-prediction model; {cls.__name__} samples with v-prediction coefficients, and "
                          "`Other.from_config(pipe.scheduler.config)` keeps that")
            return sch
        return cls.from_config(c)

    try:
        return make(cfg)
    except NotImplementedError as e:     # e.g. clip_sample=true of a saved DDIM default: must not block the load
        # drop ONLY the sampling modifiers the engine does not build and keep the rest of the saved config (betas,
        # steps_offset, timestep spacing); defaults only if the schedule itself (beta schedule / prediction type) is foreign
        # clip_sample / thresholding act on the predicted sample only (clip_sample clamps pred_x0 to [-1, 1], which DOES
        # change SD latents where it is on); the engine does not build them and ignores them with a warning.  use_karras_sigmas / rescale_betas_zero_snr / a non-linear interpolation_type change the sigma / alpha
        # SCHEDULE itself: a checkpoint saved with them would sample on a materially different schedule here, so that is an
        # error, not a warning.
        harmless = ("clip_sample", "thresholding")
        schedule = ("use_karras_sigmas", "interpolation_type", "rescale_betas_zero_snr")
        changed = sorted(k for k in schedule if cfg.get(k) not in (None, False, "linear"))
        if changed:
            raise NotImplementedError(f"{spath}: {changed} change the noise schedule and are not built from a saved config; the engine would not "
                                      f"reproduce the reference's samples -- pass the scheduler to use explicitly, "
                                      f"`from_pretrained(..., scheduler=DDIMScheduler(...))` (DDIMScheduler takes "
                                      f"rescale_betas_zero_snr and prediction_type as arguments; the saved config is then not "
                                      f"read; infer.py:33 replaces the loaded scheduler in the same way)") from e
        kept = {k: v for k, v in cfg.items() if k not in harmless}
        dropped = sorted(k for k in harmless if cfg.get(k) not in (None, False))
        try:
            sch = make(kept)
            warnings.warn(f"{spath}: {e}; the engine does not build {dropped} and IGNORES them (samples differ from a "
                          "scheduler that applies them); the rest of the saved scheduler config is kept")
            return sch
        except NotImplementedError as e2:
            warnings.warn(f"{spath}: {e2}; falling back to the engine's default {cls.__name__} configuration")
            return cls()


def from_pretrained(pipeline_cls, root: Union[str, os.PathLike], torch_dtype=torch.float16, device="cuda:0",
                    controlnet: Optional[Union[str, os.PathLike, object]] = None, use_graph: bool = True, **kw):
    """``Pipeline.from_pretrained(base_model_path, torch_dtype=torch.float16)`` of the reference scripts (infer.py:17-21;
    with ``controlnet=`` demo/controlnet_demo.py:44-47): UNet (required), VAE decoder, text encoders and tokenizers (when
    their folders exist) of a local diffusers model directory; ``controlnet`` = a HipControlNet or the folder of a
    ControlNetModel, or a list of those for a HipMultiControlNet.  ``text_encoder=`` / ``tokenizer=`` / ``text_encoder_2=`` / ``tokenizer_2=`` take a ready object, or
    None to skip that component.  ``safety_checker=`` / ``feature_extractor=`` likewise, for the SD1.5-family pipelines: the
    checker is loaded when ``safety_checker/`` exists and the caller did not pass ``safety_checker=None``; the SDXL pipeline
    never has one (the reference's has none).  ``vae=`` takes a built decoder engine (``load_tiny_vae(path)`` for diffusers'
    ``vae=AutoencoderTiny.from_pretrained(...)``) in place of the ``vae/`` folder's decoder; the inpaint pipelines' encoder still
    comes from that folder unless ``vae_encoder=`` gives a built one (HipVAEEncoder, or ``load_tiny_vae_encoder(path)``).  A
    ``vae/`` folder whose config names AutoencoderTiny is built as HipAutoencoderTiny, and for the two inpaint pipelines its
    ``encoder.*`` weights (when there) as HipAutoencoderTinyEncoder."""
    if torch_dtype not in (torch.float16, None):
        raise NotImplementedError("the engine computes in fp16 (the reference's own inference dtype, infer.py:19)")
    # diffusers loader keywords the reference scripts pass (infer.py:17-21 variant="fp16"; demo/controlnet_demo.py
    # use_safetensors=True): they select files the engine does not read -- the .fp16 weight files are preferred anyway and
    # there is no hub access.  safety_checker= / feature_extractor= (infer_SDXL.py safety_checker=None) are components
    for name in ("variant", "use_safetensors", "requires_safety_checker",
                 "local_files_only", "cache_dir", "revision", "low_cpu_mem_usage", "add_watermarker"):
        kw.pop(name, None)
    safety_given = {k: kw.pop(k) for k in SAFETY_COMPONENTS if k in kw}
    vae_given = "vae" in kw
    vae = kw.pop("vae", None)              # a built decoder (HipVAEDecoder / HipAutoencoderTiny ...), as diffusers takes vae=
    if vae_given and (vae is None or not hasattr(vae, "decode_latents")):
        raise TypeError(f"from_pretrained: vae= takes a built decoder engine (HipVAEDecoder, HipVAEDecoderF32, "
                        f"HipAutoencoderTiny), got {type(vae).__name__}")
    enc_given = "vae_encoder" in kw
    vae_encoder = kw.pop("vae_encoder", None)      # a built encoder (HipVAEEncoder / HipAutoencoderTinyEncoder), like vae=
    if enc_given and (vae_encoder is None or not hasattr(vae_encoder, "encode_inpaint")):
        raise TypeError(f"from_pretrained: vae_encoder= takes a built encoder engine (HipVAEEncoder, "
                        f"HipAutoencoderTinyEncoder), got {type(vae_encoder).__name__}")
    unknown = [k for k in kw if k not in ("scheduler", "num_tokens", "lora_rank") + TEXT_COMPONENTS]
    if unknown:
        raise TypeError(f"from_pretrained: unexpected keyword(s) {unknown}")
    root = os.fspath(root)
    if not os.path.isdir(root):
        raise FileNotFoundError(f"{root}: local diffusers model directory expected (no hub access)")
    unet = load_unet(root, device=device)
    if os.path.isdir(os.path.join(root, "vae")):
        from .pipeline import StableDiffusionInpaintConsistentIDPipeline
        from .vae import HipVAEEncoder
        vcfg, vsd = read_component(os.path.join(root, "vae"))
        if not vae_given:                 # a given vae= replaces the folder's DECODER only
            vae = _make_decoder(vcfg, vsd, device)
        # the encoder only for the two inpaint pipelines (their image= / mask_image= pre-loop), only if the weights are there
        # and no built one was given; by the config's _class_name like the decoder
        if (issubclass(pipeline_cls, StableDiffusionInpaintConsistentIDPipeline) and not enc_given and _has_encoder(vsd)):
            if is_tiny_vae(vcfg):
                from .vae_tiny import HipAutoencoderTinyEncoder
                vae_encoder = HipAutoencoderTinyEncoder(vcfg, vsd, device=device)
            else:
                vae_encoder = HipVAEEncoder(vae_config_from_diffusers(vcfg), vsd, device=device)
    text = read_text_components(root, device=device, given={k: kw.pop(k) for k in TEXT_COMPONENTS if k in kw})
    args = dict(use_graph=use_graph, vae=vae, **kw, **{k: v for k, v in text.items() if v is not None})
    from .pipeline import ConsistentIDStableDiffusionXLPipeline
    if issubclass(pipeline_cls, ConsistentIDStableDiffusionXLPipeline):
        args["force_zeros_for_empty_prompt"] = read_force_zeros(root)
    else:
        args.update(read_safety_components(root, device=device, given=safety_given))
    if vae_encoder is not None:
        args["vae_encoder"] = vae_encoder
    if "scheduler" not in args:
        base = read_scheduler(root)
        if base is not None:
            args["scheduler"] = base
    if controlnet is not None:
        cn = load_controlnet(controlnet, device=device) if isinstance(controlnet, (str, os.PathLike, list, tuple)) else controlnet
        return pipeline_cls(unet, controlnet=cn, **args)
    return pipeline_cls(unet, **args)
