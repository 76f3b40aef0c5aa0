"""HIP execution engine for the safety checker of the SD1.5-family pipelines.

The reference loads its base model without ``safety_checker=None`` (infer.py:17-21, app.py, both demos; only
infer_SDXL.py passes it), so every non-latent call of its three SD1.5-family pipelines runs diffusers'
``run_safety_checker`` between the VAE decode and the PIL conversion (pipline_StableDiffusion_ConsistentID.py:584-602,
pipelines/StableDIffusionInpaint_ConsistentID.py:371-381, pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:468-478),
returns ``nsfw_content_detected`` as a list of booleans and blacks out the flagged images.

``StableDiffusionSafetyChecker.forward`` (diffusers 0.23) is: CLIP ViT-L/14 vision tower (quick GELU) -> pooled output
(post_layernorm of the CLS token) -> visual_projection -> cosine against 3 special-care and 17 concept embeddings ->
a threshold loop in which a special-care hit lowers every later threshold by 0.01 -> flagged iff any concept hits ->
``images[idx] = zeros``.  Here the tower is ``HipCLIPVision`` (clip_vision.py), everything after its last encoder layer is
ONE ``cid_clip_head_f16`` launch for the whole batch, and a device tensor is blacked out by ``cid_blackout_f16`` from the
flags as they sit on the device.  The only host read is the list of booleans the caller is owed.

State-dict keys (transformers / diffusers names): ``vision_model.vision_model.*``, ``visual_projection.weight``,
``concept_embeds`` [17, P], ``special_care_embeds`` [3, P], ``concept_embeds_weights`` [17], ``special_care_embeds_weights``
[3].  The concept rows are L2-normalised once here, in fp32 (``cosine_distance`` normalises them on every call), and
stored special-care rows first, which is the order the threshold loop walks them in.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .clip_vision import HipCLIPVision

# transformers' CLIPVisionConfig defaults, for keys a config.json leaves out
VISION_DEFAULTS = {"num_attention_heads": 12, "patch_size": 32, "layer_norm_eps": 1e-5, "hidden_act": "quick_gelu"}
OUTER = "vision_model."           # CLIPVisionModel inside the checker: its keys are vision_model.vision_model.*
MAX_CONCEPTS = 64                 # cid_clip_head_f16's K limit


def tower_state_dict(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The checker's keys as ``HipCLIPVision`` reads them: ``vision_model.vision_model.X`` -> ``vision_model.X``, plus
    ``visual_projection.weight``; the concept tables stay behind."""
    inner = OUTER + OUTER
    sd = {k[len(OUTER):]: v for k, v in state_dict.items() if k.startswith(inner)}
    if not sd:
        raise KeyError(f"no {inner}* keys: not a StableDiffusionSafetyChecker state dict")
    sd["visual_projection.weight"] = state_dict["visual_projection.weight"]
    return sd


def concept_table(state_dict: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(rows fp32 [K, P], L2-normalised, special-care rows first; thresholds fp32 [K]; number of special-care rows)"""
    special, concept = state_dict["special_care_embeds"].float(), state_dict["concept_embeds"].float()
    thr = torch.cat([state_dict["special_care_embeds_weights"].float().reshape(-1),
                     state_dict["concept_embeds_weights"].float().reshape(-1)])
    rows = torch.nn.functional.normalize(torch.cat([special, concept]), dim=-1)      # eps 1e-12, as cosine_distance does
    if rows.shape[0] != thr.numel():
        raise ValueError(f"{rows.shape[0]} concept rows with {thr.numel()} thresholds")
    if rows.shape[0] > MAX_CONCEPTS:
        raise NotImplementedError(f"{rows.shape[0]} concept rows: the decision kernel holds at most {MAX_CONCEPTS}")
    return rows.contiguous(), thr.contiguous(), special.shape[0]


class HipSafetyChecker:
    def __init__(self, config: Optional[Dict], state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        """``config``: the checker's ``config.json`` as a dict (a CLIPConfig; only ``vision_config`` is read, for what the
        tensor shapes do not tell: heads, patch size, LayerNorm eps, activation)."""
        vc = dict(VISION_DEFAULTS, **{k: v for k, v in ((config or {}).get("vision_config") or {}).items() if v is not None})
        self.device = dev = torch.device(device)
        sd = tower_state_dict(state_dict)
        patch = int(vc["patch_size"])
        pw = sd["vision_model.embeddings.patch_embedding.weight"]
        if pw.shape[-1] != patch:
            raise ValueError(f"vision_config.patch_size {patch} against a {pw.shape[-1]} x {pw.shape[-1]} patch embedding")
        self.vision = HipCLIPVision(sd, num_heads=int(vc["num_attention_heads"]), patch_size=patch, device=dev,
                                    hidden_act=vc["hidden_act"], layer_norm_eps=float(vc["layer_norm_eps"]))
        grid = int(round((self.vision.pos.shape[0] - 1) ** 0.5))
        self.image_size = grid * patch                   # what clip_input has to measure (the position table says)
        rows, thr, self.n_special = concept_table(state_dict)
        if rows.shape[1] != self.vision.visual_projection.shape[0]:
            raise ValueError(f"concept rows of width {rows.shape[1]} against projection_dim {self.vision.visual_projection.shape[0]}")
        self.concepts, self.thresholds = rows.to(dev), thr.to(dev)

    @torch.no_grad()
    def cosines(self, clip_input: torch.Tensor):
        """-> (cos [B, K] fp32, scores [B, K] fp32 = cos - threshold + adjustment, unrounded; flags [B] int32), on the
        device; columns in table order, special-care first"""
        x, g, b, w = self.vision.head_inputs(clip_input)
        B, Np, C = x.shape
        return ops.clip_head(x, g, b, w, B=B, ldx=Np * C, eps=self.vision.eps, concepts=self.concepts,
                             thresholds=self.thresholds, n_special=self.n_special)

    @torch.no_grad()
    def __call__(self, clip_input: torch.Tensor, images):
        """``safety_checker(images=, clip_input=)`` of diffusers -> (images, has_nsfw_concepts: List[bool]).  A contiguous
        fp16 device tensor [B, ...] is blacked out in place by the kernel, before the flags reach the host; a numpy array
        or a list of arrays (or any other tensor) is zeroed item by item from the host list, as diffusers does."""
        _, _, flags = self.cosines(clip_input)
        if len(images) != flags.numel():
            raise ValueError(f"{len(images)} images with {flags.numel()} clip inputs")
        on_device = torch.is_tensor(images) and images.is_cuda and images.dtype == torch.float16 and images.is_contiguous()
        if on_device:
            ops.blackout_(images, flags)
        has_nsfw: List[bool] = [bool(v) for v in flags.cpu().tolist()]
        if not on_device:
            for idx, hit in enumerate(has_nsfw):
                if hit:
                    images[idx] = torch.zeros_like(images[idx]) if torch.is_tensor(images[idx]) else np.zeros(images[idx].shape)
        return images, has_nsfw
