"""HIP execution engine for the CLIP vision tower as the reference uses it (once per image):

    self.image_encoder(clip_image, output_hidden_states=True).hidden_states[-2]
    (pipline_StableDiffusion_ConsistentID.py:182-183, :200-201; ``CLIPVisionModelWithProjection`` of
     laion/CLIP-ViT-H-14-laion2B-s32B-b79K, loaded at :54-56)

i.e. the token states [B, 257, 1280] after all but the last encoder layer.  Weights: the ``transformers`` state_dict
(``vision_model.*``).  The 14x14/14 patch embedding is an unfold (index plumbing) + ``cid_gemm_f16`` (K padded 588 -> 640),
every encoder layer is the encoder layer of clip_layers.py (weights packed and launched there) around
``cid_self_attn_keys_f16`` (257 real keys on a 320-token padded axis), with ``cid_gelu_f16``.

The safety checker (safety.py) runs the same tower at the ViT-L/14 geometry with ``hidden_act="quick_gelu"``
(``cid_quick_gelu_f16``) and reads what follows the last layer: ``image_embeds`` = visual_projection(post_layernorm(CLS)),
one ``cid_clip_head_f16`` launch on token 0 of the padded state.  The ConsistentID pre-loop never reads that embedding.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .clip_layers import ACTIVATIONS, pack_layers, run_layer
from .weights import _h


class HipCLIPVision:
    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int, patch_size: int = 14, device="cuda:0",
                 hidden_act: str = "gelu", layer_norm_eps: float = 1e-5):
        if hidden_act not in ACTIVATIONS:
            raise NotImplementedError(f"hidden_act {hidden_act!r}: the vision towers are built for {tuple(ACTIVATIONS)} (exact GELU: "
                                      "the ViT-H tower of the reference; quick GELU: the safety checker's ViT-L)")
        self._act = ACTIVATIONS[hidden_act]
        self.device = dev = torch.device(device)
        sd = {k[len("vision_model."):]: v for k, v in state_dict.items() if k.startswith("vision_model.")}
        pw = sd["embeddings.patch_embedding.weight"]                     # [C, 3, P, P], no bias
        self.C, self.P, self.heads, self.eps = pw.shape[0], patch_size, num_heads, layer_norm_eps
        assert pw.shape[-1] == patch_size and self.C % num_heads == 0
        self.d = self.C // num_heads
        kp = pw[0].numel()
        self.kpad = (kp + 63) // 64 * 64
        w = torch.zeros(self.C, self.kpad)
        w[:, :kp] = pw.reshape(self.C, kp).float()
        W: Dict[str, torch.Tensor] = {"patch.w": _h(w, dev)}
        self.cls = _h(sd["embeddings.class_embedding"], dev)
        self.pos = _h(sd["embeddings.position_embedding.weight"], dev)   # [1 + n_patches, C]
        for n in ("pre_layrnorm",):
            W[f"{n}.g"], W[f"{n}.b"] = _h(sd[f"{n}.weight"], dev), _h(sd[f"{n}.bias"], dev)
        self.n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
        pack_layers(W, sd, self.n_layers, self.d, dev)
        # what follows the last layer (CLIPVisionTransformer.post_layernorm, CLIPVisionModelWithProjection.visual_projection):
        # read by image_embeds only; checkpoints of the bare CLIPVisionModel have no projection
        self.post_ln = (_h(sd["post_layernorm.weight"], dev), _h(sd["post_layernorm.bias"], dev)) if "post_layernorm.weight" in sd else None
        vp = state_dict.get("visual_projection.weight")
        self.visual_projection = None if vp is None else _h(vp, dev)                      # [P, C], no bias
        self.W = W

    def _empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float16, device=self.device)

    @torch.no_grad()
    def hidden_states(self, pixel_values: torch.Tensor, index: int = -2) -> torch.Tensor:
        """``image_encoder(pixel_values, output_hidden_states=True).hidden_states[index]`` -> [B, 1 + n_patches, C]"""
        x, ntok = self._padded_states(pixel_values, index)
        return x[:, :ntok].contiguous()

    @torch.no_grad()
    def _padded_states(self,pixel_values: torch.Tensor, index: int):
        """(hidden_states[index] on the padded token axis [B, Np, C], number of real tokens)"""
        W, C, P, dev = self.W, self.C, self.P, self.device
        n_run = self.n_layers + 1 + index if index < 0 else index      # hidden_states[k] = state after k layers
        assert 0 <= n_run <= self.n_layers
        x = pixel_values.to(device=dev, dtype=torch.float16)
        B, _, H, Wd = x.shape
        gh, gw = H // P, Wd // P
        ntok = 1 + gh * gw
        assert ntok == self.pos.shape[0], "image size does not match the position embedding"
        Np = (ntok + 63) // 64 * 64                                     # padded token axis
        # patch embedding: unfold (c, ky, kx) like Conv2d's weight layout, GEMM
        pt = x.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B * gh * gw, -1)
        pin = torch.zeros(B * gh * gw, self.kpad, dtype=torch.float16, device=dev)
        pin[:, :pt.shape[1]] = pt
        pe = self._empty(B * gh * gw, C)
        ops.gemm(pin, W["patch.w"], pe, M=B * gh * gw, N=C, c1=self.kpad)
        h = torch.zeros(B, Np, C, dtype=torch.float16, device=dev)      # pad rows start at zero and stay row-local
        h[:, 0] = self.cls
        h[:, 1:ntok] = pe.view(B, gh * gw, C)
        h[:, :ntok] += self.pos                                         # embeddings = patches (+cls) + position (fp16 add)
        h = h.view(B * Np, C)
        M = B * Np
        x = self._empty(M, C)
        ops.layernorm(h, x, W["pre_layrnorm.g"], W["pre_layrnorm.b"], M=M, C_=C, eps=self.eps)
        for i in range(n_run):
            x = run_layer(W, i, x, B=B, Np=Np, heads=self.heads, d=self.d, eps=self.eps, attn=ops.self_attn, n_keys=ntok,
                          act=self._act)
        return x.view(B, Np, C), ntok

    def head_inputs(self, pixel_values: torch.Tensor):
        """The operands of ``ops.clip_head`` for these images: (last hidden state on its padded axis [B, Np, C] -- row b of
        the head is its token 0, pitch Np * C --, post_layernorm gain, bias, visual_projection weight)"""
        if self.post_ln is None or self.visual_projection is None:
            raise ValueError("this state dict has no post_layernorm / visual_projection.weight: image_embeds needs a "
                             "CLIPVisionModelWithProjection checkpoint")
        x, _ = self._padded_states(pixel_values, -1)
        return x, self.post_ln[0], self.post_ln[1], self.visual_projection

    @torch.no_grad()
    def image_embeds(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """``image_encoder(pixel_values).image_embeds`` -> [B, projection_dim] fp16: every layer, then post_layernorm of
        the CLS token and visual_projection in one launch"""
        x, g, b, w = self.head_inputs(pixel_values)
        B, Np, C = x.shape
        out = self._empty(B, w.shape[0])
        return ops.clip_head(x, g, b, w, B=B, ldx=Np * C, eps=self.eps, embeds=out)

    def __call__(self, pixel_values, output_hidden_states: bool = True):
        raise NotImplementedError("hidden_states(pixel_values, index) and image_embeds(pixel_values) are implemented: the "
                                  "reference reads hidden_states[-2] from the image encoder (ref :182-183, :200-201) and its "
                                  "safety checker the projected embedding")
