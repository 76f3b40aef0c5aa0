"""Test-side restatement of perturbed-attention guidance (Ahn et al. 2024, arXiv 2403.17377; diffusers' PAG mixin) on the
oracle UNet.  PARITY UNPINNED, like tests/lcm_ref.py: diffusers is not vendored.  Written from the method's definition -- the
perturbed evaluation replaces the self-attention map of the chosen layers by the identity, so the layer's output is
``to_out(to_v(x))``, and the step moves away from it: e = u + g (c - u) + s (c - p).  Nothing here knows the product's
folded weights, row selectors or step kernels.

``PagAttnProcessor`` wraps the ``attn1`` processor of an oracle ``Attention``: the LAST 1 / ``parts`` of the batch takes the
identity path (with the ConsistentID adapter's ``to_v_lora`` / ``to_out_lora``), the rest goes through the wrapped processor.
``installed`` puts it on the selected layers for the length of a ``with`` block (the oracle models are shared and memoised).
``PagUNet`` sits behind ``oracle.loop.denoise``'s 2B-row call in the manner of ``lcm_ref.CondOnly``: it runs the 3B-row (or,
in the single pass, 2B-row) batch and hands the loop e as both halves, so the loop's u + g (c - u) is exactly e."""
from __future__ import annotations

import contextlib

import numpy as np
import torch
from torch import nn

DEFAULT_LAYERS = ("mid_block",)


def scale_at(pag_scale: float, pag_adaptive_scale: float, t) -> float:
    """the PAG scale at timestep ``t``: constant, or decreasing by ``pag_adaptive_scale`` per timestep below 1000, never negative"""
    if pag_adaptive_scale == 0.0:
        return float(pag_scale)
    return max(float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(t)), 0.0)


class PagAttnProcessor(nn.Module):
    def __init__(self, inner, parts: int):
        super().__init__()
        self.inner, self.parts = inner, parts

    def forward(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        assert encoder_hidden_states is None, "PAG perturbs self-attention only"
        b = hidden_states.shape[0]
        assert b % self.parts == 0
        lead = b - b // self.parts
        out = self.inner(attn, hidden_states[:lead], attention_mask=attention_mask, temb=temb)
        x, ls = hidden_states[lead:], self.inner.lora_scale
        v = attn.to_v(x) + ls * self.inner.to_v_lora(x)
        o = attn.to_out[0](v) + ls * self.inner.to_out_lora(v)
        o = attn.to_out[1](o)
        if attn.residual_connection:
            o = o + x
        return torch.cat([out, o / attn.rescale_output_factor])


def attn1_modules(unet, layers=DEFAULT_LAYERS):
    """{module path: oracle Attention} of every ``attn1`` under the module paths ``layers`` (whole dotted components)"""
    layers = [layers] if isinstance(layers, str) else list(layers)
    found = {}
    for name, mod in unet.named_modules():
        if name.endswith(".attn1"):
            parts = name.split(".")
            if any(parts[:len(want.split("."))] == want.split(".") for want in layers):
                found[name] = mod
    assert found, layers
    return found


@contextlib.contextmanager
def installed(unet, layers, parts: int):
    mods = attn1_modules(unet, layers)
    kept = {name: m.processor for name, m in mods.items()}
    try:
        for m in mods.values():
            m.processor = PagAttnProcessor(m.processor, parts)
        yield sorted(mods)
    finally:
        for name, m in mods.items():
            m.processor = kept[name]


def forward_rows(unet, layers, sample, t, ehs, parts: int, added=None):
    """one forward of a batch whose last 1 / ``parts`` is perturbed in ``layers`` -> the UNet's output, all rows"""
    with installed(unet, layers, parts):
        kw = {} if added is None else {"added_cond_kwargs": added}
        return unet(sample, t, encoder_hidden_states=ehs, cross_attention_kwargs={}, **kw).sample


class PagUNet:
    """The oracle UNet with PAG behind ``oracle.loop.denoise``'s 2B-row call [uncond | cond].  ``single``: the conditional rows
    only, [cond | perturbed], e = c + s (c - p); else [uncond | cond | perturbed], e = u + g (c - u) + s (c - p).  The perturbed
    rows repeat the conditional rows' latents, embeds and added conditions.  ``seen`` keeps, per call, (s, |c - p| / |c|)."""

    def __init__(self, unet, layers, guidance: float, pag_scale: float, pag_adaptive_scale: float = 0.0, single: bool = False):
        self.unet, self.layers, self.g, self.single = unet, layers, float(guidance), single
        self.pag_scale, self.adaptive = pag_scale, pag_adaptive_scale
        self.seen = []

    def __call__(self, sample, t, encoder_hidden_states, cross_attention_kwargs=None, added_cond_kwargs=None,
                 down_block_additional_residuals=None, mid_block_additional_residual=None):
        from oracle.unet import UNetOutput
        assert down_block_additional_residuals is None and mid_block_additional_residual is None
        B = sample.shape[0] // 2
        rows = (lambda v: torch.cat([v[B:], v[B:]])) if self.single else (lambda v: torch.cat([v, v[B:]]))
        added = None if added_cond_kwargs is None else {k: rows(v) for k, v in added_cond_kwargs.items()}
        out = forward_rows(self.unet, self.layers, rows(sample), t, rows(encoder_hidden_states), 2 if self.single else 3, added)
        s = scale_at(self.pag_scale, self.adaptive, t)
        if self.single:
            c, p = out.chunk(2)
            e = c + s * (c - p)
        else:
            u, c, p = out.chunk(3)
            e = u + self.g * (c - u) + s * (c - p)
        self.seen.append((s, float((c.double() - p.double()).norm() / c.double().norm())))
        return UNetOutput(sample=torch.cat([e, e]))


def combine64(eps, g: float, s: float, single: bool = False) -> np.ndarray:
    """float64 e of the step kernels from fp16 ``eps`` [3, n] (or [2, n] in the single pass): what ``multistep_ref.RowEmulator``
    is fed as both of its halves.  At s == 0 the perturbed rows do not enter (they may hold NaN, like everything else a zero
    coefficient covers in that emulator)."""
    e = np.asarray(eps.double().numpy() if isinstance(eps, torch.Tensor) else eps, dtype=np.float64)
    c, p = e[-2], e[-1]
    base = c if single else e[0] + g * (c - e[0])
    return base if s == 0.0 else base + s * (c - p)
