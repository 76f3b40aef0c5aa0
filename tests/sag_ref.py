"""Test-side restatement of self-attention guidance (Hong et al., arXiv 2210.00939; diffusers 0.23's
StableDiffusionSAGPipeline) on the oracle UNet.  PARITY UNPINNED, like tests/pag_ref.py: diffusers is not vendored.  Written
from the method's definition: the attention probabilities of ``mid_block.attentions[0]
.transformer_blocks[0].attn1`` on the guide rows give a mask (column mass > 1, nearest neighbour up to the latent size), the
guide rows' predicted sample is blurred under the mask and noised again with their predicted noise, and the step moves away
from the UNet's prediction on that: e = u + g (c - u) + s (u - e_d), or e = c + s (c - e_d) in the single pass.  The noise
model is read off the reference scheduler's own ``add_noise`` and ``scale_model_input`` (both linear), so every sampler is
degraded in its own variables.  Nothing here knows the product's kernels, buffers or coefficient tables.

``Recorder`` wraps the ``attn1`` processor of the oracle ``Attention`` and keeps the column mass of the map it computes;
``SagUNet`` sits behind ``oracle.loop.denoise``'s 2B-row call in the manner of ``pag_ref.PagUNet``.  ``colmass64`` and
``degrade64`` are float64 models of the contracts of cid_attn_colmass_f16 and cid_sag_degrade_f16 (include/cid.h)."""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

LAYER = "mid_block.attentions.0.transformer_blocks.0.attn1"
TAPS = 9


# --------------------------------------------------------------------------- the definition's pieces
def blur_weights(dtype=torch.float64) -> torch.Tensor:
    """exp(-k^2 / 2), k = -4 .. 4, normalised"""
    k = torch.arange(TAPS, dtype=torch.float64) - TAPS // 2
    w = torch.exp(-0.5 * k * k)
    return (w / w.sum()).to(dtype)


def blur(x: torch.Tensor) -> torch.Tensor:
    """the 9 x 9 Gaussian with sigma 1 on [B, C, h, w], per channel, reflect padding by 4"""
    w = blur_weights(x.dtype).to(x.device)
    k2 = (w[:, None] * w[None, :])[None, None].expand(x.shape[1], 1, TAPS, TAPS)
    return F.conv2d(F.pad(x, (TAPS // 2,) * 4, mode="reflect"), k2, groups=x.shape[1])


def nearest_index(out: int, inp: int) -> torch.Tensor:
    """source index of every destination index of a nearest-neighbour resize: floor(dst * in / out)"""
    return (torch.arange(out) * inp) // out


def upsample_mask(mask: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """[B, hm, wm] -> [B, h, w], nearest neighbour"""
    return mask[:, nearest_index(h, mask.shape[1])][:, :, nearest_index(w, mask.shape[2])]


def noise_model(sch, t, like: torch.Tensor):
    """(n_d, n_e, c_in) of the reference scheduler at timestep ``t``: add_noise(D, e, t) = n_d D + n_e e and
    scale_model_input(x, t) = c_in x, read off the two linear functions themselves"""
    one, zero = torch.ones(1, dtype=like.dtype, device=like.device), torch.zeros(1, dtype=like.dtype, device=like.device)
    return (float(sch.add_noise(one, zero, t)), float(sch.add_noise(zero, one, t)), float(sch.scale_model_input(one, t)))


def predictions(x, out, n_d: float, n_e: float, prediction: str):
    """(predicted sample, predicted noise) of the model output ``out`` at a sample x = n_d x0 + n_e eps.  v-prediction is
    defined on the normalised sample: with r = sqrt(n_d^2 + n_e^2), v = (n_d eps - n_e x0) / r"""
    if prediction == "epsilon":
        return (x - n_e * out) / n_d, out
    r = (n_d * n_d + n_e * n_e) ** 0.5
    a, b = n_d / r, n_e / r
    return a * (x / r) - b * out, a * out + b * (x / r)


def degrade(x, out, mask, n_d: float, n_e: float, prediction: str):
    """the degraded sample: the predicted sample blurred where ``mask`` [B, h, w] is set, noised again with the predicted noise"""
    x0, ehat = predictions(x, out, n_d, n_e, prediction)
    d = torch.where(mask[:, None], blur(x0), x0)
    return n_d * d + n_e * ehat


# --------------------------------------------------------------------------- the recording processor
class Recorder(nn.Module):
    """in front of the oracle's ``Consistent_AttProcessor``: computes the attention probabilities the wrapped processor is
    about to compute (same projections, LoRA terms included) and keeps their column mass, mean over heads: ``mass`` [b, N]"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.mass = inner, None

    def forward(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        assert encoder_hidden_states is None
        x, ls = hidden_states, self.inner.lora_scale
        q = attn.to_q(x) + ls * self.inner.to_q_lora(x)
        k = attn.to_k(x) + ls * self.inner.to_k_lora(x)
        b, n, c = q.shape
        split = lambda t: t.reshape(b, n, attn.heads, c // attn.heads).transpose(1, 2)
        p = (torch.matmul(split(q), split(k).transpose(-1, -2)) * attn.scale).softmax(dim=-1)     # [b, heads, i, j]
        self.mass = p.sum(dim=-2).mean(dim=1)
        return self.inner(attn, hidden_states, attention_mask=attention_mask, temb=temb)


@contextlib.contextmanager
def recording(unet):
    mod = dict(unet.named_modules())[LAYER]
    kept = mod.processor
    rec = Recorder(kept)
    try:
        mod.processor = rec
        yield rec
    finally:
        mod.processor = kept


# --------------------------------------------------------------------------- behind oracle.loop.denoise
class SagUNet:
    """The oracle UNet with SAG behind ``oracle.loop.denoise``'s 2B-row call [uncond | cond].  ``single``: the conditional rows
    only are evaluated and are the guide rows; else the unconditional rows guide.  The loop is handed e as both halves, so
    its u + g (c - u) is exactly e.  ``masses``: per call the guide rows' column mass [B, N] as float64 numpy; ``masks``: the
    thresholded [B, hm, wm]."""

    def __init__(self, unet, sch, guidance: float, sag_scale: float, single: bool = False, prediction: str = "epsilon"):
        self.unet, self.sch, self.g, self.s, self.single, self.prediction = unet, sch, float(guidance), float(sag_scale), single, prediction
        self.masses, self.masks = [], []

    def _unet(self, sample, t, ehs, added, recorder: bool):
        kw = {} if added is None else {"added_cond_kwargs": added}
        if not recorder:
            return self.unet(sample, t, encoder_hidden_states=ehs, cross_attention_kwargs={}, **kw).sample, None
        with recording(self.unet) as rec:
            out = self.unet(sample, t, encoder_hidden_states=ehs, cross_attention_kwargs={}, **kw).sample
        return out, rec.mass

    def __call__(self, sample, t, encoder_hidden_states, cross_attention_kwargs=None, added_cond_kwargs=None,
                 down_block_additional_residuals=None, mid_block_additional_residual=None):
        from oracle.unet import UNetOutput
        assert down_block_additional_residuals is None and mid_block_additional_residual is None
        B = sample.shape[0] // 2
        rows = (lambda v: v[B:]) if self.single else (lambda v: v)
        guide = lambda v: v[B:] if self.single else v[:B]
        sub = lambda f: None if added_cond_kwargs is None else {k: f(v) for k, v in added_cond_kwargs.items()}
        out, mass = self._unet(rows(sample), t, rows(encoder_hidden_states), sub(rows), True)
        e_g, mass = out[:B], mass[:B]                     # the guide rows lead what was evaluated, in both forms
        n_d, n_e, c_in = noise_model(self.sch, t, sample)
        xin = guide(sample)
        x = xin[:, :e_g.shape[1]] / c_in                  # the sample itself; a 9-channel UNet's extra channels are not scaled
        h, w = x.shape[2:]
        hm, wm = h, w
        for _ in range(len(self.unet.config.block_out_channels) - 1):      # every down block but the last halves both
            hm, wm = hm // 2, wm // 2
        assert hm * wm == mass.shape[1], (h, w, mass.shape)
        mask = mass.reshape(B, hm, wm) > 1.0
        self.masses.append(mass.detach().double().cpu().numpy())
        self.masks.append(mask.cpu().numpy())
        x_deg = degrade(x, e_g, upsample_mask(mask, h, w), n_d, n_e, self.prediction).to(sample.dtype)
        e_d, _ = self._unet(torch.cat([x_deg * c_in, xin[:, e_g.shape[1]:]], 1), t, guide(encoder_hidden_states), sub(guide), False)
        if self.single:
            e = e_g + self.s * (e_g - e_d)
        else:
            u, c = out.chunk(2)
            e = u + self.g * (c - u) + self.s * (u - e_d)
        return UNetOutput(sample=torch.cat([e, e]))


# --------------------------------------------------------------------------- float64 models of the two kernels' contracts
def colmass64(q, k, B: int, N: int, n_keys: int, heads: int, d: int, dtype=torch.float64) -> torch.Tensor:
    """cid_attn_colmass_f16 on ``q`` / ``k`` [B * N, >= heads * d] (head h at columns h * d; q carries scale * log2 e, so the
    softmax is in base 2): mass [B, N] in ``dtype`` arithmetic; columns >= n_keys are 0, rows >= n_keys do not contribute"""
    split = lambda t: t[:, :heads * d].to(dtype).reshape(B, N, heads, d).transpose(1, 2)[:, :, :n_keys]
    s = torch.matmul(split(q), split(k).transpose(-1, -2)) * float(np.log(2.0))
    mass = torch.zeros(B, N, dtype=dtype, device=q.device)
    mass[:, :n_keys] = s.softmax(dim=-1).sum(dim=-2).mean(dim=1)
    return mass


def degrade64(x, e, mass, coef, hm: int, wm: int) -> torch.Tensor:
    """cid_sag_degrade_f16 in float64: ``coef`` = p_x, p_e, q_x, q_e, n_d, n_e (further words ignored)"""
    x, e = x.double(), e.double()
    p_x, p_e, q_x, q_e, n_d, n_e = [float(v) for v in coef[:6]]
    B, _, h, w = x.shape
    x0, ehat = p_x * x + p_e * e, q_x * x + q_e * e
    mask = upsample_mask(mass.reshape(B, hm, wm) > 1.0, h, w)
    return n_d * torch.where(mask[:, None], blur(x0), x0) + n_e * ehat


def combine64(eps, eps_d, g: float, s: float, single: bool = False) -> np.ndarray:
    """float64 e of the three step entries from fp16 ``eps`` [2, n] (or [1, n] in the single pass) and ``eps_d`` [n]; at
    s == 0 ``eps_d`` does not enter (it may hold NaN)"""
    e = np.asarray(eps.double().numpy() if isinstance(eps, torch.Tensor) else eps, dtype=np.float64)
    base = e[0] if single else e[0] + g * (e[1] - e[0])
    if s == 0.0:
        return base
    return base + s * (e[0] - np.asarray(eps_d.double().numpy() if isinstance(eps_d, torch.Tensor) else eps_d, dtype=np.float64))
