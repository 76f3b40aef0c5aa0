"""Test-only reference for FreeU: diffusers 0.23's ``fourier_filter`` / ``apply_freeu`` (utils/torch_utils.py) restated with
torch.fft, the closed form the HIP kernel evaluates, and ``install_freeu``, which applies the torch.fft form
inside the first two up blocks of an oracle UNet (oracle/unet.py itself has no FreeU)."""
import math

import torch


def fourier_filter(x_in: torch.Tensor, threshold: int, scale: float) -> torch.Tensor:
    """NCHW.  diffusers: fftn -> fftshift -> the box [H//2 - t : H//2 + t, W//2 - t : W//2 + t] times ``scale`` -> ifftshift
    -> ifftn -> real part, in the input's dtype.  The fp16 arm follows diffusers: fp32 where a side is not a power of two.
    Where the FFT library refuses half precision for power-of-two sides as well (torch raises before any launch), those
    are cast to fp32 too -- at least as accurate as the half transform, so the arm is not made worse than diffusers'."""
    B, C, H, W = x_in.shape

    def run(x):
        x_freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
        mask = torch.ones((B, C, H, W), device=x.device, dtype=torch.float64 if x.dtype == torch.float64 else torch.float32)
        crow, ccol = H // 2, W // 2
        mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
        return torch.fft.ifftn(torch.fft.ifftshift(x_freq * mask, dim=(-2, -1)), dim=(-2, -1)).real.to(x_in.dtype)

    half = x_in.dtype in (torch.float16, torch.bfloat16)
    if half and (H & (H - 1)) == 0 and (W & (W - 1)) == 0:
        try:
            return run(x_in)
        except RuntimeError:        # no half-precision transform here
            pass
    return run(x_in.float() if half else x_in)


def apply_freeu(resolution_idx: int, hidden: torch.Tensor, skip: torch.Tensor, s1, s2, b1, b2):
    """NCHW.  Up block 0 / 1: the first half of ``hidden``'s channels times b1 / b2 (a new tensor here; diffusers writes in
    place), ``skip`` through the filter with s1 / s2; later blocks untouched."""
    if resolution_idx in (0, 1):
        s, b = (s1, b1) if resolution_idx == 0 else (s2, b2)
        n = hidden.shape[1] // 2
        hidden = torch.cat([hidden[:, :n] * b, hidden[:, n:]], dim=1)
        skip = fourier_filter(skip, threshold=1, scale=s)
    return hidden, skip


def closed_form(x: torch.Tensor, s: float) -> torch.Tensor:
    """[..., H, W] -> fourier_filter(x, 1, s) as seven sums per plane and a pointwise update, in x's dtype (use float64)"""
    H, W = x.shape[-2:]
    th = (2 * math.pi * torch.arange(H, dtype=x.dtype, device=x.device) / H)[:, None].expand(H, W)
    tw = (2 * math.pi * torch.arange(W, dtype=x.dtype, device=x.device) / W)[None, :].expand(H, W)
    phi = torch.stack([torch.ones_like(th), th.cos(), th.sin(), tw.cos(), tw.sin(), (th + tw).cos(), (th + tw).sin()])
    sums = torch.einsum("...hw,khw->...k", x, phi)
    return x + (s - 1.0) / (H * W) * torch.einsum("...k,khw->...hw", sums, phi)


def install_freeu(oracle_unet, s1, s2, b1, b2):
    """forward pre-hooks on the resnets of ``oracle_unet.up_blocks[0:2]``: the concatenated input [hidden | skip] is split at
    the hidden width (the previous block's output channels for resnet 0, the block's own for the others), goes through
    ``apply_freeu`` and is concatenated again -- what diffusers does in front of its torch.cat.  -> the hook handles"""
    handles = []
    prev = oracle_unet.config.block_out_channels[-1]          # the mid block's output
    for i, blk in enumerate(oracle_unet.up_blocks):
        cout = blk.resnets[0].conv1.out_channels
        if i < 2:
            for j, res in enumerate(blk.resnets):
                rin = prev if j == 0 else cout

                def hook(module, args, i=i, rin=rin):
                    x, *rest = args
                    h, k = apply_freeu(i, x[:, :rin], x[:, rin:], s1, s2, b1, b2)
                    return (torch.cat([h, k], dim=1), *rest)
                handles.append(res.register_forward_pre_hook(hook))
        prev = cout
    return handles
