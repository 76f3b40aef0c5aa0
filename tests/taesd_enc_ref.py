"""Test-side restatement of diffusers 0.23 ``AutoencoderTiny``'s ENCODER half (models/vae.py: ``EncoderTiny``; the Block is
tests/taesd_ref.py's ``AutoencoderTinyBlock``) as plain ``torch.nn`` modules with diffusers' attribute names, so that
``state_dict()`` has diffusers' keys (``encoder.layers.<i>.weight``, ``encoder.layers.<i>.conv.<j>.weight`` ...).  PARITY
UNPINNED, like tests/taesd_ref.py: diffusers is not vendored, the structure is restated from the published class.  Nothing
here imports the product.

``encoder.layers`` holds convs and Blocks only: conv(3 -> 64), then per level a bias-less stride-2 conv (from the second level
on) and n Blocks, then conv(64 -> 4); ``forward`` is ``layers(x.add(1).div(2))``.

``synthetic(seed)`` builds a model with He-scaled, fp16-representable weights (biases x 0.05, the 64 -> 4 conv x 0.05: the
residual sums grow by about sqrt(2) per Block and nothing normalises them; with these scales and uniform [-1, 1] images the
latents come out at std 0.4 - 1.8 from 16 x 24 pixels up (0.04 at 8 x 8, where every deep conv sees mostly padding) and every
activation stays far below the 1e3 that ``encode`` asserts, on the shapes of tests/test_gpu_taesd_encoder.py, checked on the CPU);
``encode(model, x)`` is the fp32 evaluation from ``half(x)`` (it asserts that no intermediate activation exceeds 1e3, so that
fp16 saturation cannot hide a difference); ``encode(model, x, fp16_activations=True)`` is the same network with every stored
activation rounded to fp16 -- the yardstick the whole-encoder tests hold the kernels to."""
from __future__ import annotations

import json
import math
import os

import torch
from torch import nn

from taesd_ref import ACT_LIMIT, CONFIG, AutoencoderTinyBlock


class EncoderTiny(nn.Module):
    def __init__(self, in_channels=3, out_channels=4, num_blocks=(1, 3, 3, 3), block_out_channels=(64, 64, 64, 64)):
        super().__init__()
        layers = []
        for i, num_block in enumerate(num_blocks):
            c = block_out_channels[i]
            if i == 0:
                layers.append(nn.Conv2d(in_channels, c, 3, padding=1))
            else:
                layers.append(nn.Conv2d(c, c, 3, padding=1, stride=2, bias=False))
            for _ in range(num_block):
                layers.append(AutoencoderTinyBlock(c, c))
        layers.append(nn.Conv2d(block_out_channels[-1], out_channels, 3, padding=1))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers(x.add(1).div(2))


class AutoencoderTinyEncRef(nn.Module):
    def __init__(self, num_encoder_blocks=(1, 3, 3, 3)):
        super().__init__()
        self.encoder = EncoderTiny(num_blocks=tuple(num_encoder_blocks), block_out_channels=(64,) * len(num_encoder_blocks))

    def encode(self, x):
        return self.encoder(x)


def synthetic(seed: int = 0, num_encoder_blocks=(1, 3, 3, 3)) -> AutoencoderTinyEncRef:
    """He-scaled conv weights (std = sqrt(2 / (9 C_in))), biases x 0.05, the 64 -> 4 output conv x 0.05; every value
    fp16-representable; fp32 module, eval."""
    g = torch.Generator().manual_seed(seed)
    m = AutoencoderTinyEncRef(num_encoder_blocks)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 4:
                v = torch.randn(p.shape, generator=g) * math.sqrt(2.0 / (9 * p.shape[1]))
                if p.shape[0] == 4:
                    v = v * 0.05
            else:
                v = torch.randn(p.shape, generator=g) * 0.05
            p.copy_(v.half().float())
    return m.eval()


def config(num_encoder_blocks=(1, 3, 3, 3)) -> dict:
    c = json.loads(json.dumps(CONFIG))
    c["num_encoder_blocks"] = list(num_encoder_blocks)
    c["encoder_block_out_channels"] = [64] * len(num_encoder_blocks)
    return c


def write_folder(folder, model: nn.Module, cfg: dict = None, dtype=torch.float16, extra: dict = None) -> str:
    """a diffusers component folder: config.json + diffusion_pytorch_model.safetensors (``extra``: further tensors, e.g. the
    ``decoder.*`` half of a whole AutoencoderTiny)"""
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(cfg or config(), f)
    sd = {k: v.detach().to(dtype).contiguous() for k, v in {**model.state_dict(), **(extra or {})}.items()}
    save_file(sd, os.path.join(folder, "diffusion_pytorch_model.safetensors"))
    return str(folder)


@torch.no_grad()
def encode(model: AutoencoderTinyEncRef, x: torch.Tensor, fp16_activations: bool = False, conv=None) -> torch.Tensor:
    """``model.encode(x)`` walked layer by layer from ``half(x)``: u = half(v + 1) / 2 (the fp16 model's ``x.add(1).div(2)``:
    one rounding, of v + 1), then fp32 convolutions.  ``fp16_activations`` rounds every tensor a layer hands to the next one
    (each conv, each conv + ReLU inside a Block, each Block's sum + ReLU, the latents) to fp16 and back.  Without it every
    intermediate is checked against ACT_LIMIT.  ``conv``: a replacement for ``module(x)`` (e.g. a float64 evaluation)."""
    rnd = (lambda t: t.half().float()) if fp16_activations else (lambda t: t)
    run = conv or (lambda m, t: m(t))

    def seen(t):
        if not fp16_activations:
            assert float(t.abs().max()) <= ACT_LIMIT, f"activation {float(t.abs().max()):.1f} exceeds {ACT_LIMIT}"
        return rnd(t)

    v = x.half()
    h = ((v + 1) / 2).float()                    # fp16 arithmetic: half(v + 1), halved exactly
    for m in model.encoder.layers:
        if isinstance(m, AutoencoderTinyBlock):
            t = h
            convs = list(m.conv)
            for j in (0, 2):
                t = seen(convs[j + 1](run(convs[j], t)))
            h = seen(m.fuse(run(convs[4], t) + m.skip(h)))
        else:
            h = seen(run(m, h))
    return h
