"""Test-side restatement of diffusers 0.23 ``AutoencoderTiny`` (decoder half; models/autoencoder_tiny.py and models/vae.py:
``DecoderTiny``, ``AutoencoderTinyBlock``) as plain ``torch.nn`` modules with diffusers' attribute names, so that
``state_dict()`` has diffusers' keys (``decoder.layers.<i>.weight``, ``decoder.layers.<i>.conv.<j>.weight`` ...).  PARITY
UNPINNED, like tests/lcm_ref.py: diffusers is not vendored, the structure is restated from the published class.  Nothing here
imports the product.

``synthetic(seed)`` builds a model with He-scaled, fp16-representable weights; ``decode(model, z)`` is the fp32 evaluation (it
asserts that no intermediate activation exceeds 1e3, so that fp16 saturation cannot hide a difference);
``decode(model, z, fp16_activations=True)`` is the same network with every stored activation rounded to fp16 -- the yardstick
the whole-decoder tests hold the kernels to."""
from __future__ import annotations

import json
import math
import os

import torch
from torch import nn

CONFIG = {"_class_name": "AutoencoderTiny", "_diffusers_version": "0.23.0", "act_fn": "relu",
          "decoder_block_out_channels": [64, 64, 64, 64], "encoder_block_out_channels": [64, 64, 64, 64],
          "force_upcast": False, "in_channels": 3, "latent_channels": 4, "latent_magnitude": 3, "latent_shift": 0.5,
          "num_decoder_blocks": [3, 3, 3, 1], "num_encoder_blocks": [1, 3, 3, 3], "out_channels": 3, "scaling_factor": 1.0,
          "upsampling_scaling_factor": 2}
ACT_LIMIT = 1e3


class AutoencoderTinyBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(out_channels, out_channels, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(out_channels, out_channels, 3, padding=1))
        self.skip = nn.Conv2d(in_channels, out_channels, 1, bias=False) if in_channels != out_channels else nn.Identity()
        self.fuse = nn.ReLU()

    def forward(self, x):
        return self.fuse(self.conv(x) + self.skip(x))


class DecoderTiny(nn.Module):
    def __init__(self, in_channels=4, out_channels=3, num_blocks=(3, 3, 3, 1), block_out_channels=(64, 64, 64, 64),
                 upsampling_scaling_factor=2):
        super().__init__()
        layers = [nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1), nn.ReLU()]
        for i, num_block in enumerate(num_blocks):
            is_final = i == len(num_blocks) - 1
            c = block_out_channels[i]
            for _ in range(num_block):
                layers.append(AutoencoderTinyBlock(c, c))
            if not is_final:
                layers.append(nn.Upsample(scale_factor=upsampling_scaling_factor))
            layers.append(nn.Conv2d(c, c if not is_final else out_channels, 3, padding=1, bias=is_final))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        x = torch.tanh(x / 3) * 3
        return self.layers(x).mul(2).sub(1)


class AutoencoderTinyRef(nn.Module):
    def __init__(self, num_decoder_blocks=(3, 3, 3, 1)):
        super().__init__()
        self.decoder = DecoderTiny(num_blocks=tuple(num_decoder_blocks), block_out_channels=(64,) * len(num_decoder_blocks))

    def decode(self, z):
        return self.decoder(z)


def synthetic(seed: int = 0, num_decoder_blocks=(3, 3, 3, 1)) -> AutoencoderTinyRef:
    """He-scaled conv weights (std = sqrt(2 / (9 C_in))), small biases, every value fp16-representable; fp32 module, eval.
    (The 64 -> 3 output conv is He-scaled times 0.01, its bias 0.5 +- 0.0005.)"""
    g = torch.Generator().manual_seed(seed)
    m = AutoencoderTinyRef(num_decoder_blocks)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 4:
                v = torch.randn(p.shape, generator=g) * math.sqrt(2.0 / (9 * p.shape[1]))
            else:
                v = torch.randn(p.shape, generator=g) * 0.05
            if p.shape[0] == 3:
                # the residual sums grow by sqrt(2) per Block (no normalisation in this net); the output conv brings the
                # image back to 0.5 +- ~1, so that it straddles both ends of decode_latents' [0, 1] clamp
                v = v * 0.01 + (0.5 if p.dim() == 1 else 0.0)
            p.copy_(v.half().float())
    return m.eval()


def config(num_decoder_blocks=(3, 3, 3, 1)) -> dict:
    c = json.loads(json.dumps(CONFIG))
    c["num_decoder_blocks"] = list(num_decoder_blocks)
    c["decoder_block_out_channels"] = [64] * len(num_decoder_blocks)
    return c


def write_folder(folder, model: AutoencoderTinyRef, cfg: dict = None, dtype=torch.float16) -> str:
    """a diffusers component folder: config.json + diffusion_pytorch_model.safetensors"""
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(cfg or config(), f)
    save_file({k: v.detach().to(dtype).contiguous() for k, v in model.state_dict().items()},
              os.path.join(folder, "diffusion_pytorch_model.safetensors"))
    return str(folder)


@torch.no_grad()
def decode(model: AutoencoderTinyRef, z: torch.Tensor, fp16_activations: bool = False, clamp01: bool = False) -> torch.Tensor:
    """``model.decode(z)`` walked layer by layer in fp32 (``clamp01``: then decode_latents' ``(image / 2 + 0.5).clamp(0, 1)``).
    ``fp16_activations`` rounds every tensor a layer hands to the next one (each conv + ReLU, each Block's sum + ReLU, each
    bias-less conv after an Upsample, the image) to fp16 and back.  Without it every intermediate is checked against ACT_LIMIT."""
    rnd = (lambda t: t.half().float()) if fp16_activations else (lambda t: t)

    def seen(t):
        if not fp16_activations:
            assert float(t.abs().max()) <= ACT_LIMIT, f"activation {float(t.abs().max()):.1f} exceeds {ACT_LIMIT}"
        return rnd(t)

    x = torch.tanh(z.float() / 3) * 3
    layers = list(model.decoder.layers)
    i = 0
    while i < len(layers):
        m = layers[i]
        if isinstance(m, AutoencoderTinyBlock):
            h = x
            convs = list(m.conv)
            for j in (0, 2):
                h = seen(convs[j + 1](convs[j](h)))
            x = seen(m.fuse(convs[4](h) + m.skip(x)))
        elif isinstance(m, nn.Conv2d):
            x = m(x)
            if i + 1 < len(layers) and isinstance(layers[i + 1], nn.ReLU):
                x = layers[i + 1](x)
                i += 1
            if i + 1 < len(layers):
                x = seen(x)
        else:                                   # nn.Upsample: its output is not stored by an fp16 pipeline either way
            x = m(x)
        i += 1
    if not fp16_activations:
        assert float(x.abs().max()) <= ACT_LIMIT
    img = x.mul(2).sub(1)
    if clamp01:
        img = (img / 2 + 0.5).clamp(0, 1)
    return rnd(img)
