"""HIP engine for diffusers' ``AutoencoderTiny`` decoder (TAESD for SD1.5, ``taesdxl`` for SDXL).

What a user of diffusers writes as ``pipe.vae = AutoencoderTiny.from_pretrained("madebyollin/taesd", torch_dtype=torch.float16)``
beside ``LCMScheduler``: a 64-channel, attention-free ReLU conv net that decodes SD latents directly (``scaling_factor`` 1.0)
at roughly a tenth of the KL decoder's arithmetic.  Here it is ``pipe.vae = loader.load_tiny_vae(folder)``; the pipelines
call ``decode_latents`` only, so it stands wherever a ``HipVAEDecoder`` stands (also beside a KL ``vae_encoder`` in the inpaint
pipelines: both work in the same latent space).

The structure below restates diffusers 0.23 ``models/vae.py: DecoderTiny`` / ``AutoencoderTinyBlock`` (diffusers is not a
dependency; UNPINNED, like the samplers of scheduler.py).  ``decoder.layers.<i>`` indices count the ReLU and Upsample modules:

    x = tanh(z / 3) * 3
    0 conv3x3(4 -> 64, bias)   1 ReLU
    per level l with n_l = num_decoder_blocks[l]:  n_l x Block(64);  then, unless last:  Upsample(2x nearest), conv3x3(64 -> 64, no bias)
    last: conv3x3(64 -> 3, bias);   image = 2 x - 1
    Block(x) = ReLU(conv.4(ReLU(conv.2(ReLU(conv.0(x))))) + x)            (skip = Identity at equal widths)

Activations are token-major fp16 ``[B, H*W, 64]`` from the first conv to the last; three kinds of launch, all in csrc/taesd.hip:
``cid_tiny_decode_in_f16`` (tanh + conv + ReLU from NCHW latents), ``cid_tiny_conv64_f16`` (every 64 -> 64 conv; bias, residual,
ReLU and the nearest-2x read are arguments) and ``cid_tiny_decode_out_f16`` (conv + ``2x - 1`` or the ``[0, 1]`` clamp, to NCHW).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

from . import ops

WIDTH = 64          # the only channel width the kernels are built for


# ------------------------------------------------------------------------------------------------ config and layer list
def check_tiny_config(config: Dict) -> Tuple[int, ...]:
    """Refuse every AutoencoderTiny config outside the published geometry, naming the key (before any weight is touched);
    returns ``num_decoder_blocks`` as a tuple."""
    def refuse(key, why):
        raise NotImplementedError(f"AutoencoderTiny config {key}={config.get(key)!r}: {why}")

    if config.get("act_fn", "relu") != "relu":
        refuse("act_fn", "only the ReLU decoder is built")
    blocks = config.get("num_decoder_blocks", (3, 3, 3, 1))
    if not isinstance(blocks, (list, tuple)) or not blocks or any((not isinstance(n, int)) or n <= 0 for n in blocks):
        refuse("num_decoder_blocks", "a non-empty list of positive block counts is expected")
    for key in ("decoder_block_out_channels", "block_out_channels"):
        ch = config.get(key, (WIDTH,) * len(blocks))
        if not isinstance(ch, (list, tuple)) or any(c != WIDTH for c in ch):
            refuse(key, f"every level must be {WIDTH} channels wide (the kernels are built for that width)")
        if len(ch) != len(blocks):
            refuse(key, f"one entry per level of num_decoder_blocks={tuple(blocks)!r} is expected")
    if config.get("latent_channels", 4) != 4:
        refuse("latent_channels", "the decoder head reads 4 latent channels")
    if config.get("out_channels", 3) != 3:
        refuse("out_channels", "the decoder tail writes 3 image channels")
    if config.get("upsampling_scaling_factor", 2) != 2:
        refuse("upsampling_scaling_factor", "only nearest 2x upsampling is built")
    return tuple(int(n) for n in blocks)


def tiny_decoder_layers(num_decoder_blocks) -> List[Tuple[str, int]]:
    """The ``decoder.layers`` walk as (kind, index) entries: ("in", 0), ("block", i), ("upconv", i) -- i is the index of the
    conv, its Upsample sits at i - 1 -- and ("out", i).  ReLU (index 1) and the Upsample modules carry no weights."""
    layers: List[Tuple[str, int]] = [("in", 0)]
    i = 2
    last = len(num_decoder_blocks) - 1
    for level, n in enumerate(num_decoder_blocks):
        for _ in range(n):
            layers.append(("block", i))
            i += 1
        if level != last:
            layers.append(("upconv", i + 1))
            i += 2
        else:
            layers.append(("out", i))
            i += 1
    return layers


def _expected_keys(layers) -> Dict[str, Tuple[int, ...]]:
    """decoder.* key -> shape, for the layer walk"""
    want: Dict[str, Tuple[int, ...]] = {}
    for kind, i in layers:
        p = f"decoder.layers.{i}"
        if kind == "in":
            want[f"{p}.weight"], want[f"{p}.bias"] = (WIDTH, 4, 3, 3), (WIDTH,)
        elif kind == "block":
            for j in (0, 2, 4):
                want[f"{p}.conv.{j}.weight"], want[f"{p}.conv.{j}.bias"] = (WIDTH, WIDTH, 3, 3), (WIDTH,)
        elif kind == "upconv":
            want[f"{p}.weight"] = (WIDTH, WIDTH, 3, 3)
        else:
            want[f"{p}.weight"], want[f"{p}.bias"] = (3, WIDTH, 3, 3), (3,)
    return want


def _pack_conv(w: torch.Tensor) -> torch.Tensor:
    """[N, C, 3, 3] -> [N, 9, C] fp16, tap = 3 ky + kx (the layout of every conv in csrc/taesd.hip)"""
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).to(torch.float16).contiguous()


def pack_tiny_decoder(config: Dict, state_dict: Dict[str, torch.Tensor]) -> Tuple[List[Tuple[str, int]], Dict[str, torch.Tensor]]:
    """diffusers AutoencoderTiny state dict -> (layer walk, packed tensors), on whatever device the tensors are (the CPU in
    the loader): ``"<i>.w"`` [N, 9, C] fp16 and ``"<i>.b"`` [N] fp16 for the single convs (no ``.b`` for the bias-less
    convs after an Upsample), ``"<i>.<j>.w"`` / ``"<i>.<j>.b"`` (j = 0, 2, 4) for a Block.  ``encoder.*`` keys are ignored;
    a missing or unexpected ``decoder.*`` key, or a wrong shape, is refused by name."""
    blocks = check_tiny_config(config)
    layers = tiny_decoder_layers(blocks)
    want = _expected_keys(layers)
    have = {k for k in state_dict if k.startswith("decoder.")}
    n_have = 1 + max((int(k.split(".")[2]) for k in have if k.startswith("decoder.layers.") and k.split(".")[2].isdigit()),
                     default=-1)
    n_want = layers[-1][1] + 1
    if n_have != n_want:
        raise NotImplementedError(f"AutoencoderTiny: the state dict has decoder.layers up to index {n_have - 1}, but "
                                  f"num_decoder_blocks={blocks!r} describes {n_want} layers (0 .. {n_want - 1})")
    missing = sorted(set(want) - have)
    if missing:
        raise NotImplementedError(f"AutoencoderTiny: missing key {missing[0]!r} (num_decoder_blocks={blocks!r} expects it; "
                                  f"{len(missing)} missing in all)")
    extra = sorted(have - set(want))
    if extra:
        raise NotImplementedError(f"AutoencoderTiny: unexpected key {extra[0]!r} (not part of the decoder that "
                                  f"num_decoder_blocks={blocks!r} describes; {len(extra)} unexpected in all)")
    for k, shape in want.items():
        if tuple(state_dict[k].shape) != shape:
            raise NotImplementedError(f"AutoencoderTiny: key {k!r} has shape {tuple(state_dict[k].shape)}, expected {shape}")
    packed: Dict[str, torch.Tensor] = {}
    for kind, i in layers:
        p = f"decoder.layers.{i}"
        if kind == "block":
            for j in (0, 2, 4):
                packed[f"{i}.{j}.w"] = _pack_conv(state_dict[f"{p}.conv.{j}.weight"])
                packed[f"{i}.{j}.b"] = state_dict[f"{p}.conv.{j}.bias"].detach().to(torch.float16).contiguous()
        else:
            packed[f"{i}.w"] = _pack_conv(state_dict[f"{p}.weight"])
            if kind != "upconv":
                packed[f"{i}.b"] = state_dict[f"{p}.bias"].detach().to(torch.float16).contiguous()
    return layers, packed


# ------------------------------------------------------------------------------------------------ the engine
class HipAutoencoderTiny:
    """``AutoencoderTiny`` (decoder only) with the decoder surface the pipelines use: ``decode_latents``, ``decode``,
    ``decode_tokens``, ``config``, ``dtype``, ``device``.  ``config``: the dict of the folder's ``config.json``;
    ``state_dict``: diffusers key names."""
    dtype = torch.float16

    def __init__(self, config: Dict, state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        self.layers, packed = pack_tiny_decoder(dict(config), state_dict)      # every refusal happens here, on the host
        self.device = torch.device(device)
        self.num_decoder_blocks = check_tiny_config(config)
        self.config = SimpleNamespace(scaling_factor=float(config.get("scaling_factor", 1.0)), latent_channels=4,
                                      out_channels=3, force_upcast=False, num_decoder_blocks=self.num_decoder_blocks,
                                      block_out_channels=(WIDTH,) * len(self.num_decoder_blocks))
        self.W = {k: v.to(self.device) for k, v in packed.items()}
        self._key: Optional[Tuple[int, int, int]] = None
        self._bufs: List[List[torch.Tensor]] = []

    @property
    def upscale(self) -> int:
        return 2 ** (len(self.num_decoder_blocks) - 1)

    def _buffers(self, B: int, h: int, w: int) -> List[List[torch.Tensor]]:
        """Three token-major buffers per resolution level, kept for the next call of the same shape.  A Block needs three:
        its input stays live as the residual of its third conv while the first two convs' outputs alternate."""
        if self._key != (B, h, w):
            self._bufs = []                 # release before allocating the new set
            self._bufs = [[torch.empty(B, (h << l) * (w << l), WIDTH, dtype=torch.float16, device=self.device) for _ in range(3)]
                          for l in range(len(self.num_decoder_blocks))]
            self._key = (B, h, w)
        return self._bufs

    @torch.no_grad()
    def _decode(self, latents: torch.Tensor, clamp01: bool) -> torch.Tensor:
        lat = latents.to(device=self.device, dtype=torch.float16).contiguous()
        if lat.dim() != 4 or lat.shape[1] != 4:
            raise ValueError(f"AutoencoderTiny decodes latents [B, 4, h, w], got {tuple(latents.shape)}")
        B, _, h, w = lat.shape
        W = self.W
        with torch.cuda.device(self.device):
            bufs = self._buffers(B, h, w)
            level, H, Wd = 0, h, w
            x = None
            for kind, i in self.layers:
                p, q, r = bufs[level]
                if kind == "in":
                    x = ops.tiny_decode_in(lat, p, W["0.w"], W["0.b"])
                elif kind == "block":
                    free = [t for t in (p, q, r) if t is not x]
                    a = ops.tiny_conv64(x, free[0], W[f"{i}.0.w"], W[f"{i}.0.b"], B=B, H=H, W=Wd, relu=True)
                    b = ops.tiny_conv64(a, free[1], W[f"{i}.2.w"], W[f"{i}.2.b"], B=B, H=H, W=Wd, relu=True)
                    x = ops.tiny_conv64(b, free[0], W[f"{i}.4.w"], W[f"{i}.4.b"], B=B, H=H, W=Wd, res=x, relu=True)
                elif kind == "upconv":
                    level += 1
                    x = ops.tiny_conv64(x, bufs[level][0], W[f"{i}.w"], None, B=B, H=H, W=Wd, up=True)
                    H, Wd = 2 * H, 2 * Wd
                else:
                    img = torch.empty(B, 3, H, Wd, dtype=torch.float16, device=self.device)
                    return ops.tiny_decode_out(x, img, W[f"{i}.w"], W[f"{i}.b"], clamp01=clamp01)
        raise AssertionError("the layer walk ends with the output conv")

    def _unscale(self, latents: torch.Tensor) -> torch.Tensor:
        """``latents / scaling_factor`` of decode_latents: the identity for every published AutoencoderTiny (1.0)"""
        sf = self.config.scaling_factor
        return latents if sf == 1.0 else latents / sf

    def decode_tokens(self, latents: torch.Tensor) -> torch.Tensor:
        """latents [B, 4, h, w] as the denoise loop leaves them (TAESD consumes SD latents directly: ``scaling_factor`` is 1.0,
        nothing is folded or undone) -> the image [B, 3, 8h, 8w] in [-1, 1], fp16: what ``AutoencoderTiny.decode`` returns."""
        return self._decode(self._unscale(latents), False)

    def decode(self, z: torch.Tensor, return_dict: bool = False):
        """diffusers ``vae.decode(z)`` protocol (``z`` already divided by ``scaling_factor`` by the caller)"""
        if return_dict:
            raise NotImplementedError("return_dict=True (the reference passes return_dict=False)")
        return (self._decode(z, False),)

    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        """``StableDiffusionPipeline.decode_latents`` up to the device tensor: [B, 3, H, W] in [0, 1].  With v = the last
        conv's output the image is 2v - 1 and ``(image / 2 + 0.5).clamp(0, 1)`` is clamp(v, 0, 1): the tail kernel's mode 1."""
        return self._decode(self._unscale(latents), True)

    def encode(self, *args, **kwargs):
        raise NotImplementedError("AutoencoderTiny.encode is not built: the inpaint pipelines keep the KL encoder "
                                  "(vae_encoder), which shares the latent space")
