"""HIP engines for diffusers' ``AutoencoderTiny`` (TAESD for SD1.5, ``taesdxl`` for SDXL): the decoder and the
encoder (``HipAutoencoderTinyEncoder`` at the end of this module).

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

from dataclasses import dataclass
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
    return layers, _pack_layers(state_dict, "decoder", blocks, layers, want, bare="upconv")


def _pack_layers(state_dict, half: str, blocks, layers, want, bare: str) -> Dict[str, torch.Tensor]:
    """the checks and the packing the two halves share: ``half`` = "decoder" | "encoder" (the key prefix, and
    ``num_<half>_blocks`` in the messages), ``want`` = key -> shape for the layer walk, ``bare`` = the kind of the bias-less convs"""
    have = {k for k in state_dict if k.startswith(f"{half}.")}
    n_have = 1 + max((int(k.split(".")[2]) for k in have if k.startswith(f"{half}.layers.") and k.split(".")[2].isdigit()),
                     default=-1)
    n_want = layers[-1][1] + 1
    if n_have != n_want:
        raise NotImplementedError(f"AutoencoderTiny: the state dict has {half}.layers up to index {n_have - 1}, but "
                                  f"num_{half}_blocks={blocks!r} describes {n_want} layers (0 .. {n_want - 1})")
    missing = sorted(set(want) - have)
    if missing:
        raise NotImplementedError(f"AutoencoderTiny: missing key {missing[0]!r} (num_{half}_blocks={blocks!r} expects it; "
                                  f"{len(missing)} missing in all)")
    extra = sorted(have - set(want))
    if extra:
        raise NotImplementedError(f"AutoencoderTiny: unexpected key {extra[0]!r} (not part of the {half} that "
                                  f"num_{half}_blocks={blocks!r} describes; {len(extra)} unexpected in all)")
    for k, shape in want.items():
        if tuple(state_dict[k].shape) != shape:
            raise NotImplementedError(f"AutoencoderTiny: key {k!r} has shape {tuple(state_dict[k].shape)}, expected {shape}")
    packed: Dict[str, torch.Tensor] = {}
    for kind, i in layers:
        p = f"{half}.layers.{i}"
        if kind == "block":
            for j in (0, 2, 4):
                packed[f"{i}.{j}.w"] = _pack_conv(state_dict[f"{p}.conv.{j}.weight"])
                packed[f"{i}.{j}.b"] = state_dict[f"{p}.conv.{j}.bias"].detach().to(torch.float16).contiguous()
        else:
            packed[f"{i}.w"] = _pack_conv(state_dict[f"{p}.weight"])
            if kind != bare:
                packed[f"{i}.b"] = state_dict[f"{p}.bias"].detach().to(torch.float16).contiguous()
    return packed


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
                                  "(vae_encoder), which shares the latent space; the tiny encoder is a class of its own, "
                                  "HipAutoencoderTinyEncoder (loader.load_tiny_vae_encoder), for pipe.vae_encoder")


# ------------------------------------------------------------------------------------------------ the encoder
# diffusers 0.23 ``models/vae.py: EncoderTiny`` restated (UNPINNED, like the decoder above).  ``encoder.layers.<i>`` holds convs
# and Blocks only (no ReLU or pooling modules), so the indices count those:
#
#     u = (x + 1) / 2                                  image [-1, 1] -> TAESD's [0, 1]
#     0 conv3x3(3 -> 64, bias)                         no activation after it
#     per level l with n_l = num_encoder_blocks[l]:    l > 0: conv3x3(64 -> 64, stride 2, padding 1, no bias);  n_l x Block(64)
#     last: conv3x3(64 -> 4, bias);   latents = output (scaling_factor 1.0, no posterior, nothing sampled)
#
# The published (1, 3, 3, 3) has 15 entries: 0 conv, 1 Block, 2 down, 3-5 Blocks, 6 down, 7-9, 10 down, 11-13, 14 conv.  A
# stride-2 conv turns n pixels into ceil(n / 2); output (y, x) reads input (2y - 1 + dy, 2x - 1 + dx), zeros outside on all four
# sides (not the right / bottom padding of the KL encoder's Downsample2D).
def check_tiny_encoder_config(config: Dict) -> Tuple[int, ...]:
    """Refuse every AutoencoderTiny config whose encoder is outside the published geometry, naming the key (before any weight
    is touched); returns ``num_encoder_blocks`` as a tuple."""
    def refuse(key, why):
        raise NotImplementedError(f"AutoencoderTiny config {key}={config.get(key)!r}: {why}")

    if config.get("act_fn", "relu") != "relu":
        refuse("act_fn", "only the ReLU encoder is built")
    blocks = config.get("num_encoder_blocks", (1, 3, 3, 3))
    if not isinstance(blocks, (list, tuple)) or not blocks or any((not isinstance(n, int)) or n <= 0 for n in blocks):
        refuse("num_encoder_blocks", "a non-empty list of positive block counts is expected")
    for key in ("encoder_block_out_channels", "block_out_channels"):
        ch = config.get(key, (WIDTH,) * len(blocks))
        if not isinstance(ch, (list, tuple)) or any(c != WIDTH for c in ch):
            refuse(key, f"every level must be {WIDTH} channels wide (the kernels are built for that width)")
        if len(ch) != len(blocks):
            refuse(key, f"one entry per level of num_encoder_blocks={tuple(blocks)!r} is expected")
    if config.get("in_channels", 3) != 3:
        refuse("in_channels", "the encoder head reads 3 image channels")
    if config.get("latent_channels", 4) != 4:
        refuse("latent_channels", "the encoder tail writes 4 latent channels")
    return tuple(int(n) for n in blocks)


def tiny_encoder_layers(num_encoder_blocks) -> List[Tuple[str, int]]:
    """The ``encoder.layers`` walk as (kind, index) entries: ("in", 0), ("block", i), ("down", i) -- the stride-2 conv in
    front of every level but the first -- and ("out", i)."""
    layers: List[Tuple[str, int]] = [("in", 0)]
    i = 1
    for level, n in enumerate(num_encoder_blocks):
        if level:
            layers.append(("down", i))
            i += 1
        for _ in range(n):
            layers.append(("block", i))
            i += 1
    layers.append(("out", i))
    return layers


def _expected_encoder_keys(layers) -> Dict[str, Tuple[int, ...]]:
    """encoder.* key -> shape, for the layer walk"""
    want: Dict[str, Tuple[int, ...]] = {}
    for kind, i in layers:
        p = f"encoder.layers.{i}"
        if kind == "in":
            want[f"{p}.weight"], want[f"{p}.bias"] = (WIDTH, 3, 3, 3), (WIDTH,)
        elif kind == "block":
            for j in (0, 2, 4):
                want[f"{p}.conv.{j}.weight"], want[f"{p}.conv.{j}.bias"] = (WIDTH, WIDTH, 3, 3), (WIDTH,)
        elif kind == "down":
            want[f"{p}.weight"] = (WIDTH, WIDTH, 3, 3)
        else:
            want[f"{p}.weight"], want[f"{p}.bias"] = (4, WIDTH, 3, 3), (4,)
    return want


def pack_tiny_encoder(config: Dict, state_dict: Dict[str, torch.Tensor]) -> Tuple[List[Tuple[str, int]], Dict[str, torch.Tensor]]:
    """``pack_tiny_decoder`` for the encoder half: (layer walk, packed tensors) with the same names -- ``"<i>.w"`` [N, 9, C] fp16
    and ``"<i>.b"`` for the single convs (no ``.b`` for the bias-less stride-2 convs), ``"<i>.<j>.w"`` / ``"<i>.<j>.b"`` (j = 0,
    2, 4) for a Block.  ``decoder.*`` keys are ignored; a missing or unexpected ``encoder.*`` key, or a wrong shape, is refused
    by name."""
    blocks = check_tiny_encoder_config(config)
    layers = tiny_encoder_layers(blocks)
    want = _expected_encoder_keys(layers)
    return layers, _pack_layers(state_dict, "encoder", blocks, layers, want, bare="down")


@dataclass
class AutoencoderTinyOutput:
    latents: torch.Tensor


class HipAutoencoderTinyEncoder:
    """``AutoencoderTiny.encode`` with the surface of ``HipVAEEncoder`` that the inpaint pipelines use (``encode_inpaint``,
    ``config``), for ``pipe.vae_encoder``.  It stands beside either decoder: TAESD and the KL VAE share a latent space.
    ``config``: the dict of the folder's ``config.json``; ``state_dict``: diffusers key names (``decoder.*`` ignored).

    Launches: ``cid_tiny_encode_in_f16`` (pre-processing + conv 3 -> 64), ``cid_tiny_conv64_f16`` for the three convs of every
    Block, ``cid_tiny_conv64_s2_f16`` between levels, ``cid_tiny_encode_out_f16`` (conv 64 -> 4, times the scale)."""
    dtype = torch.float16

    def __init__(self, config: Dict, state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        self.layers, packed = pack_tiny_encoder(dict(config), state_dict)      # every refusal happens here, on the host
        self.device = torch.device(device)
        self.num_encoder_blocks = check_tiny_encoder_config(config)
        self.config = SimpleNamespace(scaling_factor=float(config.get("scaling_factor", 1.0)), latent_channels=4,
                                      in_channels=3, force_upcast=False, num_encoder_blocks=self.num_encoder_blocks,
                                      block_out_channels=(WIDTH,) * len(self.num_encoder_blocks))
        self.W = {k: v.to(self.device) for k, v in packed.items()}
        self._key: Optional[Tuple[int, int, int]] = None
        self._bufs: List[List[torch.Tensor]] = []

    @property
    def downscale(self) -> int:
        return 2 ** (len(self.num_encoder_blocks) - 1)

    def _buffers(self, B: int, H: int, W: int) -> List[List[torch.Tensor]]:
        """Three token-major buffers per resolution level (a Block needs three, as in the decoder), kept for the next call of
        the same shape"""
        if self._key != (B, H, W):
            self._bufs = []                 # release before allocating the new set
            h, w = H, W
            for _ in self.num_encoder_blocks:
                self._bufs.append([torch.empty(B, h * w, WIDTH, dtype=torch.float16, device=self.device) for _ in range(3)])
                h, w = (h + 1) // 2, (w + 1) // 2
            self._key = (B, H, W)
        return self._bufs

    @staticmethod
    def _image_f32(x: torch.Tensor, dev) -> torch.Tensor:
        return x.to(device=dev, dtype=torch.float32).contiguous()

    @torch.no_grad()
    def _encode(self, image: torch.Tensor, mask: Optional[torch.Tensor], normalize: bool, blocks: int, scale: float,
                mask_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the whole walk on fp32 device tensors: -> latents [nblk * Bi, 4, h, w] fp16, times ``scale``"""
        Bi, _, H, Wd = image.shape
        B = Bi * (2 if blocks == 3 else 1)
        W = self.W
        with torch.cuda.device(self.device):
            bufs = self._buffers(B, H, Wd)
            level = 0
            x = None
            for kind, i in self.layers:
                p, q, r = bufs[level]
                if kind == "in":
                    x = ops.tiny_encode_in(image, p, W["0.w"], W["0.b"], mask=mask, normalize=normalize, blocks=blocks,
                                           mask_latents=mask_latents)
                elif kind == "block":
                    free = [t for t in (p, q, r) if t is not x]
                    a = ops.tiny_conv64(x, free[0], W[f"{i}.0.w"], W[f"{i}.0.b"], B=B, H=H, W=Wd, relu=True)
                    b = ops.tiny_conv64(a, free[1], W[f"{i}.2.w"], W[f"{i}.2.b"], B=B, H=H, W=Wd, relu=True)
                    x = ops.tiny_conv64(b, free[0], W[f"{i}.4.w"], W[f"{i}.4.b"], B=B, H=H, W=Wd, res=x, relu=True)
                elif kind == "down":
                    level += 1
                    x = ops.tiny_conv64_s2(x, bufs[level][0], W[f"{i}.w"], B=B, H=H, W=Wd)
                    H, Wd = (H + 1) // 2, (Wd + 1) // 2
                else:
                    lat = torch.empty(B, 4, H, Wd, dtype=torch.float16, device=self.device)
                    return ops.tiny_encode_out(x, lat, W[f"{i}.w"], W[f"{i}.b"], scale=scale)
        raise AssertionError("the layer walk ends with the output conv")

    # ------------------------------------------------------------------ diffusers protocol
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """``AutoencoderTiny.encode(x)``: ``x`` [B, 3, H, W] in [-1, 1], any H, W >= 1 (cast to fp16 like the reference's fp16
        model sees it).  Returns ``AutoencoderTinyOutput(latents=...)`` or ``(latents,)``: fp16 [B, 4, ceil(H / 2^k), ...],
        UNSCALED (diffusers' encode does not apply ``scaling_factor``; it is 1.0 for every published model anyway)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"encode: expected [B, 3, H, W], got {tuple(x.shape)}")
        if min(x.shape) < 1:
            raise ValueError(f"encode: empty input {tuple(x.shape)}")
        lat = self._encode(self._image_f32(x, self.device), None, False, 1, 1.0)
        return AutoencoderTinyOutput(latents=lat) if return_dict else (lat,)

    # ------------------------------------------------------------------ inpaint pre-processing
    def encode_inpaint(self, image: torch.Tensor, mask: torch.Tensor, *, normalize: bool = True, encode_image: bool = True,
                       encode_masked: bool = True, eps_image: Optional[torch.Tensor] = None,
                       eps_masked: Optional[torch.Tensor] = None) -> Dict[str, Optional[torch.Tensor]]:
        """``HipVAEEncoder.encode_inpaint`` on the tiny encoder: ``image`` [Bi, 3, H, W] float (in [0, 1] with ``normalize``,
        else already in [-1, 1]), ``mask`` [Bm, 1, H, W] (Bm in {1, Bi}; binarised at 0.5, 1 = repaint); both images go through
        ONE pass as one batch.  Returns ``image_latents`` and ``masked_image_latents`` ([Bi, 4, H/8, W/8] fp16, scaling_factor *
        latents; None where not encoded) and ``mask_latents`` [Bm, 1, H/8, W/8] fp16 (the nearest-sampled binarised mask).

        The encoder is deterministic (no posterior): ``eps_image`` / ``eps_masked`` are accepted and IGNORED.  That is a
        deliberate choice: ``pipeline.inpaint_draws`` still consumes its draws, so one generator gives the same ``noise``
        whichever encoder is installed.  (Later diffusers draws nothing for an encoder without ``latent_dist``; 0.23 cannot
        run an inpaint pipeline on AutoencoderTiny at all.)"""
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"encode_inpaint: image must be [B, 3, H, W], got {tuple(image.shape)}")
        Bi, _, H, Wd = image.shape
        if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != (H, Wd) or mask.shape[0] not in (1, Bi):
            raise ValueError(f"encode_inpaint: mask must be [1 or {Bi}, 1, {H}, {Wd}], got {tuple(mask.shape)}")
        if H % 8 or Wd % 8 or H <= 0 or Wd <= 0:
            raise ValueError(f"encode_inpaint needs a height and width that are multiples of 8 (got {H} x {Wd})")
        if self.downscale != 8:
            raise ValueError("encode_inpaint: the mask latents are sampled at every 8th pixel (vae_scale_factor 8); this "
                             f"encoder downsamples by {self.downscale}")
        blocks = (1 if encode_image else 0) | (2 if encode_masked else 0)
        if not blocks:
            raise ValueError("encode_inpaint: nothing to encode (encode_image and encode_masked are both False)")
        mask_lat = torch.empty(mask.shape[0], 1, H // 8, Wd // 8, dtype=torch.float16, device=self.device)
        lat = self._encode(self._image_f32(image, self.device), self._image_f32(mask, self.device), normalize, blocks,
                           self.config.scaling_factor, mask_latents=mask_lat)
        img = lat[:Bi] if encode_image else None
        msk = lat[Bi:] if encode_image and encode_masked else (lat if encode_masked else None)
        return {"image_latents": img, "masked_image_latents": msk, "mask_latents": mask_lat}
