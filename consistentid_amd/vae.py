"""HIP execution engine for the VAE decoder.

Replaces what the reference reaches through ``self.decode_latents(latents)``
(pipline_StableDiffusion_ConsistentID.py:587,:597 -> diffusers ``StableDiffusionPipeline.decode_latents``:
``latents / scaling_factor`` -> ``vae.decode`` -> ``(image / 2 + 0.5).clamp(0, 1)``).

Same design as the UNet engine: activations token-major fp16 ``[B, H*W, C]`` from the first conv to the last, every
op a kernel behind the C ABI (3x3 convs / linears / nearest-2x upsample fused into the following conv:
``cid_gemm_f16``; GroupNorm(+SiLU): ``cid_groupnorm_f16``).  The mid block's attention is ONE head of width C over
all latent pixels -- too wide for a register-resident flash kernel, and run once per image -- so it is four GEMMs
around a row softmax: S = Q K^T (scores, base-2 logits), softmax, V^T by a GEMM with the operand roles swapped,
O = P V.  Weight preparation at load: the 1/scaling_factor latent scale is folded into ``post_quant_conv``, the
attention scale and log2(e) into ``to_q``, the K bias is dropped (softmax is shift-invariant per row) and the V bias
moves through the softmax (rows of P sum to 1) into the output projection's bias.

SDXL's VAE sets ``force_upcast``: the reference decodes it in float32 (``upcast_vae()``,
pipline_StableDiffusionXL_ConsistentID.py:670-676).  ``HipVAEDecoderF32`` below is that decoder on the fp32 kernels
(``cid_gemm_f32`` / ``cid_groupnorm_f32`` / ``cid_softmax_rows_f32``, csrc/f32.hip): the same weight loading, blocks and
decode walk (``_HipVAEBlocks``, ``_HipVAEDecoderWalk``) with its own primitives, weight converters, head and tail;
``make_vae_decoder`` picks the engine from the config like the reference's ``needs_upcasting`` test does.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import ops
from .vae_spec import VAEConfig, decoder_blocks, encoder_blocks
from .weights import LOG2E, _conv3, _f, _h


class _HipVAEBlocks:
    """The building blocks the decoders and the encoder share, on token-major activations: ResnetBlock2D, the mid block's
    single-head attention and their weight loading, written on four primitives (``_gn``: GroupNorm(+SiLU), ``_conv``: 3x3
    convolution, ``_linear``, ``_softmax``) and two weight converters (``_t``: a plain tensor, ``_t3``: a 3x3 kernel,
    tap-major [Cout, 9 * Cin]).  The primitives and converters here are the fp16 ones; ``HipVAEDecoderF32`` replaces them.
    Subclasses fill ``W``, ``config`` and ``device``."""
    config: VAEConfig
    device: torch.device
    dtype = torch.float16
    W: Dict[str, torch.Tensor]
    _gn_ws: Optional[torch.Tensor]
    _gemm_ws: torch.Tensor

    # ------------------------------------------------------------------ fp16 primitives and converters
    def _t(self, t):
        return _h(t, self.device)

    def _t3(self, w):
        return _conv3(w, self.device)

    def _empty(self, *shape):
        return torch.empty(*shape, dtype=self.dtype, device=self.device)

    def _gn(self, x, c, B, HW, g, b, silu):
        need = ops.groupnorm_ws_bytes(B, c)
        if self._gn_ws is None or self._gn_ws.numel() < need:
            self._gn_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)   # arrival counters start at zero
        out = self._empty(B * HW, c)
        ops.groupnorm(x, out, g, b, self._gn_ws, B=B, HW=HW, c1=c, groups=self.config.norm_num_groups, eps=1e-6, silu=silu)
        return out

    def _conv(self, x, n, cin, cout, B, H, Wd, res=None, up=0):
        Ho, Wo = H << up, Wd << up
        out = self._empty(B * Ho * Wo, cout)
        ops.gemm(x, self.W[f"{n}.w"], out, M=B * Ho * Wo, N=cout, c1=cin, bias=self.W[f"{n}.b"], res=res,
                 ldr=cout if res is not None else 0, taps=9, Hi=H, Wi=Wd, Ho=Ho, Wo=Wo, stride=1, up=up, ws=self._gemm_ws)
        return out

    def _linear(self, x, w, b, M, N, c, res=None, out=None, ws=False):
        """x [M, c] @ w [N, c]^T (+ b) (+ res) -> ``out`` (a fresh [M, N] by default); ``ws``: with the split-K workspace"""
        out = self._empty(M, N) if out is None else out
        ops.gemm(x, w, out, M=M, N=N, c1=c, bias=b, res=res, ws=self._gemm_ws if ws else None)      # (res at pitch N)
        return out

    def _softmax(self, s, n):
        ops.softmax_rows(s, rows=n, cols=n, ld=n)

    # ------------------------------------------------------------------ weights
    def _load_resnet(self, sd: Dict[str, torch.Tensor], n: str):
        """weights of one ResnetBlock2D (temb-less, as in the VAE) into W under ``n``"""
        W, t = self.W, self._t
        for k in ("norm1", "norm2"):
            W[f"{n}.{k}.g"], W[f"{n}.{k}.b"] = t(sd[f"{n}.{k}.weight"]), t(sd[f"{n}.{k}.bias"])
        for k in ("conv1", "conv2"):
            W[f"{n}.{k}.w"], W[f"{n}.{k}.b"] = self._t3(sd[f"{n}.{k}.weight"]), t(sd[f"{n}.{k}.bias"])
        if f"{n}.conv_shortcut.weight" in sd:
            sw = sd[f"{n}.conv_shortcut.weight"]
            W[f"{n}.short.w"] = t(sw.reshape(sw.shape[0], sw.shape[1]))
            W[f"{n}.short.b"] = t(sd[f"{n}.conv_shortcut.bias"])

    def _load_attention(self, sd: Dict[str, torch.Tensor], a: str, c: int):
        """the mid block's single-head attention ``a`` into W["attn.*"], with the folds described in the module docstring"""
        W, t, dev = self.W, self._t, self.device
        W["attn.gn.g"], W["attn.gn.b"] = t(sd[f"{a}.group_norm.weight"]), t(sd[f"{a}.group_norm.bias"])
        qs = (c ** -0.5) * LOG2E
        W["attn.q.w"] = t(_f(sd[f"{a}.to_q.weight"], dev) * qs)
        W["attn.q.b"] = t(_f(sd[f"{a}.to_q.bias"], dev) * qs)
        W["attn.k.w"] = t(sd[f"{a}.to_k.weight"])                           # bias dropped: constant per score row
        W["attn.v.w"] = t(sd[f"{a}.to_v.weight"])
        wo = _f(sd[f"{a}.to_out.0.weight"], dev)
        W["attn.o.w"] = t(wo)
        W["attn.o.b"] = t(_f(sd[f"{a}.to_out.0.bias"], dev) + wo @ _f(sd[f"{a}.to_v.bias"], dev))

    # ------------------------------------------------------------------ blocks
    def _resnet(self, n, x, cin, cout, B, H, Wd):
        W, HW = self.W, H * Wd
        h = self._gn(x, cin, B, HW, W[f"{n}.norm1.g"], W[f"{n}.norm1.b"], True)
        h = self._conv(h, f"{n}.conv1", cin, cout, B, H, Wd)
        h = self._gn(h, cout, B, HW, W[f"{n}.norm2.g"], W[f"{n}.norm2.b"], True)
        sc = x if cin == cout else self._linear(x, W[f"{n}.short.w"], W[f"{n}.short.b"], B * HW, cout, cin, ws=True)
        return self._conv(h, f"{n}.conv2", cout, cout, B, H, Wd, res=sc)

    def _attention(self, x, c, B, HW):
        """single-head attention over all HW positions of each sample (diffusers Attention, residual_connection)"""
        W, M = self.W, B * HW
        t = self._gn(x, c, B, HW, W["attn.gn.g"], W["attn.gn.b"], False)
        q = self._linear(t, W["attn.q.w"], W["attn.q.b"], M, c, c)
        k = self._linear(t, W["attn.k.w"], None, M, c, c)
        o = self._empty(M, c)
        s, vt = self._empty(HW, HW), self._empty(c, HW)
        for b in range(B):
            rows = slice(b * HW, (b + 1) * HW)
            self._linear(q[rows], k[rows], None, HW, HW, c, out=s)               # S = Q K^T      [HW, HW]
            self._softmax(s, HW)
            self._linear(W["attn.v.w"], t[rows], None, c, HW, c, out=vt)         # V^T = Wv T^T   [C, HW]
            self._linear(s, vt, None, HW, c, HW, out=o[rows], ws=True)           # O = P V        [HW, C]
        return self._linear(o, W["attn.o.w"], W["attn.o.b"], M, c, c, res=x)


class _HipVAEDecoderWalk(_HipVAEBlocks):
    """What the two decoders share: the weight loading and the decode walk (mid block, up blocks, ``conv_norm_out``)
    between a head (``post_quant_conv`` + ``conv_in``: ``_load_head`` / ``_head``) and a tail (``conv_out`` to NCHW:
    ``_tail``) that each precision writes itself."""

    def __init__(self, cfg: VAEConfig, vae_sd: Dict[str, torch.Tensor], device="cuda:0"):
        self.config = cfg
        self.device = torch.device(device)
        sd = vae_sd
        W: Dict[str, torch.Tensor] = {}
        self.W = W
        with torch.cuda.device(self.device):
            self._load_head(sd)
            m = "decoder.mid_block"
            self._load_resnet(sd, f"{m}.resnets.0")
            self._load_resnet(sd, f"{m}.resnets.1")
            self._load_attention(sd, f"{m}.attentions.0", cfg.block_out_channels[-1])
            self.blocks = decoder_blocks(cfg)
            for name, cin, cout, n, up in self.blocks:
                for j in range(n):
                    self._load_resnet(sd, f"{name}.resnets.{j}")
                if up:
                    u = f"{name}.upsamplers.0.conv"
                    W[f"{u}.w"], W[f"{u}.b"] = self._t3(sd[f"{u}.weight"]), self._t(sd[f"{u}.bias"])
            W["norm_out.g"], W["norm_out.b"] = self._t(sd["decoder.conv_norm_out.weight"]), self._t(sd["decoder.conv_norm_out.bias"])
            W["conv_out.w"], W["conv_out.b"] = self._t3(sd["decoder.conv_out.weight"]), self._t(sd["decoder.conv_out.bias"])
        self._gn_ws: Optional[torch.Tensor] = None

    @torch.no_grad()
    def decode_tokens(self, latents: torch.Tensor):
        """latents [B, L, h, w] (UNSCALED, as the denoise loop leaves them) -> image token-major is internal; returns
        the decoded image [B, 3, 8h, 8w] NCHW in the VAE's [-1, 1] range, in the engine's dtype."""
        cfg, W = self.config, self.W
        lat = latents.to(device=self.device, dtype=self.dtype)
        B, L, H, Wd = lat.shape
        assert L == cfg.latent_channels
        c = cfg.block_out_channels[-1]
        x = lat.permute(0, 2, 3, 1).reshape(B * H * Wd, L).contiguous()        # 32 KB per image: host-side plumbing
        x = self._head(x, c, B, H, Wd)
        m = "decoder.mid_block"
        x = self._resnet(f"{m}.resnets.0", x, c, c, B, H, Wd)
        x = self._attention(x, c, B, H * Wd)
        x = self._resnet(f"{m}.resnets.1", x, c, c, B, H, Wd)
        for name, cin, cout, n, up in self.blocks:
            for j in range(n):
                x = self._resnet(f"{name}.resnets.{j}", x, cin if j == 0 else cout, cout, B, H, Wd)
            if up:
                x = self._conv(x, f"{name}.upsamplers.0.conv", cout, cout, B, H, Wd, up=1)
                H, Wd = 2 * H, 2 * Wd
            c = cout
        g = self._gn(x, c, B, H * Wd, W["norm_out.g"], W["norm_out.b"], True)
        return self._tail(g, c, B, H, Wd)

    def decode(self, z: torch.Tensor, return_dict: bool = False):
        """diffusers ``vae.decode(z)`` protocol: ``z`` is ALREADY divided by scaling_factor by the caller
        (pipline_StableDiffusionXL_ConsistentID.py:676); the fold in post_quant_conv is undone here."""
        if return_dict:
            raise NotImplementedError("return_dict=True (the reference passes return_dict=False)")
        return (self.decode_tokens(z * self.config.scaling_factor),)

    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        """``StableDiffusionPipeline.decode_latents`` up to the device tensor: [B, 3, H, W] in [0, 1]."""
        return (self.decode_tokens(latents) / 2 + 0.5).clamp(0, 1)


class HipVAEDecoder(_HipVAEDecoderWalk):
    def __init__(self, cfg: VAEConfig, vae_sd: Dict[str, torch.Tensor], device="cuda:0"):
        if cfg.force_upcast:
            raise NotImplementedError("force_upcast VAEs (SDXL) decode in fp32 in the reference: use HipVAEDecoderF32 "
                                      "(make_vae_decoder picks it)")
        super().__init__(cfg, vae_sd, device)
        self._gemm_ws = torch.empty(64 << 20, dtype=torch.uint8, device=self.device)

    def _load_head(self, sd):
        # post_quant_conv (1x1, L -> L) with the latent scale folded in, carried as the centre tap of a 3x3 conv
        # whose output is padded to 8 channels (the small-conv kernel's granule); conv_in reads those 8 channels
        cfg, W, dev = self.config, self.W, self.device
        L, c_mid = cfg.latent_channels, cfg.block_out_channels[-1]
        pq = _f(sd["post_quant_conv.weight"], dev).reshape(L, L) / cfg.scaling_factor
        w = torch.zeros(8, 9, L, device=dev)
        w[:L, 4, :] = pq
        W["pq.w"] = _h(w.reshape(8, 9 * L), dev)
        b = torch.zeros(8, device=dev)
        b[:L] = _f(sd["post_quant_conv.bias"], dev)
        W["pq.b"] = _h(b, dev)
        ci = _f(sd["decoder.conv_in.weight"], dev)                         # [C, L, 3, 3]
        w = torch.zeros(c_mid, 9, 8, device=dev)
        w[:, :, :L] = ci.permute(0, 2, 3, 1).reshape(c_mid, 9, L)
        W["conv_in.w"] = _h(w.reshape(c_mid, 72), dev)
        W["conv_in.b"] = _h(sd["decoder.conv_in.bias"], dev)

    def _head(self, x, c, B, H, Wd):
        W, L = self.W, self.config.latent_channels
        z = self._empty(B * H * Wd, 8)
        ops.conv3x3_small(x, z, W["pq.w"], W["pq.b"], B=B, Hi=H, Wi=Wd, cin=L, cout=8)
        x = self._empty(B * H * Wd, c)
        return ops.conv3x3_small(z, x, W["conv_in.w"], W["conv_in.b"], B=B, Hi=H, Wi=Wd, cin=8, cout=c)

    def _tail(self, g, c, B, H, Wd):
        W, co = self.W, self.config.out_channels
        return ops.conv_out(g, self._empty(B, co, H, Wd), W["conv_out.w"], W["conv_out.b"], B=B, H=H, W=Wd, cin=c, cout=co)


# ---------------------------------------------------------------------------------------------------------------- encoder
def fold_quant_conv(conv_w: torch.Tensor, conv_b: torch.Tensor, q_w: torch.Tensor, q_b: torch.Tensor):
    """quant_conv (1x1, 2L -> 2L) folded into encoder.conv_out (3x3, cin -> 2L): W' = Q W per tap, b' = Q b + q_b, in the
    dtype of the inputs (the engine passes fp32 and rounds W' once to fp16; the tests pass fp64).  Returns (W' [2L, cin, 3, 3],
    b' [2L])."""
    Q = q_w.reshape(q_w.shape[0], q_w.shape[1])
    return torch.einsum("oj,jcyx->ocyx", Q, conv_w), Q @ conv_b + q_b


def randn_tensor(shape, generator=None, device="cpu", dtype=torch.float16) -> torch.Tensor:
    """diffusers 0.23 ``randn_tensor``: a CPU generator draws on the CPU and the result is moved to ``device``; a generator on
    the device draws there; no generator draws from the device's default generator.  (Lists of per-sample generators are not
    built.)"""
    device = torch.device(device)
    if isinstance(generator, (list, tuple)):
        raise NotImplementedError("a list of generators (one per sample) is not supported: pass one torch.Generator")
    if generator is None:
        return torch.randn(shape, device=device, dtype=dtype)
    gdev = generator.device
    if gdev.type == "cpu":
        return torch.randn(shape, generator=generator, device="cpu", dtype=dtype).to(device)
    if gdev.type != device.type:
        raise ValueError(f"cannot draw on {device} with a generator on {gdev}")
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


class HipDiagonalGaussian:
    """diffusers ``DiagonalGaussianDistribution`` of an encoded batch (``vae.encode(x).latent_dist``): ``sample(generator)``
    and ``mode()`` return UNSCALED fp16 latents [B, L, h, w], computed by cid_vae_encode_out_f16 from the kept last
    activation (so the draw is the only thing that happens on the host); ``mean`` / ``logvar`` (clamped to [-30, 20]) /
    ``std`` / ``var`` come from the fp32 moments."""

    def __init__(self, encoder: "HipVAEEncoder", tokens: torch.Tensor, moments: torch.Tensor, B: int, h: int, w: int):
        self._enc, self._tokens, self._B, self._h, self._w = encoder, tokens, B, h, w
        self.parameters = moments
        L = encoder.config.latent_channels
        self.mean = moments[:, :L]
        self.logvar = moments[:, L:].clamp(-30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        self.deterministic = False

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        eps = randn_tensor(self.mean.shape, generator=generator, device=self._enc.device, dtype=torch.float16)
        return self._enc._posterior(self._tokens, self._B, self._h, self._w, eps=eps, scale=1.0)

    def mode(self) -> torch.Tensor:
        return self._enc._posterior(self._tokens, self._B, self._h, self._w, eps=None, scale=1.0)


@dataclass
class AutoencoderKLOutput:
    latent_dist: HipDiagonalGaussian


class HipVAEEncoder(_HipVAEBlocks):
    """fp16 HIP engine for ``AutoencoderKL.encode`` (the encoder, quant_conv and the posterior), which the inpaint pipelines
    run on the init image and on the masked image before the loop (pipelines/StableDIffusionInpaint_ConsistentID.py:231-295,
    StableDIffusionControlNetInpaint_ConsistentID.py:254-356 -> diffusers prepare_latents / prepare_mask_latents).

    conv_in runs with the inpaint pre-processing folded into its loads (cid_vae_encode_in_f16: normalisation, the binarised
    mask, image * (mask < 0.5), both images in one batch); the down blocks, Downsample2D(padding=0) (cid_gemm_f16 pad_mode 1),
    the mid block and conv_norm_out are the decoder's building blocks; conv_out, quant_conv (folded into conv_out's weights at
    load) and the posterior sample are one launch (cid_vae_encode_out_f16)."""

    def __init__(self, cfg: VAEConfig, vae_sd: Dict[str, torch.Tensor], device="cuda:0"):
        if cfg.force_upcast:
            raise NotImplementedError("force_upcast VAEs (SDXL) run in fp32 in the reference; the HIP encoder is fp16 only "
                                      "(there is no SDXL inpaint pipeline)")
        self.config = cfg
        self.device = torch.device(device)
        dev, sd = self.device, vae_sd
        W: Dict[str, torch.Tensor] = {}
        self.W = W
        boc, L = cfg.block_out_channels, cfg.latent_channels
        with torch.cuda.device(self.device):
            ci = sd["encoder.conv_in.weight"]                                   # [C0, 3, 3, 3]
            W["conv_in.w"] = _h(ci.permute(0, 2, 3, 1).reshape(ci.shape[0], 9 * ci.shape[1]), dev)
            W["conv_in.b"] = _h(sd["encoder.conv_in.bias"], dev)
            self.blocks = encoder_blocks(cfg)
            for name, cin, cout, n, down in self.blocks:
                for j in range(n):
                    self._load_resnet(sd, f"{name}.resnets.{j}")
                if down:
                    d = f"{name}.downsamplers.0.conv"
                    W[f"{d}.w"], W[f"{d}.b"] = _conv3(sd[f"{d}.weight"], dev), _h(sd[f"{d}.bias"], dev)
            m = "encoder.mid_block"
            self._load_resnet(sd, f"{m}.resnets.0")
            self._load_resnet(sd, f"{m}.resnets.1")
            self._load_attention(sd, f"{m}.attentions.0", boc[-1])
            W["norm_out.g"], W["norm_out.b"] = _h(sd["encoder.conv_norm_out.weight"], dev), _h(sd["encoder.conv_norm_out.bias"], dev)
            w, b = fold_quant_conv(_f(sd["encoder.conv_out.weight"], dev), _f(sd["encoder.conv_out.bias"], dev),
                                   _f(sd["quant_conv.weight"], dev), _f(sd["quant_conv.bias"], dev))
            W["conv_out.w"] = _conv3(w, dev)                                       # [2L, 9 * cin], rounded once
            W["conv_out.b"] = b.contiguous()                                       # fp32
            assert W["conv_out.w"].shape[0] == 2 * L
        self._gn_ws: Optional[torch.Tensor] = None
        self._gemm_ws = torch.empty(64 << 20, dtype=torch.uint8, device=self.device)

    def _check_size(self, H: int, W: int):
        if H % 8 or W % 8 or H <= 0 or W <= 0:
            raise ValueError(f"the VAE encoder needs a height and width that are multiples of 8 (got {H} x {W})")

    def _posterior(self, x, B, h, w, eps=None, scale=1.0, moments=None):
        L = self.config.latent_channels
        out = self._empty(B, L, h, w)
        if eps is not None:
            eps = eps.to(device=self.device, dtype=torch.float16).contiguous()
            if tuple(eps.shape) != (B, L, h, w):
                raise ValueError(f"eps {tuple(eps.shape)}: expected {(B, L, h, w)}")
        ops.vae_encode_out(x, out, self.W["conv_out.w"], self.W["conv_out.b"], B=B, H=h, W=w,
                           cin=self.config.block_out_channels[-1], L=L, scale=scale, eps=eps, moments=moments)
        return out

    @torch.no_grad()
    def _trunk(self, image: torch.Tensor, mask: Optional[torch.Tensor], normalize: bool, blocks: int,
               mask_latents: Optional[torch.Tensor] = None):
        """conv_in (pre-processing folded in) -> down blocks -> mid block -> conv_norm_out + SiLU: token-major
        [nblk * Bi * h * w, C] and (nblk * Bi, h, w)"""
        cfg, W = self.config, self.W
        Bi, _, H, Wd = image.shape
        self._check_size(H, Wd)
        B = Bi * bin(blocks).count("1")
        c = cfg.block_out_channels[0]
        x = self._empty(B * H * Wd, c)
        ops.vae_encode_in(image, x, W["conv_in.w"], W["conv_in.b"], mask=mask, normalize=normalize, blocks=blocks,
                          mask_latents=mask_latents)
        for name, cin, cout, n, down in self.blocks:
            for j in range(n):
                x = self._resnet(f"{name}.resnets.{j}", x, cin if j == 0 else cout, cout, B, H, Wd)
            if down:
                Ho, Wo = H // 2, Wd // 2
                y = self._empty(B * Ho * Wo, cout)
                d = f"{name}.downsamplers.0.conv"
                ops.gemm(x, W[f"{d}.w"], y, M=B * Ho * Wo, N=cout, c1=cout, bias=W[f"{d}.b"], taps=9, Hi=H, Wi=Wd,
                         Ho=Ho, Wo=Wo, stride=2, pad_mode=1, ws=self._gemm_ws)
                x, H, Wd = y, Ho, Wo
            c = cout
        m = "encoder.mid_block"
        x = self._resnet(f"{m}.resnets.0", x, c, c, B, H, Wd)
        x = self._attention(x, c, B, H * Wd)
        x = self._resnet(f"{m}.resnets.1", x, c, c, B, H, Wd)
        return self._gn(x, c, B, H * Wd, W["norm_out.g"], W["norm_out.b"], True), B, H, Wd

    @staticmethod
    def _image_f32(x: torch.Tensor, dev) -> torch.Tensor:
        return x.to(device=dev, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ diffusers protocol
    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """``vae.encode(x)``: ``x`` [B, 3, H, W] in [-1, 1] (the pipelines' pre-processed image; cast to fp16 like the
        reference's fp16 VAE sees it).  Returns ``AutoencoderKLOutput(latent_dist=...)``, or ``(latent_dist,)``."""
        if x.dim() != 4 or x.shape[1] != self.config.in_channels:
            raise ValueError(f"encode: expected [B, {self.config.in_channels}, H, W], got {tuple(x.shape)}")
        tokens, B, h, w = self._trunk(self._image_f32(x, self.device), None, False, 1)
        moments = torch.empty(B, 2 * self.config.latent_channels, h, w, dtype=torch.float32, device=self.device)
        self._posterior(tokens, B, h, w, eps=None, moments=moments)
        dist = HipDiagonalGaussian(self, tokens, moments, B, h, w)
        return AutoencoderKLOutput(latent_dist=dist) if return_dict else (dist,)

    # ------------------------------------------------------------------ inpaint pre-processing
    @torch.no_grad()
    def encode_inpaint(self, image: torch.Tensor, mask: torch.Tensor, *, normalize: bool = True, encode_image: bool = True,
                       encode_masked: bool = True, eps_image: Optional[torch.Tensor] = None,
                       eps_masked: Optional[torch.Tensor] = None) -> Dict[str, Optional[torch.Tensor]]:
        """What the inpaint pipelines do between their raw inputs and the loop, in one encoder pass with both images in one
        batch: ``image`` [Bi, 3, H, W] float (in [0, 1] with ``normalize``, else already in [-1, 1]), ``mask`` [Bm, 1, H, W]
        (Bm in {1, Bi}; binarised at 0.5, 1 = repaint).  Returns scaled ``image_latents`` and ``masked_image_latents``
        ([Bi, L, H/8, W/8] fp16, scaling_factor * (mean + std * eps); the mean where eps is None; None where not encoded) and
        ``mask_latents`` [Bm, 1, H/8, W/8] fp16 (the nearest-sampled binarised mask)."""
        if image.dim() != 4 or image.shape[1] != self.config.in_channels:
            raise ValueError(f"encode_inpaint: image must be [B, {self.config.in_channels}, H, W], got {tuple(image.shape)}")
        Bi, _, H, Wd = image.shape
        if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != (H, Wd) or mask.shape[0] not in (1, Bi):
            raise ValueError(f"encode_inpaint: mask must be [1 or {Bi}, 1, {H}, {Wd}], got {tuple(mask.shape)}")
        self._check_size(H, Wd)
        if 2 ** (len(self.config.block_out_channels) - 1) != 8:
            raise ValueError("encode_inpaint: the mask latents are sampled at every 8th pixel (vae_scale_factor 8); this VAE "
                             f"downsamples by {2 ** (len(self.config.block_out_channels) - 1)}")
        blocks = (1 if encode_image else 0) | (2 if encode_masked else 0)
        if not blocks:
            raise ValueError("encode_inpaint: nothing to encode (encode_image and encode_masked are both False)")
        mask_lat = self._empty(mask.shape[0], 1, H // 8, Wd // 8)
        tokens, B, h, w = self._trunk(self._image_f32(image, self.device), self._image_f32(mask, self.device), normalize,
                                      blocks, mask_latents=mask_lat)
        eps = None
        want = [e for e, on in ((eps_image, encode_image), (eps_masked, encode_masked)) if on]
        if any(e is not None for e in want):
            if any(e is None for e in want):
                raise ValueError("encode_inpaint: give eps for every encoded image or for none (the posterior mean)")
            eps = torch.cat([e.to(device=self.device, dtype=torch.float16) for e in want])
        lat = self._posterior(tokens, B, h, w, eps=eps, scale=self.config.scaling_factor)
        img = lat[:Bi] if encode_image else None
        msk = lat[Bi:] if encode_image and encode_masked else (lat if encode_masked else None)
        return {"image_latents": img, "masked_image_latents": msk, "mask_latents": mask_lat}


class HipVAEDecoderF32(_HipVAEDecoderWalk):
    """The same decoder in float32, for VAEs with ``force_upcast`` (SDXL): what the reference runs after
    ``upcast_vae()`` (pipline_StableDiffusionXL_ConsistentID.py:670-676).  Token-major fp32 activations, every op one of
    the three fp32 kernels of csrc/f32.hip; the weight folds (latent scale into post_quant_conv, attention scale and
    log2 e into to_q, K bias dropped, V bias through the softmax into the output bias) are the fp16 engine's."""
    dtype = torch.float32

    def _t(self, t):
        return _f(t, self.device).contiguous()

    def _t3(self, w):
        return self._t(w).permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()       # [Cout, 9 * Cin], tap-major

    def _gn(self, x, c, B, HW, g, b, silu):
        need = ops.groupnorm_f32_ws_bytes(B, HW, c)
        if self._gn_ws is None or self._gn_ws.numel() < need:
            self._gn_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = self._empty(B * HW, c)
        ops.groupnorm_f32(x, out, g, b, self._gn_ws, B=B, HW=HW, C_=c, groups=self.config.norm_num_groups, eps=1e-6, silu=silu)
        return out

    def _conv(self, x, n, cin, cout, B, H, Wd, res=None, up=0):
        out = self._empty(B * (H << up) * (Wd << up), cout)
        ops.gemm_f32(x, self.W[f"{n}.w"], out, M=out.shape[0], N=cout, c=cin, bias=self.W[f"{n}.b"], res=res, taps=9, Hi=H, Wi=Wd, up=up)
        return out

    def _linear(self, x, w, b, M, N, c, res=None, out=None, ws=False):
        out = self._empty(M, N) if out is None else out
        ops.gemm_f32(x, w, out, M=M, N=N, c=c, bias=b, res=res)
        return out

    def _softmax(self, s, n):
        ops.softmax_rows_f32(s, rows=n, cols=n, ld=n)

    def _load_head(self, sd):
        cfg, W, L = self.config, self.W, self.config.latent_channels
        W["pq.w"] = (self._t(sd["post_quant_conv.weight"]).reshape(L, L) / cfg.scaling_factor).contiguous()
        W["pq.b"] = self._t(sd["post_quant_conv.bias"])
        W["conv_in.w"], W["conv_in.b"] = self._t3(sd["decoder.conv_in.weight"]), self._t(sd["decoder.conv_in.bias"])

    def _head(self, x, c, B, H, Wd):
        L = self.config.latent_channels
        z = self._linear(x, self.W["pq.w"], self.W["pq.b"], B * H * Wd, L, L)
        return self._conv(z, "conv_in", L, c, B, H, Wd)

    def _tail(self, g, c, B, H, Wd):
        co = self.config.out_channels
        img = self._conv(g, "conv_out", c, co, B, H, Wd)                           # [B * H * W, 3]
        return img.view(B, H, Wd, co).permute(0, 3, 1, 2).contiguous()             # NCHW for the caller (plumbing)


def make_vae_decoder(cfg: VAEConfig, vae_sd: Dict[str, torch.Tensor], device="cuda:0"):
    """fp32 engine for ``force_upcast`` VAEs (the reference's ``needs_upcasting`` test, SDXL :670), fp16 engine otherwise"""
    return (HipVAEDecoderF32 if cfg.force_upcast else HipVAEDecoder)(cfg, vae_sd, device)
