"""HIP execution engine for the UNet denoiser with ConsistentID identity injection.

Drop-in for the object the reference pipelines call as
``self.unet(latent_model_input, t, encoder_hidden_states=..., cross_attention_kwargs=...,
added_cond_kwargs=..., down_block_additional_residuals=..., mid_block_additional_residual=...)
.sample``  (pipline_StableDiffusion_ConsistentID.py:552-557, SDXL :634-641,
pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:418-425).

Design (MI355X-first, not a module tree):
  * activations are token-major fp16 ``[B, H*W, C]`` end to end, so ResNet <-> Transformer
    transitions are free (no NCHW permutes) and skip concatenation is done by giving the
    consumer kernels two source pointers instead of copying;
  * every op is a hand-written HIP kernel behind the C ABI (ops.py -> libcid.so);
  * weights are packed once (weights.py); cross-attention K/V of each embed set are
    projected + packed once per generation (``set_context``), not once per step;
  * the whole step is allocation-stable and sync-free, so one hipGraph (torch.cuda.CUDAGraph
    capturing the same HIP stream) replays it for every timestep: the timestep value,
    DDIM coefficients and the K/V row selector live in device buffers.
"""
from __future__ import annotations

import itertools
import math
import os

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .unet_spec import PAG_DEFAULT_LAYERS, BlockSpec, ResnetSpec, TransformerSpec, UNetConfig, pag_blocks, walk
from .weights import PackedUNet


@dataclass
class UNetOutput:
    sample: torch.Tensor


class _Ctx:
    """packed K/V of one set of encoder_hidden_states rows, per cross-attention layer"""

    def __init__(self):
        self.kp: Dict[str, torch.Tensor] = {}
        self.vp: Dict[str, torch.Tensor] = {}
        # generation (0 / 2 / 3) of the fused kernel whose K/V operand layout the layer holds, or LONG_CONTEXT
        self.v2: Dict[str, int] = {}
        self.rows = 0
        self.n_txt = 0
        self.n_ip = 0
        # implicit cache of __call__: (address, version, shape) of the caller's tensor.  The tensor itself is kept alive in
        # key_ref: without the strong reference the caching allocator may hand the same address (version 0, same shape)
        # to the NEXT prompt's embeddings and the stale K/V would be served
        self.key = None
        self.key_ref = None


LONG_CONTEXT = 4    # _Ctx.v2 value: the K/V images are those of the long-context kernel (more than 96 context rows)


def _tensor_key(t: torch.Tensor):
    return t.data_ptr(), t._version, tuple(t.shape)


def fused_gen1(c: int, tokens: int, fused_max_c: int = 320) -> bool:
    """one launch of the first-generation fused cross-attention kernel instead of LN + GEMM + core + GEMM, where the third
    generation does not serve?  (HipUNet._fused_gen1 with the engine's CID_XATTN_FUSED_MAX_C; the measurements are there)"""
    return c <= fused_max_c or (c <= 640 and tokens >= 16384 and fused_max_c >= 320)


def guidance_scale_embedding(w, dim: int, device="cpu") -> torch.Tensor:
    """diffusers' ``get_guidance_scale_embedding`` (LatentConsistencyModelPipeline; w = guidance_scale - 1) -> fp32 [1, dim]:
    1000 w exp(-ln(10000) / (dim / 2 - 1) arange(dim / 2)) as [sin | cos], zero-padded to an odd ``dim``.  What a UNet with
    ``time_cond_proj_dim`` = dim projects (``time_embedding.cond_proj``, no bias) and adds to the timestep's sinusoid row."""
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float32, device=device) * -(math.log(10000.0) / (half - 1)))
    arg = (torch.tensor([1000.0 * float(w)], dtype=torch.float32, device=device))[:, None] * freq[None, :]
    emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
    return torch.nn.functional.pad(emb, (0, 1)) if dim % 2 else emb


class HipUNet:
    _serials = itertools.count(1)       # one number per object ever built (id() is recycled after garbage collection)

    def __init__(self, cfg: UNetConfig, unet_sd: Optional[Dict[str, torch.Tensor]] = None,
                 adapter_sd: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0",
                 num_tokens: int = 4, lora_scale: float = 1.0, packed: Optional[PackedUNet] = None,
                 encoder_only: bool = False, keep_base: bool = False):
        self.config = cfg
        self.device = torch.device(device)
        self.dtype = torch.float16
        self.num_tokens = num_tokens
        if packed is not None:          # weights received through distributed.broadcast_weights
            self.packed = packed
        else:
            with torch.cuda.device(self.device):
                self.packed = PackedUNet(cfg, unet_sd, adapter_sd, self.device, lora_scale, encoder_only=encoder_only,
                                         keep_base=keep_base)
        self.W = self.packed.w
        self.downs, self.mid, self.ups = walk(cfg)
        if self.packed.encoder_only:
            self.ups = []
        self._ctx = _Ctx()
        # what a captured denoise step bakes in of this object (denoise.captured_reads): which object it is, and an epoch
        # that counts every change of a host-side launch argument (ip_scale) and every move of the K/V buffers
        self.serial = next(HipUNet._serials)
        self.epoch = 0
        self._gn_ws: Optional[torch.Tensor] = None
        self._gemm_ws = torch.empty(ops.GEMM_WS_BYTES, dtype=torch.uint8, device=self.device)   # split-K partials
        # widest level that runs the one-launch fused ID cross-attention (wider levels: GEMMs around the core)
        self._xattn_fused_max_c = int(os.environ.get("CID_XATTN_FUSED_MAX_C", "320"))
        self._cfg_dedup = os.environ.get("CID_CFG_DEDUP", "1") != "0"
        self._qattn = os.environ.get("CID_QATTN", "1") != "0"      # A/B switch: query projection with the attention epilogue
        # A/B switch: generation of the fused cross-attention kernel at the SD1.5 level-0 geometry (3: xattn3.hip,
        # 1: the first-generation xattn.hip); CID_XATTN_V2=0 is the older spelling of generation 1
        self._xattn_gen = ops.xattn_generation()
        self._t_buf = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._freeu = None      # (s1, s2, b1, b2) while FreeU is enabled
        self._pag: tuple = ()   # the transformer blocks whose attn1 is the identity on perturbed rows (enable_pag)
        # time_cond_proj_dim: cond_proj(guidance embedding) [1, c0] of the current generation, at a stable address
        self._cond_row: Optional[torch.Tensor] = None

    def set_guidance_embedding(self, guidance_scale: float) -> torch.Tensor:
        """A UNet with ``time_cond_proj_dim`` (a distilled latent consistency model): the row ``time_embedding.cond_proj``
        adds to every timestep's sinusoid, [1, c0] fp16, for w = guidance_scale - 1.  Once per generation: the embedding in
        fp32 torch, cast to fp16 as diffusers hands it to the UNet, the projection on cid_linear_small_f16."""
        dim = self.config.time_cond_proj_dim
        assert dim is not None, "set_guidance_embedding: the UNet has no time_cond_proj_dim"
        c0 = self.config.block_out_channels[0]
        if self._cond_row is None:
            self._cond_row = torch.zeros(1, c0, dtype=torch.float16, device=self.device)
        w_emb = guidance_scale_embedding(float(guidance_scale) - 1.0, dim, self.device).half().contiguous()
        ops.linear_small(w_emb, self.W["time_embedding.cond_proj.w"], None, self._cond_row, M=1, N=c0, K=dim)
        return self._cond_row

    def _add_guidance(self, sc: torch.Tensor):
        """sinusoid rows += the guidance row, in front of linear_1 (nothing without time_cond_proj_dim)"""
        if self.config.time_cond_proj_dim is not None:
            if self._cond_row is None:
                raise RuntimeError("a UNet with time_cond_proj_dim needs its guidance embedding first: "
                                   "set_guidance_embedding(guidance_scale) (the denoise engine does that in every generation)")
            ops.add_inplace(sc, self._cond_row)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' ``enable_freeu`` (0.23, UNet2DConditionModel): the inputs of every resnet of up block i in {0, 1} go
        through cid_freeu_f16 -- the skip tensor through the low-frequency filter with scale s_{i+1}, the first half of the
        backbone's channels times b_{i+1}.  The four values are launch scalars kept on the host: captured steps hold the
        old ones, so the epoch moves (and the workspace may grow)."""
        vals = tuple(float(v) for v in (s1, s2, b1, b2))
        if vals != self._freeu:
            self._freeu = vals
            self.epoch += 1
        return self

    def disable_freeu(self):
        if self._freeu is not None:
            self._freeu = None
            self.epoch += 1
        return self

    def enable_pag(self, layers=PAG_DEFAULT_LAYERS):
        """Perturbed-attention guidance (arXiv 2403.17377; diffusers' ``pag_applied_layers``): select the self-attention
        layers that skip their attention map on the perturbed rows of a forward (``forward_tokens(pag_rows=)``) --
        ``unet_spec.pag_blocks`` resolves the ids, an unknown one raises ValueError -- and build their folded
        ``to_out . to_v`` weights (``PackedUNet.set_pag``; RuntimeError without ``keep_base=True``).  Rows that are not
        perturbed, and forwards without perturbed rows, launch what they always launched.  A captured step holds the
        selection it was captured under, so the epoch moves when it changes."""
        blocks = tuple(pag_blocks(self.config, layers))
        if self.packed.encoder_only:
            raise NotImplementedError("enable_pag: a ControlNet encoder takes no perturbed rows")
        if blocks != self._pag:
            with torch.cuda.device(self.device):
                self.packed.set_pag(blocks)
            self._pag = blocks
            self.epoch += 1
        return self

    def disable_pag(self):
        """drop the selection and the folded weights of :meth:`enable_pag`"""
        if self._pag:
            self.packed.set_pag(())
            self._pag = ()
            self.epoch += 1
        return self

    @property
    def pag_layers(self) -> tuple:
        """the selected transformer blocks (``<transformer>.transformer_blocks.<k>``), () while PAG is off"""
        return self._pag

    def load_adapter_modules(self, adapter_sd: Dict[str, torch.Tensor], lora_scale: Optional[float] = None):
        """``adapter_modules`` of a ConsistentID checkpoint -> packed weights, in place (needs ``keep_base=True``);
        the cached cross-attention K/V are dropped because the K/V projections changed."""
        with torch.cuda.device(self.device):
            self.packed.load_adapter_modules(adapter_sd, lora_scale)
        self._ctx.key = self._ctx.key_ref = None
        self.epoch += 1         # ip_scale is a launch argument kept on the host: captured steps hold its old value
        return self

    def require_base(self):
        """raise the RuntimeError of :meth:`set_lora` now, before a caller changes anything else"""
        self.packed.require_base()

    def set_lora(self, entries):
        """the active community LoRA entries ``[(modules, weight), ...]`` (lora.parse_lora's ``unet`` part) -> packed weights,
        in place (``PackedUNet.set_lora``; needs ``keep_base=True``); ``[]`` restores the base.  The cached cross-attention
        K/V are dropped because the K/V projections changed.  No address and no host-side launch argument changes, so the
        epoch stays."""
        with torch.cuda.device(self.device):
            self.packed.set_lora(entries)
        self._ctx.key = self._ctx.key_ref = None
        return self

    # -- attributes the reference pipelines read
    @property
    def in_channels(self) -> int:
        return self.config.in_channels

    def to(self, *a, **k):
        return self

    # ------------------------------------------------------------------ context (K/V cache)
    def set_context(self, ehs: torch.Tensor, num_tokens: Optional[int] = None):
        """Project + pack cross-attention K/V for ``ehs`` [R, L, Dc] (L = text + ID tokens).
        Replaces the per-step to_k/to_v/to_k_ip/to_v_ip GEMMs of attention.py:249-250,266-269."""
        nt = self.num_tokens if num_tokens is None else num_tokens
        given, ehs = ehs, ehs.to(device=self.device, dtype=torch.float16).contiguous()
        R, L, _ = ehs.shape
        # more than 96 context rows (weighted / chunked prompts of 77 k rows): every layer is packed for the long-context
        # kernel (csrc/xattn_long.hip), whose caps are checked here, before anything is launched or changed
        long_ctx = L > ops.XATTN_SHORT_MAX
        if long_ctx:
            # (a context without ID rows -- a ControlNet's: the pipeline's text AND ID rows as one stream -- may be longer
            # by the ID tile's slots, or a prompt at the cap would be refused by its ControlNet)
            cap = ops.xattn_long_max_txt() + (0 if nt else ops.XATTN_LONG_MAX_IP)
            if L - nt > cap or L - nt < 1 or not 0 <= nt <= ops.XATTN_LONG_MAX_IP:
                raise ValueError(f"set_context: {L - nt} text rows + {nt} ID rows; the cross-attention kernels take at most "
                                 f"{cap} text rows and {ops.XATTN_LONG_MAX_IP} ID rows")
        ctx = self._ctx
        ctx.rows, ctx.n_txt, ctx.n_ip = R, L - nt, nt
        moved = False
        for b in self.packed.xattn_layers:
            wt = self.W[f"{b}.attn2.kv_txt.w"]
            C_ = wt.shape[0] // 2
            heads = self._heads_of(b)
            # fragment order of the third-generation fused kernel (SD1.5 level 0) where it serves
            v3 = (not long_ctx and self._xattn_gen >= 3 and f"{b}.attn2.wq_p" in self.W
                  and ops.id_xattn3_supported(C_, heads, ctx.n_txt, ctx.n_ip))
            # (the buffers of the last context are reused: addresses stay stable across generations)
            ctx.kp[b], ctx.vp[b], new = ops.context_kv(ehs, wt, self.W[f"{b}.attn2.kv_ip.w"], R=R, L=L, C_=C_, heads=heads,
                                                       n_txt=ctx.n_txt, n_ip=ctx.n_ip, v3=v3, kp=ctx.kp.get(b),
                                                       vp=ctx.vp.get(b), long=long_ctx)
            moved |= new
            ctx.v2[b] = LONG_CONTEXT if long_ctx else 3 if v3 else 0
        ctx.key, ctx.key_ref = _tensor_key(given), given
        if moved:       # the allocator may hand an old address out again: the addresses alone do not tell
            self.epoch += 1
        return self

    def refresh_context(self, ehs: torch.Tensor, num_tokens: Optional[int] = None):
        """:meth:`set_context` unless ``ehs`` is the tensor the kept K/V were computed from: the same object, unchanged
        (address, version, shape)"""
        if self._ctx.key != _tensor_key(ehs) or self._ctx.key_ref is not ehs:
            self.set_context(ehs, num_tokens)

    def context_addresses(self):
        """the device addresses and scalar launch arguments a captured step reads from this object besides its weights: the
        packed K/V of every cross-attention layer, the GroupNorm workspace (``reserve_workspace``) and the context lengths"""
        ws = 0 if self._gn_ws is None else self._gn_ws.data_ptr()
        return (tuple(t.data_ptr() for t in self._ctx.kp.values()) + tuple(t.data_ptr() for t in self._ctx.vp.values())
                + (ws, self._ctx.n_txt, self._ctx.n_ip))

    def reserve_workspace(self, B: int):
        """size the GroupNorm workspace for a forward of batch ``B`` now, so that its address is known before the first step"""
        self._ws(B)

    def mid_size(self, h: int, w: int) -> tuple:
        """(H_mid, W_mid) of the mid block for latents of ``h`` x ``w``: every down block's sampler halves both"""
        for blk in self.downs:
            if blk.sampler:
                h, w = h // 2, w // 2
        return h, w

    def _heads_of(self, block_name: str) -> int:
        for blk in self.downs + [self.mid] + self.ups:
            for t in blk.attentions:
                if block_name.startswith(t.name + "."):
                    return t.heads
        raise KeyError(block_name)

    # ------------------------------------------------------------------ forward
    def _ws(self, B: int) -> torch.Tensor:
        need = ops.groupnorm_ws_bytes(B, 2560)
        if self._freeu is not None:     # cid_freeu_f16's partial sums share the scratch: launches on one stream, each done with it
            need = max([need] + [ops.freeu_ws_bytes(B, c, 1024, 1024) for c in set(self.config.block_out_channels)])
        if self._gn_ws is None or self._gn_ws.numel() < need:
            self._gn_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return self._gn_ws

    def _empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float16, device=self.device)

    def _ln(self, b: str, which: str):
        """(s, b', eps) of a LayerNorm folded into projection ``which`` of transformer block ``b`` (weights.fold_ln)"""
        return (self.W[f"{b}.{which}s"].view(torch.float32), self.W[f"{b}.{which}b"].view(torch.float32), ops.LN_EPS)

    def _gn(self, x1, c1, B, HW, g, b, eps, silu, x2=None, c2=0):
        out = self._empty(B * HW, c1 + c2)
        ops.groupnorm(x1, out, g, b, self._ws(B), B=B, HW=HW, c1=c1, x2=x2, c2=c2,
                      groups=self.config.norm_num_groups, eps=eps, silu=silu)
        return out

    def _resnet(self, r: ResnetSpec, x, skip, c_x, c_skip, B, H, Wd, temb_all, temb_rows, rep: int = 1):
        """``rep`` = 2: the output is wanted twice (the CFG batch's two halves share it so far) -- conv2 writes both copies
        (cid_gemm_desc.out2) and the result is [2 * B * HW, cout], its first half being the B-sample tensor"""
        W, n = self.W, r.name
        HW = H * Wd
        M = B * HW
        cin = c_x + c_skip
        assert cin == r.cin, (n, cin, r.cin)
        h = self._gn(x, c_x, B, HW, W[f"{n}.norm1.g"], W[f"{n}.norm1.b"], self.config.norm_eps, True, skip, c_skip)
        h1 = self._empty(M, r.cout)
        off = self.packed.temb_offsets[n]
        rps = HW if temb_rows > 1 else M   # shared timestep row vs per-sample rows (SDXL)
        ops.gemm(h, W[f"{n}.conv1.w"], h1, M=M, N=r.cout, c1=cin, bias=W[f"{n}.conv1.b"],
                 rowbias=temb_all[:, off:], ld_rowbias=self.packed.temb_total, rows_per_sample=rps,
                 taps=9, Hi=H, Wi=Wd, Ho=H, Wo=Wd, ws=self._gemm_ws, gn_hw=HW)      # (norm2 reads h1)
        h2 = self._gn(h1, r.cout, B, HW, W[f"{n}.norm2.g"], W[f"{n}.norm2.b"], self.config.norm_eps, True)
        if r.cin != r.cout:
            sc = self._empty(M, r.cout)
            ops.gemm(x, W[f"{n}.short.w"], sc, M=M, N=r.cout, c1=c_x, x2=skip, c2=c_skip, bias=W[f"{n}.short.b"],
                     ws=self._gemm_ws)
        else:
            assert skip is None
            sc = x
        full = self._empty(rep * M, r.cout)
        out = full[:M] if rep == 2 else full
        ops.gemm(h2, W[f"{n}.conv2.w"], out, M=M, N=r.cout, c1=r.cout, bias=W[f"{n}.conv2.b"], res=sc, ldr=r.cout,
                 taps=9, Hi=H, Wi=Wd, Ho=H, Wo=Wd, ws=self._gemm_ws, gn_hw=HW,      # (a GroupNorm reads every resnet output)
                 out2=full[M:] if rep == 2 else None)
        if rep == 2:
            out._cfg_full = full
        return out

    def _dup(self, t: torch.Tensor, rep: int) -> torch.Tensor:
        """[rows, c] -> [rep * rows, c], the CFG ``torch.cat([x] * 2)`` of a tensor both halves share"""
        out = self._empty(rep * t.shape[0], t.shape[1])
        out.view(rep, -1).copy_(t.reshape(1, -1).expand(rep, -1))
        return out

    def _attn1_core(self, t: TransformerSpec, b: str, h, Bs: int, N: int, N_real: int, sag=None):
        """fused q / k / v projection of LayerNorm1(``h``) and the self-attention of ``Bs`` samples of N tokens -> [Bs * N, c].
        ``sag`` = (mass fp32 [rows, N_real], first_row, rows): the column mass of the attention map of samples
        [first_row, first_row + rows) is written there (cid_attn_colmass_f16) while q and k are still in their buffer."""
        W, c = self.W, t.channels
        d = c // t.heads
        M = Bs * N
        qk = self._empty(M, 2 * c)
        vt = self._empty(Bs * t.heads * ops.dvp_of(d) * N)
        if ops.ln_fold(M):     # norm1 folded into the projection: the GEMM reads the residual stream itself
            ops.gemm(h, W[f"{b}.attn1.qkv.wl"], qk, M=M, N=3 * c, c1=c, mode=2, vt=vt, n_vt0=2 * c,
                     heads=t.heads, dhead=d, ntok=N, ln=self._ln(b, "attn1.qkv.ln"))
        else:
            ln = self._empty(M, c)
            ops.layernorm(h, ln, W[f"{b}.norm1.g"], W[f"{b}.norm1.b"], M=M, C_=c)
            ops.gemm(ln, W[f"{b}.attn1.qkv.w"], qk, M=M, N=3 * c, c1=c, mode=2, vt=vt, n_vt0=2 * c,
                     heads=t.heads, dhead=d, ntok=N)
        ao = self._empty(M, c)
        ops.self_attn(qk, qk[:, c:], vt, ao, B=Bs, N=N, heads=t.heads, d=d, ldq=2 * c, ldk=2 * c, ldo=c,
                      n_keys=N_real)
        if sag is not None:
            mass, first, rows = sag
            assert 0 <= first and first + rows <= Bs and tuple(mass.shape) == (rows, N_real), (first, rows, Bs, mass.shape, N_real)
            qs = qk[first * N:(first + rows) * N]
            # a padded token axis: the kernel's rows are N wide (pad columns 0); the real columns are copied out
            wide = mass if N == N_real else torch.empty(rows, N, dtype=torch.float32, device=self.device)
            ops.attn_colmass(qs, qs[:, c:], wide, B=rows, N=N, heads=t.heads, d=d, ldq=2 * c, ldk=2 * c, n_keys=N_real)
            if wide is not mass:
                mass.copy_(wide[:, :N_real])
        return ao

    def _attn1_perturbed(self, t: TransformerSpec, b: str, h, B: int, N: int, N_real: int, pag_rows: int):
        """``h + attn1(LN1(h))`` of a block PAG selects: the leading B - pag_rows samples run the attention as ever -- their
        token-major rows are one contiguous range, pad rows of a padded token axis included -- and the trailing ``pag_rows``
        samples take identity attention, to_out(to_v(LN1(h))): ONE GEMM on the pre-multiplied weight (weights.fold_vo) with the
        residual in its epilogue; no q / k / v projection, no attention and no out projection run for them."""
        W, P, c = self.W, self.packed.pag, t.channels
        lead = B - pag_rows
        Ml, Mp = lead * N, pag_rows * N
        h2 = self._empty(B * N, c)
        if lead:
            ao = self._attn1_core(t, b, h[:Ml], lead, N, N_real)
            ops.gemm(ao, W[f"{b}.attn1.out.w"], h2[:Ml], M=Ml, N=c, c1=c, bias=W[f"{b}.attn1.out.b"], res=h[:Ml], ldr=c)
        hp = h[Ml:]
        if ops.ln_fold(Mp):     # norm1 folded: the GEMM reads the residual stream itself (to_out's bias is inside lnb)
            ln = (P[f"{b}.attn1.vo.lns"].view(torch.float32), P[f"{b}.attn1.vo.lnb"].view(torch.float32), ops.LN_EPS)
            ops.gemm(hp, P[f"{b}.attn1.vo.wl"], h2[Ml:], M=Mp, N=c, c1=c, ln=ln, res=hp, ldr=c)
        else:
            ln1 = self._empty(Mp, c)
            ops.layernorm(hp, ln1, W[f"{b}.norm1.g"], W[f"{b}.norm1.b"], M=Mp, C_=c)
            ops.gemm(ln1, P[f"{b}.attn1.vo.w"], h2[Ml:], M=Mp, N=c, c1=c, bias=W[f"{b}.attn1.out.b"], res=hp, ldr=c)
        return h2

    def _transformer(self, t: TransformerSpec, x, B, H, Wd, kvrow, Bp: Optional[int] = None, pag_rows: int = 0, sag=None):
        """``sag``: ``_attn1_core``'s, for the first transformer block (self-attention guidance reads the mid block's).
        ``pag_rows`` > 0: the trailing ``pag_rows`` samples of the batch are perturbed -- in the blocks ``enable_pag``
        selected their self-attention is the identity (``_attn1_perturbed``); every other block runs all rows as ever.
        ``Bp`` < B: the rows of ``x`` are the Bp distinct samples of a CFG batch B = rep * Bp whose halves were identical
        so far (same latents, same timestep).  Everything up to the first cross-attention -- the first place the two
        halves see different inputs -- runs once on Bp samples and is then repeated; the result is the same tensor the
        full batch would produce, row for row."""
        W, n, c = self.W, t.name, t.channels
        N = H * Wd
        ctx = self._ctx
        Bc = B if Bp is None else Bp          # batch of the part computed so far
        g = self._gn(x, c, Bc, N, W[f"{n}.norm.g"], W[f"{n}.norm.b"], 1e-6, False)
        # The attention kernels tile the token axis (64 keys per step; 128 / 64 tokens per workgroup in the fused
        # cross-attention).  512^2 and 1024^2 images give multiples at every level; other sizes run the block on a
        # zero-padded token axis: every other op of the block is row-wise, the self-attention masks the pad keys
        # (cid_self_attn_keys_f16), and the pad rows are dropped at the end.
        gens = {ctx.v2.get(f"{n}.transformer_blocks.{k}", 0) for k in range(t.n_layers)}
        # (the long-context core tiles 32 tokens; the self-attention's 64 decide there)
        need = 128 if (2 in gens or (c <= self._xattn_fused_max_c and c > 128 and not gens <= {3, LONG_CONTEXT})) else 64
        N_real = N
        if N % need:
            N = (N + need - 1) // need * need

            def pad(tn):
                o = torch.zeros(tn.shape[0] // N_real, N, c, dtype=torch.float16, device=self.device)
                o[:, :N_real] = tn.view(-1, N_real, c)
                return o.view(-1, c)
            g, x = pad(g), pad(x)
        M = Bc * N
        h = self._empty(M, c)
        ops.gemm(g, W[f"{n}.proj_in.w"], h, M=M, N=c, c1=c, bias=W[f"{n}.proj_in.b"])
        for k in range(t.n_layers):
            b = f"{n}.transformer_blocks.{k}"
            # --- self attention (Consistent_AttProcessor, attention.py:110-174)
            rep = B // Bc
            mass = sag if k == 0 else None
            # (the mass is taken from a block that runs the whole batch through one attention launch; only the mid block is asked)
            assert mass is None or (Bc == B and not (pag_rows > 0 and b in self._pag)), "sag on a de-duplicated or perturbed block"
            if pag_rows > 0 and b in self._pag:     # identity attention on the trailing pag_rows samples
                assert Bc == B, "a perturbed block runs on the whole batch (forward_tokens keeps it out of the de-duplication)"
                h2 = self._attn1_perturbed(t, b, h, B, N, N_real, pag_rows)
            elif rep == 2:    # the halves part ways at the cross-attention: the out projection writes the shared stream twice
                ao = self._attn1_core(t, b, h, Bc, N, N_real)
                h2 = self._empty(2 * M, c)
                ops.gemm(ao, W[f"{b}.attn1.out.w"], h2[:M], M=M, N=c, c1=c, bias=W[f"{b}.attn1.out.b"], res=h, ldr=c, out2=h2[M:])
            else:
                ao = self._attn1_core(t, b, h, Bc, N, N_real, sag=mass)
                h2 = self._empty(M, c)
                ops.gemm(ao, W[f"{b}.attn1.out.w"], h2, M=M, N=c, c1=c, bias=W[f"{b}.attn1.out.b"], res=h, ldr=c)
            if Bc != B:     # ... and the block input (the residual of proj_out) exists twice already where its producer wrote it so
                if rep != 2:
                    h2 = self._dup(h2, rep)
                full = getattr(x, "_cfg_full", None)
                x = full if full is not None and full.shape[0] == rep * x.shape[0] else self._dup(x, rep)
                Bc, M = B, B * N
            # --- identity cross attention (Consistent_IPAttProcessor, attention.py:207-294) inside x + attn2(LN(x), ehs)
            gn_hw = N if N == N_real else 0
            # the last block's ff2 and proj_out as one GEMM over the row [ff | h3]: both live in ONE
            # [M, 5c] buffer, written at pitch 5c by their producers (the first-generation fused kernel has no pitched form)
            fold = (k == t.n_layers - 1 and ops.ff2_fold(M, c, gn_hw)
                    and (ctx.v2.get(b) in (3, LONG_CONTEXT) or not self._fused_gen1(c, M)))
            buf = self._empty(M, 5 * c) if fold else None
            ldh = 5 * c if fold else c
            h3 = self.cross_attention(b, h2, B, N, c, t.heads, kvrow, out=buf[:, 4 * c:] if fold else None)
            # --- feed forward (GEGLU)
            ff = buf if fold else self._empty(M, 4 * c)
            if ops.ln_fold_geglu(M, c):     # norm3 folded into the GEGLU projection
                ops.gemm(h3, W[f"{b}.ff1.wl"], ff, M=M, N=8 * c, c1=c, ld1=ldh, ldo=ldh if fold else None, mode=1,
                         ln=self._ln(b, "ff1.ln"))
            else:
                ln3 = self._empty(M, c)
                ops.layernorm(h3, ln3, W[f"{b}.norm3.g"], W[f"{b}.norm3.b"], M=M, C_=c, ldx=ldh if fold else None)
                ops.gemm(ln3, W[f"{b}.ff1.w"], ff, M=M, N=8 * c, c1=c, ldo=ldh if fold else None, bias=W[f"{b}.ff1.b"], mode=1)
            if fold:
                out = self._empty(M, c)
                ops.gemm(buf, W[f"{n}.ffpo.w"], out, M=M, N=c, c1=5 * c, bias=W[f"{n}.ffpo.b"], res=x, ldr=c,
                         ws=self._gemm_ws, gn_hw=gn_hw)
            else:
                h = self._empty(M, c)
                ops.gemm(ff, W[f"{b}.ff2.w"], h, M=M, N=c, c1=4 * c, bias=W[f"{b}.ff2.b"], res=h3, ldr=c,
                         ws=self._gemm_ws)
        if not fold:
            out = self._empty(M, c)
            ops.gemm(h, W[f"{n}.proj_out.w"], out, M=M, N=c, c1=c, bias=W[f"{n}.proj_out.b"], res=x, ldr=c,
                     gn_hw=N if N == N_real else 0)      # (the next resnet's norm1 / a skip consumer reads it)
        if N != N_real:
            out = out.view(-1, N, c)[:, :N_real].reshape(-1, c)      # reshape of a sliced view: one copy
        return out

    def cross_attention(self, b: str, h2: torch.Tensor, B: int, N: int, c: int, heads: int, kvrow: torch.Tensor,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``h2 + attn2(LayerNorm(h2), context)`` of transformer block ``b`` on token-major ``h2`` [B * N, c]: the launch
        sequence the denoise step uses for this layer (bench.py times exactly this for the roofline block).
          * SD1.5 level 0 (C = 320, 8 heads): ONE launch of the third-generation fused kernel (csrc/xattn3.hip):
            LayerNorm folded into Wq, x read from HBM once;
          * C <= CID_XATTN_FUSED_MAX_C otherwise: one launch of the first-generation fused kernel;
          * wider levels: LayerNorm + q GEMM + two-stream attention core + out GEMM (+ bias + residual) -- a
            [tokens x C] tile does not fit in LDS next to the weight slabs there;
          * any level, more than 96 context rows: (LayerNorm +) q GEMM + long-context core (csrc/xattn_long.hip) + out GEMM.
        ``out``: a [B * N, c] column block of a wider buffer to write instead of a fresh contiguous tensor (its row stride is
        the pitch; not with the first-generation fused kernel)."""
        W, ctx = self.W, self._ctx
        M = B * N
        h3 = self._empty(M, c) if out is None else out
        ldo = None if out is None else out.stride(0)
        if ctx.v2.get(b) == LONG_CONTEXT:
            # more than 96 context rows (tested first: _fused_gen1 does not look at the context): the (LayerNorm-folded)
            # query projection, the long-context core (csrc/xattn_long.hip), the out projection (+ bias + residual)
            q2 = self._empty(M, c)
            if ops.ln_fold(M):
                ops.gemm(h2, W[f"{b}.attn2.wql"], q2, M=M, N=c, c1=c, ln=self._ln(b, "attn2.wq_ln"))
            else:
                ln2 = self._empty(M, c)
                ops.layernorm(h2, ln2, W[f"{b}.norm2.g"], W[f"{b}.norm2.b"], M=M, C_=c)
                ops.gemm(ln2, W[f"{b}.attn2.wq"], q2, M=M, N=c, c1=c)
            o2 = self._empty(M, c)
            ops.id_xattn_long(q2, o2, kp=ctx.kp[b], vp=ctx.vp[b], kvrow=kvrow, B=B, N=N, C_=c, heads=heads,
                              n_txt=ctx.n_txt, n_ip=ctx.n_ip, ip_scale=self.packed.ip_scale[b])
            ops.gemm(o2, W[f"{b}.attn2.wo"], h3, M=M, N=c, c1=c, ldo=ldo, bias=W[f"{b}.attn2.bo"], res=h2, ldr=c)
        elif ctx.v2.get(b) == 3:
            ops.id_xattn3(h2, h3, wq_p=W[f"{b}.attn2.wq_p"], q_rowsum=W[f"{b}.attn2.qs"].view(torch.float32),
                          q_bias=W[f"{b}.attn2.qb"].view(torch.float32), wo_p=W[f"{b}.attn2.wo_p"], bo=W[f"{b}.attn2.bo"],
                          kp=ctx.kp[b], vp=ctx.vp[b], kvrow=kvrow, B=B, N=N, C_=c, heads=heads, n_txt=ctx.n_txt,
                          n_ip=ctx.n_ip, ip_scale=self.packed.ip_scale[b], has_ln=True, add_residual=True, ln_eps=ops.LN_EPS,
                          ldo=ldo)
        elif self._fused_gen1(c, B * N):
            assert out is None, "cross_attention: the first-generation fused kernel writes contiguous rows"
            ops.id_xattn(h2, h3, wq=W[f"{b}.attn2.wq"], wo=W[f"{b}.attn2.wo"], bo=W[f"{b}.attn2.bo"],
                         kp=ctx.kp[b], vp=ctx.vp[b], kvrow=kvrow, B=B, N=N, C_=c, heads=heads,
                         n_txt=ctx.n_txt, n_ip=ctx.n_ip, ip_scale=self.packed.ip_scale[b], residual=h2,
                         ln_gamma=W[f"{b}.norm2.g"], ln_beta=W[f"{b}.norm2.b"], ln_eps=ops.LN_EPS)
        elif self._qattn and ops.qattn_supported(c, heads, N, ctx.n_txt, ctx.n_ip):
            # wider levels: the (LayerNorm-folded) query projection runs the attention as its epilogue (cid_gemm_f16 mode 3:
            # tiles of whole heads, Q never leaves the CU), then the out projection (+ bias + residual) -- two launches
            o2 = self._empty(M, c)
            att = (ctx.kp[b], ctx.vp[b], kvrow, ctx.n_txt, ctx.n_ip, self.packed.ip_scale[b])
            if ops.ln_fold_q(M):
                ops.gemm(h2, W[f"{b}.attn2.wql"], o2, M=M, N=c, c1=c, mode=3, heads=heads, dhead=c // heads, ntok=N,
                         ln=self._ln(b, "attn2.wq_ln"), att=att)
            else:
                ln2 = self._empty(M, c)
                ops.layernorm(h2, ln2, W[f"{b}.norm2.g"], W[f"{b}.norm2.b"], M=M, C_=c)
                ops.gemm(ln2, W[f"{b}.attn2.wq"], o2, M=M, N=c, c1=c, mode=3, heads=heads, dhead=c // heads, ntok=N, att=att)
            ops.gemm(o2, W[f"{b}.attn2.wo"], h3, M=M, N=c, c1=c, ldo=ldo, bias=W[f"{b}.attn2.bo"], res=h2, ldr=c)
        else:
            q2 = self._empty(M, c)
            if ops.ln_fold(M):     # norm2 folded into the query projection
                ops.gemm(h2, W[f"{b}.attn2.wql"], q2, M=M, N=c, c1=c, ln=self._ln(b, "attn2.wq_ln"))
            else:
                ln2 = self._empty(M, c)
                ops.layernorm(h2, ln2, W[f"{b}.norm2.g"], W[f"{b}.norm2.b"], M=M, C_=c)
                ops.gemm(ln2, W[f"{b}.attn2.wq"], q2, M=M, N=c, c1=c)
            o2 = self._empty(M, c)
            ops.id_xattn_core(q2, o2, kp=ctx.kp[b], vp=ctx.vp[b], kvrow=kvrow, B=B, N=N, C_=c, heads=heads,
                              n_txt=ctx.n_txt, n_ip=ctx.n_ip, ip_scale=self.packed.ip_scale[b])
            ops.gemm(o2, W[f"{b}.attn2.wo"], h3, M=M, N=c, c1=c, ldo=ldo, bias=W[f"{b}.attn2.bo"], res=h2, ldr=c)
        return h3

    def _fused_gen1(self, c: int, tokens: int) -> bool:
        """one launch of the first-generation fused kernel instead of LN + GEMM + core + GEMM?  Measured per level
        (tools/xattn_levels.py, profiles/r02_xattn_levels.txt): always up to CID_XATTN_FUSED_MAX_C = 320 channels; at 640
        channels only with >= 16 k tokens in flight (SDXL's 64 x 64 level at CFG batch 4: 68.5 vs 78.2 us; SD1.5's
        32 x 32 level at CFG batch 8 has 8 k: 61.8 vs 53.3 us); never at 1280 (144-149 vs 54-67 us)."""
        return fused_gen1(c, tokens, self._xattn_fused_max_c)

    def cross_attention_path(self, b: str, c: int, B: int, N: int) -> str:
        """the launch sequence :meth:`cross_attention` runs for block ``b`` on B samples of N tokens, as text (bench.py's
        roofline block, tools/xattn_levels.py) -- the same predicates on the same arguments as the method itself"""
        assert B > 0 and N > 0, "cross_attention_path: B samples of N tokens (the shape decides the launch sequence)"
        tokens = B * N
        if self._ctx.v2.get(b) == LONG_CONTEXT:
            return (f"q GEMM + id_xattn_long core<{self._ctx.n_txt},{self._ctx.n_ip}> + out GEMM (three launches)"
                    if ops.ln_fold(tokens) else
                    f"layernorm + q GEMM + id_xattn_long core<{self._ctx.n_txt},{self._ctx.n_ip}> + out GEMM (four launches)")
        if self._ctx.v2.get(b):
            gen = self._ctx.v2[b]
            return f"id_xattn{gen}_kernel<{self._ctx.n_txt},{self._ctx.n_ip}> (one launch)"
        if self._fused_gen1(c, tokens):
            return "id_xattn_kernel (one launch, first generation)"
        heads = self._heads_of(b)
        if self._qattn and ops.qattn_supported(c, heads, N, self._ctx.n_txt, self._ctx.n_ip):
            return ("q GEMM with attention epilogue + out GEMM (two launches)" if ops.ln_fold_q(tokens)
                    else "layernorm + q GEMM with attention epilogue + out GEMM (three launches)")
        return "layernorm + q GEMM + id_xattn core + out GEMM (four launches)"

    def time_embed(self, t_dev: torch.Tensor, B: int, added_cond_kwargs=None) -> torch.Tensor:
        """sinusoid -> MLP (-> + SDXL text_time embedding) -> all ResnetBlock2D.time_emb_proj
        at once.  Returns [rows, sum(Cout)] with rows = 1 (shared timestep) or B (SDXL)."""
        cfg, W = self.config, self.W
        c0, ted = cfg.block_out_channels[0], cfg.time_embed_dim
        sc = self._empty(1, c0)
        ops.sincos_embed(t_dev, sc, rows=1, dim=c0)
        self._add_guidance(sc)
        e1 = self._empty(1, ted)
        ops.linear_small(sc, W["time_embedding.linear_1.w"], W["time_embedding.linear_1.b"], e1,
                         M=1, N=ted, K=c0, act_out=1)
        emb = self._empty(1, ted)
        ops.linear_small(e1, W["time_embedding.linear_2.w"], W["time_embedding.linear_2.b"], emb, M=1, N=ted, K=ted)
        rows = 1
        if cfg.addition_embed_type == "text_time":
            text_embeds = added_cond_kwargs["text_embeds"].to(device=self.device, dtype=torch.float16).contiguous()
            time_ids = added_cond_kwargs["time_ids"].to(device=self.device, dtype=torch.float32).contiguous()
            assert text_embeds.shape[0] == B and time_ids.shape[0] == B
            ad = cfg.addition_time_embed_dim
            nid = time_ids.shape[1]
            pdim = text_embeds.shape[1] + nid * ad
            assert pdim == cfg.projection_class_embeddings_input_dim
            cat = self._empty(B, pdim)
            cat[:, :text_embeds.shape[1]].copy_(text_embeds)
            tid = self._empty(B * nid, ad)
            ops.sincos_embed(time_ids.reshape(-1), tid, rows=B * nid, dim=ad)
            cat[:, text_embeds.shape[1]:].copy_(tid.reshape(B, nid * ad))
            a1 = self._empty(B, ted)
            ops.linear_small(cat, W["add_embedding.linear_1.w"], W["add_embedding.linear_1.b"], a1,
                             M=B, N=ted, K=pdim, act_out=1)
            embB = self._empty(B, ted)
            ops.linear_small(a1, W["add_embedding.linear_2.w"], W["add_embedding.linear_2.b"], embB,
                             M=B, N=ted, K=ted, add=emb, ldadd=0)
            emb, rows = embB, B
        out = self._empty(rows, self.packed.temb_total)
        ops.linear_small(emb, W["temb_all.w"], W["temb_all.b"], out, M=rows, N=self.packed.temb_total, K=ted, act_in=1)
        return out

    @torch.no_grad()
    def time_embed_table(self, tvals: torch.Tensor, guidance_scale: Optional[float] = None) -> torch.Tensor:
        """The time path of EVERY step of a generation at once: [S] timesteps -> [S, sum(Cout)].  Without SDXL's
        text_time conditioning the per-resnet time rows depend on the timestep only, so the three GEMVs that would
        otherwise re-read 50 MB of time-projection weights in every step run once per generation; a step then takes
        its row from the table (``forward_tokens(temb=...)``).  ``guidance_scale``: required by a UNet with
        ``time_cond_proj_dim`` -- its rows are MLP(sinusoid(t) + cond_proj(guidance embedding)), see set_guidance_embedding."""
        cfg, W = self.config, self.W
        assert cfg.addition_embed_type is None
        if cfg.time_cond_proj_dim is not None:
            if guidance_scale is None:
                raise ValueError("time_embed_table: a UNet with time_cond_proj_dim needs guidance_scale")
            self.set_guidance_embedding(guidance_scale)
        c0, ted = cfg.block_out_channels[0], cfg.time_embed_dim
        tv = tvals.to(device=self.device, dtype=torch.float32).contiguous()
        S = tv.numel()
        out = self._empty(S, self.packed.temb_total)
        for lo in range(0, S, 64):                              # cid_linear_small_f16 takes up to 64 rows
            n = min(64, S - lo)
            sc, e1, emb = self._empty(n, c0), self._empty(n, ted), self._empty(n, ted)
            ops.sincos_embed(tv[lo:lo + n], sc, rows=n, dim=c0)
            self._add_guidance(sc)
            ops.linear_small(sc, W["time_embedding.linear_1.w"], W["time_embedding.linear_1.b"], e1,
                             M=n, N=ted, K=c0, act_out=1)
            ops.linear_small(e1, W["time_embedding.linear_2.w"], W["time_embedding.linear_2.b"], emb, M=n, N=ted, K=ted)
            ops.linear_small(emb, W["temb_all.w"], W["temb_all.b"], out[lo:lo + n], M=n, N=self.packed.temb_total,
                             K=ted, act_in=1)
        return out

    @torch.no_grad()
    def forward_tokens(self, sample: torch.Tensor, t_dev: torch.Tensor, kvrow: torch.Tensor, B: int,
                       added_cond_kwargs=None, down_residuals: Optional[Sequence[torch.Tensor]] = None,
                       mid_residual: Optional[torch.Tensor] = None, temb: Optional[torch.Tensor] = None,
                       in_scale: Optional[torch.Tensor] = None, extra: Optional[torch.Tensor] = None,
                       residual_scales: Optional[torch.Tensor] = None, pag_rows: int = 0, sag=None) -> torch.Tensor:
        """sample: NCHW fp16 [Bin, cin, H, W] with B % Bin == 0 (batch row b reads sample b % Bin,
        i.e. the CFG duplication of ref :537-539 costs no copy).  Returns NCHW fp16 [B, cout, H, W].
        ``residual_scales`` (DEVICE fp32, one value per net) selects the multi-ControlNet form: ``down_residuals`` and
        ``mid_residual`` are then lists with one entry per net -- that net's UNSCALED residuals (a list of skip-shaped
        tensors / the mid tensor), or None for a net that did not run and whose scale is 0 -- and two cid_residual_accum_f16
        launches add sum_k scale_k * r_k to the skip tensors and to the mid block's output, whatever the number of nets.
        ``extra`` [Bin, cin2, H, W]: the trailing input channels of a 9-channel inpainting UNet (cat([mask,
        masked_image_latents]), inpaint ref :320-321), read by conv_in beside the latents instead of a concatenated copy
        and not touched by ``in_scale``.
        ``pag_rows`` > 0 (perturbed-attention guidance): the TRAILING ``pag_rows`` batch rows are the perturbed evaluation of
        the rows in front of them -- same latents (b % Bin), same time row, whatever ``kvrow`` and ``added_cond_kwargs`` give
        them -- and the blocks ``enable_pag`` selected run identity self-attention on them.
        ``sag`` = (mass, first_row, rows) (self-attention guidance): ``mass`` fp32 [rows, hm * wm], (hm, wm) =
        ``mid_size(H, W)``, receives the column mass of the attention map of ``mid_block.attentions[0].transformer_blocks[0]
        .attn1`` for batch rows [first_row, first_row + rows) -- one more launch beside that layer's attention; None launches
        what is launched without it."""
        cfg, W = self.config, self.W
        if sag is not None:
            mass, first, rows = sag
            if pag_rows:
                raise NotImplementedError("self-attention guidance together with perturbed rows is not built")
            if not (0 <= first and rows > 0 and first + rows <= B):
                raise ValueError(f"forward_tokens: sag rows [{first}, {first + rows}) of B = {B} batch rows")
            hm, wm = self.mid_size(sample.shape[2], sample.shape[3])
            if mass.dtype != torch.float32 or tuple(mass.shape) != (rows, hm * wm) or not mass.is_contiguous():
                raise ValueError(f"forward_tokens: sag mass {tuple(mass.shape)} {mass.dtype}; contiguous fp32 {(rows, hm * wm)}")
        if pag_rows:
            if not 0 < pag_rows <= B:
                raise ValueError(f"forward_tokens: pag_rows = {pag_rows} of B = {B} batch rows")
            if not self._pag:
                raise RuntimeError("forward_tokens(pag_rows=): no layer is selected; call enable_pag(layers) first")
            if down_residuals is not None or mid_residual is not None:
                raise NotImplementedError("PAG with ControlNet residuals is not built")
        Bin, cin, H, Wd = sample.shape
        if extra is not None:
            cin += extra.shape[1]
        assert B % Bin == 0 and cin == cfg.in_channels, (B, Bin, cin, cfg.in_channels)
        if temb is None:
            temb = self.time_embed(t_dev, B, added_cond_kwargs)
        trows = temb.shape[0]
        c0 = cfg.block_out_channels[0]
        # CFG batches arrive as B = rep * Bin with batch row b reading latent b % Bin: until the first cross-attention the
        # rep copies are the same computation on the same data (same latents, same timestep row), so conv_in, the first
        # ResnetBlock2D and the first transformer's GroupNorm / proj_in / self-attention run on the Bin distinct samples
        # only and are repeated where the halves start to differ (their encoder_hidden_states).  Row-for-row the same
        # tensors as the full batch; CID_CFG_DEDUP=0 disables it.
        Bp = B
        if (self._cfg_dedup and B > Bin and trows == 1 and self.downs and self.downs[0].attentions
                and self.downs[0].attentions[0].n_layers >= 1):
            Bp = Bin
        # ... unless PAG perturbs that first self-attention: the perturbed rows then differ from the others inside it
        if pag_rows and Bp != B and f"{self.downs[0].attentions[0].name}.transformer_blocks.0" in self._pag:
            Bp = B
        # (conv_in reads latent b % Bin for batch row b: run on all B rows it writes the duplicated skip tensor itself, and the
        #  first Bp samples of that buffer are the deduplicated stream)
        xfull = self._empty(B * H * Wd, c0)
        ops.conv_in(sample, xfull, W["conv_in.w"], W["conv_in.b"], B=B, Bin=Bin, cin=cin, H=H, W=Wd, cout=c0, in_scale=in_scale,
                    extra=extra)
        x = xfull[:Bp * H * Wd]
        skips = [(xfull, c0, H, Wd)]
        c = c0
        for bi, blk in enumerate(self.downs):
            for j, r in enumerate(blk.resnets):
                first = Bp != B and bi == 0 and j == 0
                x = self._resnet(r, x, None, c, 0, Bp if first else B, H, Wd, temb, trows, rep=2 if first and B == 2 * Bp else 1)
                c = r.cout
                if blk.attentions:
                    x = self._transformer(blk.attentions[j], x, B, H, Wd, kvrow, Bp=Bp if first else None, pag_rows=pag_rows)
                skips.append((x, c, H, Wd))
            if blk.sampler:
                n = f"{blk.name}.{blk.sampler}.conv"
                Ho, Wo = H // 2, Wd // 2
                y = self._empty(B * Ho * Wo, c)
                ops.gemm(x, W[f"{n}.w"], y, M=B * Ho * Wo, N=c, c1=c, bias=W[f"{n}.b"], taps=9,
                         Hi=H, Wi=Wd, Ho=Ho, Wo=Wo, stride=2, ws=self._gemm_ws, gn_hw=Ho * Wo)
                x, H, Wd = y, Ho, Wo
                skips.append((x, c, H, Wd))
        multi = residual_scales is not None
        if multi:
            # the same two exceptions as below get a copy; then ONE launch over all skip tensors
            ran = [d for d in down_residuals if d is not None]
            assert ran and all(len(d) == len(skips) for d in ran) and len(mid_residual) == len(down_residuals)
            new, seen = [], set()
            for (s, sc_, sh, sw) in skips:
                if s is x or s.data_ptr() in seen:
                    s = s.clone()
                seen.add(s.data_ptr())
                new.append((s, sc_, sh, sw))
            skips = new
            ops.residual_accum([s for s, _, _, _ in skips], down_residuals, residual_scales)
        elif down_residuals is not None:
            # ControlNet residuals (CN :418-425), given token-major [B or B/2, HW, C]
            assert len(down_residuals) == len(skips)
            # The down path is complete: every skip tensor has been read by whatever followed it there, the up blocks are the
            # only readers left -- the residual is added IN PLACE.  Two exceptions get a copy: the last skip is also the
            # mid block's input (which takes no down residual, CN :418-425 add to the skip list only), and a tensor that
            # sits in the list twice (none today) must not be added to twice.
            new, seen = [], set()
            for (s, sc_, sh, sw), r in zip(skips, down_residuals):
                if s is x or s.data_ptr() in seen:
                    s = s.clone()
                seen.add(s.data_ptr())
                ops.add_inplace(s, r.to(device=self.device, dtype=torch.float16).contiguous())
                new.append((s, sc_, sh, sw))
            skips = new
        x = self._resnet(self.mid.resnets[0], x, None, c, 0, B, H, Wd, temb, trows)
        x = self._transformer(self.mid.attentions[0], x, B, H, Wd, kvrow, pag_rows=pag_rows, sag=sag)
        x = self._resnet(self.mid.resnets[1], x, None, c, 0, B, H, Wd, temb, trows)
        if multi:
            ops.residual_accum([x], [None if m is None else [m] for m in mid_residual], residual_scales)
        elif mid_residual is not None:     # (x is the mid block's own output here: nobody else holds it)
            ops.add_inplace(x, mid_residual.to(device=self.device, dtype=torch.float16).contiguous())
        for bi, blk in enumerate(self.ups):
            for j, r in enumerate(blk.resnets):
                s, sc_, sh, sw = skips.pop()
                assert (sh, sw) == (H, Wd)
                if self._freeu is not None and bi < 2:
                    # FreeU, IN PLACE on both: a skip tensor is read exactly once on the up path -- by this resnet -- and the
                    # down path, the mid block and the residual adds above are done with it (the two exceptions there got
                    # their copies); x is the previous block's own output, which nobody else holds.
                    ops.freeu(x, s, self._ws(B), B=B, H=H, W=Wd, c_x=c, c_skip=sc_, s=self._freeu[bi], b=self._freeu[2 + bi])
                x = self._resnet(r, x, s, c, sc_, B, H, Wd, temb, trows)
                c = r.cout
                if blk.attentions:
                    x = self._transformer(blk.attentions[j], x, B, H, Wd, kvrow, pag_rows=pag_rows)
            if blk.sampler:
                n = f"{blk.name}.{blk.sampler}.conv"
                Ho, Wo = H * 2, Wd * 2
                y = self._empty(B * Ho * Wo, c)
                ops.gemm(x, W[f"{n}.w"], y, M=B * Ho * Wo, N=c, c1=c, bias=W[f"{n}.b"], taps=9,
                         Hi=H, Wi=Wd, Ho=Ho, Wo=Wo, stride=1, up=1, ws=self._gemm_ws, gn_hw=Ho * Wo, w_up4=W.get(f"{n}.w4"))
                x, H, Wd = y, Ho, Wo
        g = self._gn(x, c, B, H * Wd, W["conv_norm_out.g"], W["conv_norm_out.b"], cfg.norm_eps, True)
        out = self._empty(B, cfg.out_channels, H, Wd)
        ops.conv_out(g, out, W["conv_out.w"], W["conv_out.b"], B=B, H=H, W=Wd, cin=c, cout=cfg.out_channels)
        return out

    # ------------------------------------------------------------------ diffusers-style call
    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states=None, cross_attention_kwargs=None,
                 added_cond_kwargs=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, return_dict=True):
        sample = sample.to(device=self.device, dtype=torch.float16).contiguous()
        B = sample.shape[0]
        self.refresh_context(encoder_hidden_states)
        kvrow = torch.arange(B, dtype=torch.int32, device=self.device)
        self._t_buf.fill_(float(timestep))

        def tok(r):  # NCHW -> token-major
            r = r.to(device=self.device, dtype=torch.float16)
            return r.permute(0, 2, 3, 1).reshape(r.shape[0], -1, r.shape[1]).contiguous()

        dres = [tok(r) for r in down_block_additional_residuals] if down_block_additional_residuals is not None else None
        mres = tok(mid_block_additional_residual) if mid_block_additional_residual is not None else None
        out = self.forward_tokens(sample, self._t_buf, kvrow, B, added_cond_kwargs, dres, mres)
        return UNetOutput(sample=out) if return_dict else (out,)
