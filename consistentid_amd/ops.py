"""Thin torch-tensor front end of the C ABI (include/cid.h).  PyTorch is used for
device memory and the current HIP stream only; every op below is one (or a fixed few)
hand-written HIP kernel launch in libcid.so.  Nothing here computes on the CPU."""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Optional

import torch

from . import _lib
from ._lib import GemmDesc, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _req(t: torch.Tensor, name: str, dtype=torch.float16):
    if not t.is_cuda:
        raise _lib.CidError(f"{name}: tensor must live on the GPU (got {t.device}); libcid has no CPU path")
    if t.dtype != dtype:
        raise _lib.CidError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.data_ptr() % 16:
        raise _lib.CidError(f"{name}: base pointer must be 16-byte aligned")


def dvp_of(d: int) -> int:
    """rows reserved per head in the transposed-V buffer (head dim rounded up to 32)."""
    return (d + 31) // 32 * 32


# --------------------------------------------------------------------------- GEMM / conv
_DUMMY = 64      # a 16-byte-aligned stand-in address for gemm_plan (the planner tests pointers for NULL and alignment only)


def _addr(t, name: str, dtype=torch.float16, check_tensor: bool = True) -> Optional[int]:
    """device address of an operand: a tensor (checked), None, or -- for :func:`gemm_plan` -- True / an integer address"""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        if check_tensor:
            _req(t, name, dtype)
        return t.data_ptr()
    return _DUMMY if t is True else int(t)


def _gemm_desc(x1, w, out, *, M: int, N: int, c1: int, ld1: Optional[int] = None,
               x2=None, c2: int = 0, ld2: Optional[int] = None, ldo: Optional[int] = None,
               bias=None, rowbias=None, ld_rowbias: int = 0,
               rows_per_sample: int = 1, res=None, ldr: Optional[int] = None,
               taps: int = 1, Hi: int = 0, Wi: int = 0, Ho: int = 0, Wo: int = 0, stride: int = 1, up: int = 0,
               mode: int = 0, vt=None, n_vt0: int = 0, heads: int = 0, dhead: int = 0,
               ntok: int = 0, ws=None, ln=None, att=None,
               out2=None, pad_mode: int = 0, act: int = 0, w_up4=None, ws_bytes: Optional[int] = None,
               check_tensors: bool = True) -> GemmDesc:
    """The cid_gemm_desc of a :func:`gemm` / :func:`gemm_plan` call (everything but gn_stats, which the caller attaches)."""
    a = lambda t, name, dtype=torch.float16: _addr(t, f"gemm.{name}", dtype, check_tensors)
    d = GemmDesc()
    d.x1, d.w, d.out = a(x1, "x1"), a(w, "w"), a(out, "out")
    d.x2, d.bias, d.rowbias, d.res = a(x2, "x2"), a(bias, "bias"), a(rowbias, "rowbias"), a(res, "res")
    d.vt, d.out2, d.w_up4 = a(vt, "vt"), a(out2, "out2"), a(w_up4, "w_up4")
    d.c1, d.c2 = c1, c2
    d.ld1 = ld1 if ld1 is not None else c1
    d.ld2 = ld2 if ld2 is not None else c2
    n_out = N // 2 if mode == 1 else (n_vt0 if mode == 2 else N)
    d.ldo = ldo if ldo is not None else n_out
    d.ld_rowbias, d.rows_per_sample = ld_rowbias, rows_per_sample
    d.ldr = ldr if ldr is not None else N
    d.M, d.N, d.taps = M, N, taps
    d.Hi, d.Wi, d.Ho, d.Wo, d.stride, d.up = Hi, Wi, Ho, Wo, stride, up
    d.pad_mode = pad_mode
    d.act = act
    d.mode = mode
    d.n_vt0, d.heads, d.dhead, d.dvp, d.ntok = n_vt0, heads, dhead, dvp_of(dhead) if dhead else 0, ntok
    if ws is not None:
        if isinstance(ws, torch.Tensor):
            d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
        else:
            d.ws, d.ws_bytes = _DUMMY, int(ws_bytes or 0)
    if att is not None:
        kp, vp, kvrow, n_txt, n_ip, ip_scale = (True, True, True, 77, 4, 1.0) if att is True else att
        d.att_kp, d.att_vp, d.att_kvrow = a(kp, "att_kp"), a(vp, "att_vp"), a(kvrow, "att_kvrow", torch.int32)
        d.att_n_txt, d.att_n_ip, d.att_ip_scale = int(n_txt), int(n_ip), float(ip_scale)
    if ln is not None:
        ls, lb, eps = (True, True, LN_EPS) if ln is True else ln
        d.ln_s, d.ln_b, d.ln_eps = a(ls, "ln_s", torch.float32), a(lb, "ln_b", torch.float32), float(eps)
    return d


def _stats_rows(rows: int, gn_hw: int, act: int) -> int:
    """tile height of the GroupNorm statistics :func:`gemm` attaches for a consumer over ``gn_hw`` tokens per sample (0 = none)"""
    if gn_hw > GN_SMALL_MAX_HW and GN_EPILOGUE_STATS and not act and rows > 0 and gn_hw % rows == 0:
        return rows                # (smaller samples: cid_groupnorm_f16 is one launch anyway)
    return 0


def gemm(x1: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, M: int, N: int, c1: int, ld1: Optional[int] = None,
         x2: Optional[torch.Tensor] = None, c2: int = 0, ld2: Optional[int] = None, ldo: Optional[int] = None,
         bias: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None, ld_rowbias: int = 0,
         rows_per_sample: int = 1, res: Optional[torch.Tensor] = None, ldr: Optional[int] = None,
         taps: int = 1, Hi: int = 0, Wi: int = 0, Ho: int = 0, Wo: int = 0, stride: int = 1, up: int = 0,
         mode: int = 0, vt: Optional[torch.Tensor] = None, n_vt0: int = 0, heads: int = 0, dhead: int = 0,
         ntok: int = 0, ws: Optional[torch.Tensor] = None, ln=None, gn_hw: int = 0, att=None,
         out2: Optional[torch.Tensor] = None, pad_mode: int = 0, act: int = 0, w_up4: Optional[torch.Tensor] = None):
    """``att`` = (kp, vp, kvrow, n_txt, n_ip, ip_scale) with ``mode=3``: the query projection of the identity cross-attention
    with the two-stream attention as its epilogue (``heads``, ``dhead``, ``ntok`` describe the heads and the tokens per sample).
    ``ln`` = (s, b, eps): LayerNorm folded into the projection -- ``x1`` is the raw residual stream, ``w`` carries gamma,
    s / b are the fp32 [N] fold vectors (weights.fold_ln); no ``bias`` then (it is inside b).
    ``gn_hw`` > 0: the consumer of ``out`` is a GroupNorm over samples of ``gn_hw`` tokens -- if this launch can emit the
    statistics from its epilogue they are attached as ``out._gn_stats = (fp32 [M / rows, 32, 2], rows)`` for
    ``groupnorm`` to pick up (saves its statistics pass).
    ``out2``: a second destination for the same rows (same pitch as ``out``; mode 0): the CFG duplication of a tensor both
    halves of the batch share, written by the producer.
    ``pad_mode=1``: Downsample2D(padding=0) -- pad (0, 1, 0, 1), then the stride-2 3x3 conv without padding.
    ``act=1``: ReLU after bias / rowbias / res (mode 0; not with ``ws``, ``ln`` or ``gn_hw``).
    ``w_up4``: the folded weights of an Upsample2D convolution (:func:`upconv_fold` of ``w``; ``taps=9, up=1``): the launch
    runs as four 2x2 phase convolutions at input resolution where the library can tile it so, from ``w`` otherwise."""
    lib = _lib.load()
    for name, t in (("x1", x1), ("w", w), ("out", out)):
        if not isinstance(t, torch.Tensor):
            raise _lib.CidError(f"gemm.{name}: a tensor is required (addresses are for gemm_plan)")
    d = _gemm_desc(x1, w, out, M=M, N=N, c1=c1, ld1=ld1, x2=x2, c2=c2, ld2=ld2, ldo=ldo, bias=bias, rowbias=rowbias,
                   ld_rowbias=ld_rowbias, rows_per_sample=rows_per_sample, res=res, ldr=ldr, taps=taps, Hi=Hi, Wi=Wi, Ho=Ho,
                   Wo=Wo, stride=stride, up=up, mode=mode, vt=vt, n_vt0=n_vt0, heads=heads, dhead=dhead, ntok=ntok, ws=ws,
                   ln=ln, att=att, out2=out2, pad_mode=pad_mode, act=act, w_up4=w_up4)
    stats = None
    rows = 0
    if gn_hw > GN_SMALL_MAX_HW:
        rows = _stats_rows(int(lib.cid_gemm_stats_rows(C.byref(d))), gn_hw, act)
        if rows > 0:
            stats = torch.empty(M // rows, 32, 2, dtype=torch.float32, device=out.device)
            d.gn_stats = stats.data_ptr()
    check(lib.cid_gemm_f16(C.byref(d), _stream()), "cid_gemm_f16")
    if stats is not None:
        out._gn_stats = (stats, rows)
    elif hasattr(out, "_gn_stats"):
        del out._gn_stats            # a reused output tensor must not carry the statistics of what it held before
    return out


def gemm_plan(x1=True, w=True, out=True, **kw) -> dict:
    """What :func:`gemm` with the same keywords would launch (cid_gemm_plan: host code, no launch, no GPU needed): ``family``
    (one of ``_lib.GEMM_FAMILIES``), tile ``bm`` x ``bn``, ``splitk``, ``nloop``, ``nbuf``, the ``ln`` / ``act`` / ``vmode``
    instance flags, ``splitk_epilogue``, ``stats_rows`` (tile height if the launch can emit GroupNorm statistics, else 0) and
    ``stats`` (whether :func:`gemm` would attach them for this ``gn_hw``).  Every operand may be a tensor, ``True`` (present,
    at a dummy 16-byte-aligned address) or None; ``ws=True`` takes its size from ``ws_bytes``, ``ln=True`` / ``att=True``
    stand for present operands with the usual constants.  Raises CidError where :func:`gemm` would."""
    lib = _lib.load()
    gn_hw = kw.pop("gn_hw", 0)
    d = _gemm_desc(x1, w, out, check_tensors=False, **kw)
    info = _lib.GemmPlanInfo()
    check(lib.cid_gemm_plan(C.byref(d), C.byref(info)), "cid_gemm_plan")
    plan = {n: int(getattr(info, n)) for n, _ in info._fields_}
    plan["family"] = _lib.GEMM_FAMILIES[plan["family"]]
    plan["stats"] = int(_stats_rows(plan["stats_rows"], gn_hw, d.act) > 0)
    return plan


def upconv_fold(w: torch.Tensor) -> torch.Tensor:
    """Packed nine-tap weights ``[N, 9 * C]`` of an Upsample2D convolution (``weights._conv3``) -> the folded
    ``[4 parities * N, 4 taps * C]`` tensor for ``gemm(..., w_up4=)`` (cid_upconv_fold_f16; once per weight load)."""
    _req(w, "upconv_fold.w")
    N, C_ = w.shape[0], w.shape[1] // 9
    if w.dim() != 2 or w.shape[1] != 9 * C_ or not w.is_contiguous():
        raise _lib.CidError(f"upconv_fold: expected contiguous [N, 9 * C] weights, got {tuple(w.shape)}")
    w4 = torch.empty(4 * N, 4 * C_, dtype=torch.float16, device=w.device)
    check(_lib.load().cid_upconv_fold_f16(_p(w), _p(w4), N, C_, _stream()), "cid_upconv_fold_f16")
    return w4


LN_EPS = 1e-5        # diffusers BasicTransformerBlock LayerNorms: shared by layernorm(), the folded projections and the fused kernels

def qattn_supported(C_: int, heads: int, N: int, n_txt: int, n_ip: int) -> bool:
    """can ``gemm(mode=3)`` (query projection + attention epilogue) serve this cross-attention level?"""
    if heads <= 0 or C_ % heads:
        return False
    d = C_ // heads
    return (d in (64, 80, 160) and n_txt == 77 and n_ip == 4 and N % 64 == 0 and (d != 64 or (C_ % 128 == 0 and N % 128 == 0))
            and C_ % (128 if d == 64 else 160) == 0)


# A/B switches (environment): the GEMM epilogues emit GroupNorm statistics / LayerNorm is folded into the projections
GN_EPILOGUE_STATS = os.environ.get("CID_GN_EPILOGUE_STATS", "1") != "0"
# LayerNorm fold: "auto" (default) folds where it measured faster than layernorm + GEMM -- up to 2048 tokens per launch (the
# in-loop row statistics cost the GEMMs of the larger levels more than the LayerNorm kernel they replace:
# profiles/r03_kbench.txt; SDXL folded everywhere 1.52 images/s, with this rule 1.59 -- profiles/r03_bench_sdxl_*.json);
# "1" always, "0" never
_LN_FOLD_MODE = os.environ.get("CID_LN_FOLD", "auto")


def ln_fold(M: int) -> bool:
    return _LN_FOLD_MODE == "1" or (_LN_FOLD_MODE == "auto" and M <= 2048)


_GEGLU_FOLD_MAX = int(os.environ.get("CID_GEGLU_FOLD_MAX", "8192"))      # A/B switch (2048 = the rule of rounds 3-5)


@functools.lru_cache(maxsize=None)
def _geglu_on_h32(M: int, C_: int) -> bool:
    """does the unfolded GEGLU projection of ``M`` tokens x ``C_`` channels run on csrc/linear_h32.hip?  (the planner's answer)"""
    return gemm_plan(M=M, N=8 * C_, c1=C_, mode=1, bias=True)["family"] == "geglu_h32"


def ln_fold_geglu(M: int, C_: int) -> bool:
    """norm3 folded into the GEGLU projection?  Like :func:`ln_fold`, except where the launch runs on csrc/linear_h32.hip
    (the planner's route_linear_h32, asked through :func:`gemm_plan`), which takes a plain LayerNorm-ed input: layernorm + that
    kernel measured 8 + 64 us against 84 us for the folded 16 x 16 x 32 form at SD1.5's 16 x 16 level (profiles/r06_kbench.txt)"""
    if _LN_FOLD_MODE != "auto":
        return ln_fold(M)
    # (the GEGLU launch takes its row statistics during the first n-tile only: folded it stays ahead of layernorm + GEMM up to
    #  8192 tokens -- 69.7 vs 8.0 + 65.0 us at SD1.5's 32 x 32 level, profiles/r06_kbench.txt; 86.0 vs 10.2 + 73.9 at 64 x 64)
    return M <= _GEGLU_FOLD_MAX and not _geglu_on_h32(M, C_)


# ff2 + proj_out of a transformer's tail as ONE GEMM over the row [ff | h3] (weights [Wp W2 | Wp]): "auto"
# (default) folds where the folded launch plans to the kernel family, tile, ring depth and split / unsplit class of the ff2
# launch it replaces -- the launch variants the models reach then stay the ones tests/golden/gemm_calls.json lists; "0" never;
# "1" wherever the library accepts the launch (tests at tiny shapes)
_FF2_FOLD_MODE = os.environ.get("CID_FF2_FOLD", "auto")
GEMM_WS_BYTES = 64 << 20     # the engine's split-K workspace (HipUNet._gemm_ws allocates this): part of what the planner decides on


@functools.lru_cache(maxsize=None)
def ff2_fold(M: int, C_: int, gn_hw: int = 0) -> bool:
    """does the tail of a transformer with ``C_`` channels on ``M`` tokens run as one GEMM?  (``gn_hw``: what proj_out passes)"""
    if _FF2_FOLD_MODE == "0":
        return False
    try:
        folded = gemm_plan(M=M, N=C_, c1=5 * C_, bias=True, res=True, ldr=C_, ws=True, ws_bytes=GEMM_WS_BYTES, gn_hw=gn_hw)
    except _lib.CidError:
        return False
    if _FF2_FOLD_MODE == "1":
        return True
    ff2 = gemm_plan(M=M, N=C_, c1=4 * C_, bias=True, res=True, ldr=C_, ws=True, ws_bytes=GEMM_WS_BYTES)
    same = lambda p: (p["family"], p["bm"], p["bn"], p["nbuf"], p["splitk"] > 1)
    return same(folded) == same(ff2)


# the query projection of the cross-attention with the attention epilogue (gemm mode 3): folded up to 8192 tokens per launch
# (SD1.5's 32 x 32 level at CFG batch 8: 43.1 -> 39.9 us with norm2 folded; SDXL's 4096-token level 58.4 vs 57.9; A/B switch)
_QATTN_FOLD_MAX = int(os.environ.get("CID_QATTN_LNFOLD_MAX", "8192"))


def ln_fold_q(M: int) -> bool:
    return _LN_FOLD_MODE == "1" or (_LN_FOLD_MODE == "auto" and M <= _QATTN_FOLD_MAX)


# --------------------------------------------------------------------------- attention
def self_attn(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, *, B: int, N: int,
              heads: int, d: int, ldq: int, ldk: int, ldo: int, n_keys: Optional[int] = None):
    """``n_keys``: only the first n_keys tokens of every sample are real keys (padding beyond)"""
    lib = _lib.load()
    for name, t in (("q", q), ("k", k), ("vt", vt), ("out", out)):
        _req(t, f"self_attn.{name}")
    if n_keys is not None and n_keys != N:
        check(lib.cid_self_attn_keys_f16(_p(q), _p(k), _p(vt), _p(out), B, N, heads, d, ldq, ldk, dvp_of(d), ldo, n_keys,
                                         _stream()), "cid_self_attn_keys_f16")
        return out
    check(lib.cid_self_attn_f16(_p(q), _p(k), _p(vt), _p(out), B, N, heads, d, ldq, ldk, dvp_of(d), ldo, _stream()),
          "cid_self_attn_f16")
    return out


def attn_colmass(q: torch.Tensor, k: torch.Tensor, mass: torch.Tensor, *, B: int, N: int, heads: int, d: int, ldq: int,
                 ldk: int, n_keys: Optional[int] = None):
    """column mass of the self-attention map of ``B`` samples (cid_attn_colmass_f16; self-attention guidance):
    ``mass`` fp32 [B, N] = mean over heads of the column sums of softmax(q k^T); ``q`` / ``k`` as ``self_attn`` takes them.
    Columns >= ``n_keys`` are written as 0, rows >= ``n_keys`` do not contribute.  Deterministic."""
    lib = _lib.load()
    _req(q, "attn_colmass.q")
    _req(k, "attn_colmass.k")
    _req(mass, "attn_colmass.mass", torch.float32)
    if mass.numel() != B * N or not mass.is_contiguous():
        raise _lib.CidError(f"attn_colmass.mass: {mass.numel()} elements; B * N = {B * N}, contiguous")
    for name, t, ld in (("q", q, ldq), ("k", k, ldk)):      # (slices of one buffer: what lies behind the pointer counts)
        have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if have < (B * N - 1) * ld + heads * d:
            raise _lib.CidError(f"attn_colmass.{name}: {have} elements behind the pointer; B * N = {B * N} rows at pitch {ld} "
                                f"need {(B * N - 1) * ld + heads * d}")
    check(lib.cid_attn_colmass_f16(_p(q), ldq, _p(k), ldk, _p(mass), B, N, N if n_keys is None else n_keys, heads, d,
                                   _stream()), "cid_attn_colmass_f16")
    return mass


def sag_degrade(latents: torch.Tensor, eps_g: torch.Tensor, mass: torch.Tensor, out: torch.Tensor, coef: torch.Tensor, *,
                hm: int, wm: int):
    """the degraded latents of self-attention guidance (cid_sag_degrade_f16): ``latents`` / ``eps_g`` / ``out`` fp16
    [B, C, h, w], ``mass`` fp32 [B, hm * wm] (``attn_colmass``), ``coef`` eight fp32 words on the device
    (``scheduler.sag_coefficient_table``): out = n_d (mass > 1 ? blur(x0) : x0) + n_e ehat"""
    lib = _lib.load()
    if latents.dim() != 4:
        raise _lib.CidError(f"sag_degrade.latents: shape {tuple(latents.shape)}; [B, C, h, w]")
    B, C_, h, w = latents.shape
    for name, t in (("latents", latents), ("eps_g", eps_g), ("out", out)):
        _req(t, f"sag_degrade.{name}")
        if tuple(t.shape) != (B, C_, h, w) or not t.is_contiguous():
            raise _lib.CidError(f"sag_degrade.{name}: shape {tuple(t.shape)}; contiguous {(B, C_, h, w)}")
    _req(mass, "sag_degrade.mass", torch.float32)
    _req(coef, "sag_degrade.coef", torch.float32)
    if mass.numel() != B * hm * wm or not mass.is_contiguous() or coef.numel() < 8:
        raise _lib.CidError(f"sag_degrade: mass / coef hold {mass.numel()} / {coef.numel()} elements; B * hm * wm = "
                            f"{B * hm * wm} (contiguous) / at least 8")
    check(lib.cid_sag_degrade_f16(_p(latents), _p(eps_g), _p(mass), _p(out), _p(coef), B, C_, h, w, hm, wm, _stream()),
          "cid_sag_degrade_f16")
    return out


def self_attn_causal(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, *, B: int, N: int,
                     heads: int, d: int, ldq: int, ldk: int, ldo: int, n_keys: int):
    """causal self-attention of the CLIP text towers: key j is visible to query i iff j <= i and j < n_keys (d = 64)"""
    lib = _lib.load()
    for name, t in (("q", q), ("k", k), ("vt", vt), ("out", out)):
        _req(t, f"self_attn_causal.{name}")
    check(lib.cid_self_attn_causal_f16(_p(q), _p(k), _p(vt), _p(out), B, N, heads, d, ldq, ldk, dvp_of(d), ldo, n_keys,
                                       _stream()), "cid_self_attn_causal_f16")
    return out


def kv_pack_elems(C_: int, heads: int):
    lib = _lib.load()
    return int(lib.cid_kv_pack_elems(C_, heads, 0)), int(lib.cid_kv_pack_elems(C_, heads, 1))


def kv_pack(kv_txt: torch.Tensor, kv_ip: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, *, R: int, C_: int,
            heads: int, n_txt: int, n_ip: int):
    lib = _lib.load()
    for name, t in (("kv_txt", kv_txt), ("kv_ip", kv_ip), ("kp", kp), ("vp", vp)):
        _req(t, f"kv_pack.{name}")
    check(lib.cid_kv_pack_f16(_p(kv_txt), _p(kv_ip), _p(kp), _p(vp), R, C_, heads, n_txt, n_ip, _stream()),
          "cid_kv_pack_f16")


def pack_wfrag(w: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _req(w, "pack_wfrag.w")
    rows, K = w.shape
    out = torch.empty_like(w)
    check(lib.cid_pack_wfrag_f16(_p(w.contiguous()), _p(out), rows, K, _stream()), "cid_pack_wfrag_f16")
    return out


def id_xattn(x: torch.Tensor, out: torch.Tensor, *, wq: torch.Tensor, wo: torch.Tensor, bo: Optional[torch.Tensor],
             kp: torch.Tensor, vp: torch.Tensor, kvrow: torch.Tensor, B: int, N: int, C_: int, heads: int,
             n_txt: int, n_ip: int, ip_scale: float, residual: Optional[torch.Tensor] = None,
             ln_gamma: Optional[torch.Tensor] = None, ln_beta: Optional[torch.Tensor] = None, ln_eps: float = 1e-5):
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("wq", wq), ("wo", wo), ("kp", kp), ("vp", vp)):
        _req(t, f"id_xattn.{name}")
    for name, t in (("bo", bo), ("residual", residual), ("ln_gamma", ln_gamma), ("ln_beta", ln_beta)):
        if t is not None:
            _req(t, f"id_xattn.{name}")
    _req(kvrow, "id_xattn.kvrow", torch.int32)
    check(lib.cid_id_xattn_f16(_p(x), _p(out), _p(residual), _p(ln_gamma), _p(ln_beta), ln_eps, _p(wq), _p(wo),
                               _p(bo), _p(kp), _p(vp), _p(kvrow), B, N, C_, heads, n_txt, n_ip, float(ip_scale),
                               _stream()), "cid_id_xattn_f16")
    return out


def xattn_long_max_txt() -> int:
    """most text rows the long-context kernel takes (CID_XATTN_LONG_MAX_TXT of the built library)"""
    return int(_lib.load().cid_xattn_long_max_txt())


XATTN_LONG_MAX_IP = 32      # CID_XATTN_LONG_MAX_IP (include/cid.h): the ID keys fill one key tile at the most
XATTN_SHORT_MAX = 96        # key slots of the register-resident kernels (csrc/xattn_core.h); longer contexts run csrc/xattn_long.hip


def kv_pack_long_elems(C_: int, heads: int, n_txt: int, n_ip: int):
    lib = _lib.load()
    ke, ve = (int(lib.cid_kv_pack_long_elems(C_, heads, n_txt, n_ip, w)) for w in (0, 1))
    if ke < 0 or ve < 0:
        raise ValueError(f"kv_pack_long_elems: no long-context layout for C={C_} heads={heads} n_txt={n_txt} n_ip={n_ip} "
                         f"(1..{xattn_long_max_txt()} text rows, {XATTN_LONG_MAX_IP} more without ID rows; "
                         f"0..{XATTN_LONG_MAX_IP} ID rows)")
    return ke, ve


def kv_pack_long(kv_txt: torch.Tensor, kv_ip: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, *, R: int, C_: int,
                 heads: int, n_txt: int, n_ip: int):
    """projected [K | V] rows ([R, L, 2C], text and ID projections) -> the operands of cid_id_xattn_long_f16 (include/cid.h):
    key tiles of 32 slots, the ID keys on a tile of their own behind the last text tile"""
    lib = _lib.load()
    for name, t in (("kv_txt", kv_txt), ("kv_ip", kv_ip), ("kp", kp), ("vp", vp)):
        _req(t, f"kv_pack_long.{name}")
    check(lib.cid_kv_pack_long_f16(_p(kv_txt), _p(kv_ip), _p(kp), _p(vp), R, C_, heads, n_txt, n_ip, _stream()),
          "cid_kv_pack_long_f16")


def id_xattn_long(q: torch.Tensor, out: torch.Tensor, *, kp: torch.Tensor, vp: torch.Tensor, kvrow: torch.Tensor,
                  B: int, N: int, C_: int, heads: int, n_txt: int, n_ip: int, ip_scale: float):
    """two-stream attention core over a long context (kv_pack_long operands); q [B * N, C_] projected and pre-scaled"""
    lib = _lib.load()
    for name, t in (("q", q), ("out", out), ("kp", kp), ("vp", vp)):
        _req(t, f"id_xattn_long.{name}")
    _req(kvrow, "id_xattn_long.kvrow", torch.int32)
    check(lib.cid_id_xattn_long_f16(_p(q), _p(out), _p(kp), _p(vp), _p(kvrow), B, N, C_, heads, n_txt, n_ip,
                                    float(ip_scale), _stream()), "cid_id_xattn_long_f16")
    return out


def kv_pack2_elems(C_: int, heads: int):
    lib = _lib.load()
    return int(lib.cid_kv_pack2_elems(C_, heads, 0)), int(lib.cid_kv_pack2_elems(C_, heads, 1))


_KV_IDX_CACHE = {}


def kv_pack2(kv_txt: torch.Tensor, kv_ip: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, *, R: int, L: int, C_: int,
             heads: int, n_txt: int, n_ip: int, order: str):
    """projected [K | V] rows of R context rows ([R, L, 2C], text and ID projections) -> the fragment-ordered
    operands of cid_id_xattn3_f16 (order "reg": register-major keys, xattn_pack.slot_key; order "slot" is the
    key order of the retired second generation, kept for the layout tests); index tables from xattn_pack, cached on the device"""
    from . import xattn_pack
    lib = _lib.load()
    for name, t in (("kv_txt", kv_txt), ("kv_ip", kv_ip), ("kp", kp), ("vp", vp)):
        _req(t, f"kv_pack2.{name}")
    key = (C_, heads, n_txt, n_ip, order, kv_txt.device)
    if key not in _KV_IDX_CACHE:
        ki, vi = xattn_pack.kv_index_tables(C_, heads, n_txt, n_ip, order)
        _KV_IDX_CACHE[key] = (torch.from_numpy(ki).to(kv_txt.device), torch.from_numpy(vi).to(kv_txt.device))
    ki, vi = _KV_IDX_CACHE[key]
    assert L == n_txt + n_ip
    for idx, dst in ((ki, kp), (vi, vp)):
        check(lib.cid_gather_pack_f16(_p(kv_txt), _p(kv_ip), idx.data_ptr(), _p(dst), R, L * 2 * C_, idx.numel(), _stream()),
              "cid_gather_pack_f16")


def context_kv(ehs: torch.Tensor, w_txt: torch.Tensor, w_ip: torch.Tensor, *, R: int, L: int, C_: int, heads: int,
               n_txt: int, n_ip: int, v3: bool, kp: Optional[torch.Tensor] = None, vp: Optional[torch.Tensor] = None,
               long: bool = False):
    """The packed K/V of one cross-attention layer for context rows ``ehs`` [R, L, Dc]: both [K | V] projections
    (``w_txt`` / ``w_ip`` [2 C, Dc]), then the operand layout of the third-generation fused kernel (``v3``), of the
    long-context kernel (``long``: run-time key-tile count, csrc/xattn_long.hip) or of the first-generation kernels.
    ``kp`` / ``vp`` are written in place where their size fits (a captured step keeps their addresses).  Returns
    (kp, vp, whether they are new tensors)."""
    assert not (v3 and long), "context_kv: one operand layout"
    M, Dc = R * L, ehs.shape[-1]
    kv_txt = torch.empty(M, 2 * C_, dtype=torch.float16, device=ehs.device)
    kv_ip = torch.empty(M, 2 * C_, dtype=torch.float16, device=ehs.device)
    gemm(ehs, w_txt, kv_txt, M=M, N=2 * C_, c1=Dc)
    gemm(ehs, w_ip, kv_ip, M=M, N=2 * C_, c1=Dc)
    if long:
        ke, ve = kv_pack_long_elems(C_, heads, n_txt, n_ip)
    else:
        ke, ve = kv_pack2_elems(C_, heads) if v3 else kv_pack_elems(C_, heads)
    # (both sizes: a K image of one layout can be as large as another layout's while the V^T images differ)
    moved = kp is None or kp.numel() != R * ke or vp.numel() != R * ve
    if moved:
        kp = torch.empty(R * ke, dtype=torch.float16, device=ehs.device)
        vp = torch.empty(R * ve, dtype=torch.float16, device=ehs.device)
    if long:
        kv_pack_long(kv_txt, kv_ip, kp, vp, R=R, C_=C_, heads=heads, n_txt=n_txt, n_ip=n_ip)
    elif v3:
        kv_pack2(kv_txt, kv_ip, kp, vp, R=R, L=L, C_=C_, heads=heads, n_txt=n_txt, n_ip=n_ip, order="reg")
    else:
        kv_pack(kv_txt, kv_ip, kp, vp, R=R, C_=C_, heads=heads, n_txt=n_txt, n_ip=n_ip)
    return kp, vp, moved


XATTN_GEN_DEFAULT = 3


def xattn_generation() -> int:
    """which fused cross-attention kernel serves the SD1.5 level-0 geometry: 3 = csrc/xattn3.hip,
    1 = the first-generation csrc/xattn.hip (A/B switch: CID_XATTN_GEN; CID_XATTN_V2=0 is the older spelling of 1)"""
    import os
    if os.environ.get("CID_XATTN_V2", "1") == "0":
        return 1
    return int(os.environ.get("CID_XATTN_GEN", str(XATTN_GEN_DEFAULT)))


def id_xattn3_supported(C_: int, heads: int, n_txt: int, n_ip: int) -> bool:
    return bool(_lib.load().cid_id_xattn3_supported(C_, heads, n_txt, n_ip))


def id_xattn3(x: torch.Tensor, out: torch.Tensor, *, wq_p: torch.Tensor, q_rowsum: torch.Tensor, q_bias: torch.Tensor,
              wo_p: torch.Tensor, bo: Optional[torch.Tensor], kp: torch.Tensor, vp: torch.Tensor, kvrow: torch.Tensor,
              B: int, N: int, C_: int, heads: int, n_txt: int, n_ip: int, ip_scale: float, has_ln: bool,
              add_residual: bool, ln_eps: float = 1e-5, ldo: Optional[int] = None):
    """third-generation fused identity cross-attention: ``wq_p`` / ``wo_p`` = xattn_pack.pack_w3 of the (LayerNorm-folded)
    query and the output projection; K / V operands from kv_pack2(order="reg").  ``ldo``: row pitch of ``out`` in halfs
    where it is a column block of a wider buffer (cid_id_xattn3_ld_f16); ``x`` is contiguous either way"""
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("wq_p", wq_p), ("wo_p", wo_p), ("kp", kp), ("vp", vp)):
        _req(t, f"id_xattn3.{name}")
    if bo is not None:
        _req(bo, "id_xattn3.bo")
    _req(q_rowsum, "id_xattn3.q_rowsum", torch.float32)
    _req(q_bias, "id_xattn3.q_bias", torch.float32)
    _req(kvrow, "id_xattn3.kvrow", torch.int32)
    flags = (1 if has_ln else 0) | (2 if add_residual else 0)
    if ldo is None:
        check(lib.cid_id_xattn3_f16(_p(x), _p(out), _p(wq_p), _p(q_rowsum), _p(q_bias), _p(wo_p), _p(bo), _p(kp), _p(vp),
                                    _p(kvrow), B, N, C_, heads, n_txt, n_ip, float(ip_scale), float(ln_eps), flags,
                                    _stream()), "cid_id_xattn3_f16")
    else:
        check(lib.cid_id_xattn3_ld_f16(_p(x), _p(out), ldo, _p(wq_p), _p(q_rowsum), _p(q_bias), _p(wo_p), _p(bo), _p(kp),
                                       _p(vp), _p(kvrow), B, N, C_, heads, n_txt, n_ip, float(ip_scale), float(ln_eps),
                                       flags, _stream()), "cid_id_xattn3_ld_f16")
    return out


def id_xattn_core(q: torch.Tensor, out: torch.Tensor, *, kp: torch.Tensor, vp: torch.Tensor, kvrow: torch.Tensor,
                  B: int, N: int, C_: int, heads: int, n_txt: int, n_ip: int, ip_scale: float):
    lib = _lib.load()
    for name, t in (("q", q), ("out", out), ("kp", kp), ("vp", vp)):
        _req(t, f"id_xattn_core.{name}")
    _req(kvrow, "id_xattn_core.kvrow", torch.int32)
    check(lib.cid_id_xattn_core_f16(_p(q), _p(out), _p(kp), _p(vp), _p(kvrow), B, N, C_, heads, n_txt, n_ip,
                                    float(ip_scale), _stream()), "cid_id_xattn_core_f16")
    return out


# --------------------------------------------------------------------------- norms
def layernorm(x: torch.Tensor, out: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, M: int, C_: int,
              eps: float = 1e-5, ldx: Optional[int] = None, ldo: Optional[int] = None):
    """``ldx`` / ``ldo``: row pitches in halfs where ``x`` / ``out`` is a column block of a wider buffer (cid_layernorm_ld_f16)"""
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("gamma", gamma), ("beta", beta)):
        _req(t, f"layernorm.{name}")
    if ldx is None and ldo is None:
        check(lib.cid_layernorm_f16(_p(x), _p(out), _p(gamma), _p(beta), M, C_, eps, _stream()), "cid_layernorm_f16")
    else:
        check(lib.cid_layernorm_ld_f16(_p(x), C_ if ldx is None else ldx, _p(out), C_ if ldo is None else ldo, _p(gamma),
                                       _p(beta), M, C_, eps, _stream()), "cid_layernorm_ld_f16")
    return out


GN_SMALL_MAX_HW = 256     # up to 16 x 16 pixels cid_groupnorm_f16 is ONE launch anyway (gn_small_kernel, GNS_MAXHW)


def groupnorm_ws_bytes(B: int, C_: int) -> int:
    return int(_lib.load().cid_groupnorm_ws_bytes(B, C_))


def groupnorm(x1: torch.Tensor, out: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, ws: torch.Tensor, *,
              B: int, HW: int, c1: int, x2: Optional[torch.Tensor] = None, c2: int = 0, groups: int = 32,
              eps: float = 1e-5, silu: bool = True):
    lib = _lib.load()
    for name, t in (("x1", x1), ("out", out), ("gamma", gamma), ("beta", beta)):
        _req(t, f"groupnorm.{name}")
    if x2 is not None:
        _req(x2, "groupnorm.x2")
    st1, st2 = getattr(x1, "_gn_stats", None), (getattr(x2, "_gn_stats", None) if x2 is not None else None)
    if st1 is not None and (x2 is None or st2 is not None) and HW > GN_SMALL_MAX_HW and \
            lib.cid_groupnorm_stats_ok(c1, c2, groups) and st1[0].shape[0] * st1[1] == B * HW and \
            (st2 is None or st2[0].shape[0] * st2[1] == B * HW):
        # statistics already emitted by the GEMM epilogue(s) that wrote x1 / x2: one launch, one read of x
        check(lib.cid_groupnorm_stats_f16(_p(x1), _p(x2), c1, c2, _p(out), _p(gamma), _p(beta), B, HW, groups, eps,
                                          1 if silu else 0, st1[0].data_ptr(), st1[1],
                                          st2[0].data_ptr() if st2 is not None else None, st2[1] if st2 is not None else 0,
                                          _stream()), "cid_groupnorm_stats_f16")
        return out
    if ws.numel() * ws.element_size() < groupnorm_ws_bytes(B, c1 + c2):
        raise _lib.CidError("groupnorm: workspace too small")
    check(lib.cid_groupnorm_f16(_p(x1), _p(x2), c1, c2, _p(out), _p(gamma), _p(beta), B, HW, groups, eps,
                                1 if silu else 0, ws.data_ptr(), _stream()), "cid_groupnorm_f16")
    return out


# --------------------------------------------------------------------------- UNet ends, time path, loop glue
def conv_in(sample: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, B: int, Bin: int,
            cin: int, H: int, W: int, cout: int, in_scale: Optional[torch.Tensor] = None,
            extra: Optional[torch.Tensor] = None):
    """``in_scale``: fp32 device scalar multiplying the sample (scheduler.scale_model_input); ``extra``: NCHW
    [Bin, cin - sample channels, H, W] read as the trailing input channels, unscaled (9-channel inpainting UNets:
    cat([mask, masked_image_latents]), inpaint ref :320-321)"""
    lib = _lib.load()
    for name, t in (("sample", sample), ("out", out), ("w", w), ("bias", bias)):
        _req(t, f"conv_in.{name}")
    if in_scale is not None:
        _req(in_scale, "conv_in.in_scale", torch.float32)
    if extra is not None:
        _req(extra, "conv_in.extra")
        cin1, cin2 = sample.shape[1], extra.shape[1]
        if cin1 + cin2 != cin or extra.shape[0] != Bin or tuple(extra.shape[2:]) != (H, W):
            raise _lib.CidError(f"conv_in: sample {tuple(sample.shape)} + extra {tuple(extra.shape)} do not make {cin} channels")
        check(lib.cid_conv_in_cat_f16(_p(sample), cin1, _p(extra), cin2, _p(out), _p(w), _p(bias), B, Bin, H, W, cout,
                                      _p(in_scale), _stream()), "cid_conv_in_cat_f16")
        return out
    check(lib.cid_conv_in_f16(_p(sample), _p(out), _p(w), _p(bias), B, Bin, cin, H, W, cout, _p(in_scale), _stream()),
          "cid_conv_in_f16")
    return out


def gelu_(x: torch.Tensor):
    """in-place exact-erf GELU"""
    lib = _lib.load()
    _req(x, "gelu.x")
    check(lib.cid_gelu_f16(_p(x), x.numel(), _stream()), "cid_gelu_f16")
    return x


def quick_gelu_(x: torch.Tensor):
    """in-place x * sigmoid(1.702 x) (CLIP's quick_gelu)"""
    lib = _lib.load()
    _req(x, "quick_gelu.x")
    check(lib.cid_quick_gelu_f16(_p(x), x.numel(), _stream()), "cid_quick_gelu_f16")
    return x


def clip_head(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w_proj: torch.Tensor, *, B: int, ldx: int,
              eps: float = 1e-5, concepts: Optional[torch.Tensor] = None, thresholds: Optional[torch.Tensor] = None,
              n_special: int = 0, embeds: Optional[torch.Tensor] = None):
    """The tail of the CLIP vision tower and of the safety checker in one launch (cid_clip_head_f16): post_layernorm of the
    CLS row of each of ``B`` images (row b at ``x`` + b * ``ldx``), ``w_proj`` [P, C], then -- with ``concepts`` fp32 [K, P]
    (L2-normalised rows, the ``n_special`` special-care rows first) and ``thresholds`` fp32 [K] -- the cosines and the
    decision.  Returns (cos [B, K] fp32, scores [B, K] fp32, flags [B] int32), or ``embeds`` when there are no concepts."""
    lib = _lib.load()
    for name, t in (("x", x), ("gamma", gamma), ("beta", beta), ("w_proj", w_proj)) + ((("embeds", embeds),) if embeds is not None else ()):
        _req(t, f"clip_head.{name}")
    P, C_ = w_proj.shape
    if x.numel() < (B - 1) * ldx + C_ or gamma.numel() != C_ or beta.numel() != C_ or not w_proj.is_contiguous():
        raise _lib.CidError(f"clip_head: x of {x.numel()} elements / gamma / beta do not hold B = {B} rows of C = {C_} at pitch {ldx}")
    if embeds is not None and (embeds.numel() != B * P or not embeds.is_contiguous()):
        raise _lib.CidError(f"clip_head: embeds must be contiguous [{B}, {P}]")
    K = 0
    cos = scores = flags = None
    if concepts is not None:
        _req(concepts, "clip_head.concepts", torch.float32)
        _req(thresholds, "clip_head.thresholds", torch.float32)
        K = concepts.shape[0]
        if tuple(concepts.shape) != (K, P) or thresholds.numel() != K or not concepts.is_contiguous():
            raise _lib.CidError(f"clip_head: concepts {tuple(concepts.shape)} / thresholds {tuple(thresholds.shape)} against P = {P}")
        cos = torch.empty(B, K, dtype=torch.float32, device=x.device)
        scores = torch.empty(B, K, dtype=torch.float32, device=x.device)
        flags = torch.empty(B, dtype=torch.int32, device=x.device)
    check(lib.cid_clip_head_f16(_p(x), ldx, _p(gamma), _p(beta), eps, _p(w_proj), _p(concepts), _p(thresholds), B, C_, P, K,
                                n_special, _p(embeds), _p(cos), _p(scores), _p(flags), _stream()), "cid_clip_head_f16")
    return (cos, scores, flags) if K else embeds


def blackout_(images: torch.Tensor, flags: torch.Tensor):
    """in place: image b of fp16 ``images`` [B, ...] becomes zero where ``flags`` [B] (int32, on the GPU) is non-zero; nothing
    is read back"""
    lib = _lib.load()
    if not images.is_cuda or images.dtype != torch.float16 or not images.is_contiguous():
        raise _lib.CidError(f"blackout.images: a contiguous fp16 GPU tensor is expected (got {images.dtype} on {images.device})")
    _req(flags, "blackout.flags", torch.int32)
    B = images.shape[0]
    if flags.numel() != B:
        raise _lib.CidError(f"blackout: {flags.numel()} flags for {B} images")
    check(lib.cid_blackout_f16(_p(images), _p(flags), B, images.numel() // B, _stream()), "cid_blackout_f16")
    return images


def text_embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, *, B: int, T: int, Tp: int):
    """CLIPTextEmbeddings: ``out`` [B, Tp, C] = tok[ids] + pos[:T], zero rows for t >= T.  ``ids`` int32 [B, T] on the GPU,
    already range-checked by the caller (clip_text.check_ids)"""
    lib = _lib.load()
    _req(ids, "text_embed.ids", torch.int32)
    for name, t in (("tok", tok), ("pos", pos), ("out", out)):
        _req(t, f"text_embed.{name}")
    V, C_ = tok.shape
    check(lib.cid_text_embed_f16(_p(ids), B, T, Tp, _p(tok), _p(pos), _p(out), V, C_, _stream()), "cid_text_embed_f16")
    return out


def small_attn(q: torch.Tensor, kv1: torch.Tensor, kv2: Optional[torch.Tensor], out: torch.Tensor, *, B: int, Lq: int,
               n1: int, n2: int, heads: int, dim_head: int = 64):
    """PerceiverAttention core: q [B*Lq, heads*64], kv* [B*n*, 2*heads*64] ([K | V] rows), out [B*Lq, heads*64]"""
    lib = _lib.load()
    for name, t in (("q", q), ("kv1", kv1), ("out", out)) + ((("kv2", kv2),) if kv2 is not None else ()):
        _req(t, f"small_attn.{name}")
    inner = heads * dim_head
    check(lib.cid_small_attn_f16(_p(q), inner, _p(kv1), n1, _p(kv2), n2, 2 * inner, _p(out), inner, B, Lq, heads,
                                 dim_head, dim_head ** -0.5, _stream()), "cid_small_attn_f16")
    return out


def softmax_rows(x: torch.Tensor, *, rows: int, cols: int, ld: int):
    """in-place base-2 softmax over fp16 rows (VAE mid-block attention scores)"""
    lib = _lib.load()
    _req(x, "softmax_rows.x")
    check(lib.cid_softmax_rows_f16(_p(x), rows, cols, ld, _stream()), "cid_softmax_rows_f16")
    return x


def conv3x3_small(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, B: int, Hi: int, Wi: int,
                  cin: int, cout: int, stride: int = 1, silu: bool = False):
    """token-major [B, Hi*Wi, cin] -> [B, Ho*Wo, cout]; small-channel direct convolution (ControlNet condition embedding)."""
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("w", w), ("bias", bias)):
        _req(t, f"conv3x3_small.{name}")
    check(lib.cid_conv3x3_small_f16(_p(x), _p(out), _p(w), _p(bias), B, Hi, Wi, cin, cout, stride, int(silu), _stream()),
          "cid_conv3x3_small_f16")
    return out


def conv_out(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, B: int, H: int, W: int,
             cin: int, cout: int):
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("w", w), ("bias", bias)):
        _req(t, f"conv_out.{name}")
    check(lib.cid_conv_out_f16(_p(x), _p(out), _p(w), _p(bias), B, H, W, cin, cout, _stream()), "cid_conv_out_f16")
    return out


def vae_encode_in(image: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *,
                  mask: Optional[torch.Tensor] = None, normalize: bool = True, blocks: int = 1,
                  mask_latents: Optional[torch.Tensor] = None):
    """VAE encoder conv_in with the inpaint pre-processing folded in (cid_vae_encode_in_f16): ``image`` fp32 [Bi, 3, H, W],
    ``mask`` fp32 [Bm, 1, H, W] or None; ``blocks`` bit 0 = the image, bit 1 = image * (mask < 0.5); ``out`` token-major
    [nblk * Bi, H * W, cout]; ``mask_latents`` fp16 [Bm, 1, H / 8, W / 8] or None."""
    lib = _lib.load()
    _req(image, "vae_encode_in.image", torch.float32)
    for name, t in (("out", out), ("w", w), ("bias", bias)):
        _req(t, f"vae_encode_in.{name}")
    if mask is not None:
        _req(mask, "vae_encode_in.mask", torch.float32)
    if mask_latents is not None:
        _req(mask_latents, "vae_encode_in.mask_latents")
    Bi, _, H, W = image.shape
    check(lib.cid_vae_encode_in_f16(_p(image), Bi, _p(mask), mask.shape[0] if mask is not None else 0, _p(out), _p(w),
                                    _p(bias), H, W, out.shape[-1], int(normalize), blocks, _p(mask_latents), _stream()),
          "cid_vae_encode_in_f16")
    return out


def vae_encode_out(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, B: int, H: int, W: int,
                   cin: int, L: int, scale: float, eps: Optional[torch.Tensor] = None,
                   moments: Optional[torch.Tensor] = None):
    """VAE encoder conv_out + quant_conv (folded into ``w`` / fp32 ``bias``) + posterior (cid_vae_encode_out_f16):
    ``out`` fp16 [B, L, H, W] = scale * (mean + std * eps) (the mean when ``eps`` is None); ``moments`` fp32 [B, 2L, H, W]."""
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("w", w)):
        _req(t, f"vae_encode_out.{name}")
    _req(bias, "vae_encode_out.bias", torch.float32)
    if eps is not None:
        _req(eps, "vae_encode_out.eps")
    if moments is not None:
        _req(moments, "vae_encode_out.moments", torch.float32)
    check(lib.cid_vae_encode_out_f16(_p(x), _p(out), _p(moments), _p(w), _p(bias), _p(eps), B, H, W, cin, L, float(scale),
                                     _stream()), "cid_vae_encode_out_f16")
    return out


# --------------------------------------------------------------------------- AutoencoderTiny decoder (csrc/taesd.hip)
def _req_shape(t: torch.Tensor, name: str, shape, dtype=torch.float16):
    """dtype, the exact shape and contiguity of one operand (host-side facts: every operand is held to them first, then
    ``_req`` tests device and alignment)"""
    if t.dtype != dtype:
        raise _lib.CidError(f"{name}: expected {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise _lib.CidError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise _lib.CidError(f"{name}: tensor must be contiguous")


def tiny_conv64_tile():
    """(tile_h, tile_w, grid_cap) of cid_tiny_conv64_f16: its output tile and the most workgroups a launch has"""
    v = [C.c_int32() for _ in range(3)]
    _lib.load().cid_tiny_conv64_tile(*(C.byref(i) for i in v))
    return tuple(i.value for i in v)


def tiny_conv64(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, B: int, H: int,
                W: int, res: Optional[torch.Tensor] = None, relu: bool = False, up: bool = False):
    """AutoencoderTiny's 64 -> 64 3x3 convolution (cid_tiny_conv64_f16): ``x`` token-major [B, H * W, 64], ``out``
    [B, Ho * Wo, 64] with (Ho, Wo) = (H, W), or (2H, 2W) with ``up`` (nearest 2x in front of the conv, never materialised);
    ``w`` [64, 9, 64] = [cout, tap, cin]; out = act(conv + bias + res)."""
    lib = _lib.load()
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    _req_shape(x, "tiny_conv64.x", (B, H * W, 64))
    _req_shape(out, "tiny_conv64.out", (B, Ho * Wo, 64))
    _req_shape(w, "tiny_conv64.w", (64, 9, 64))
    if bias is not None:
        _req_shape(bias, "tiny_conv64.bias", (64,))
    if res is not None:
        _req_shape(res, "tiny_conv64.res", (B, Ho * Wo, 64))
    for name, t in (("x", x), ("out", out), ("w", w), ("bias", bias), ("res", res)):
        if t is not None:
            _req(t, f"tiny_conv64.{name}")
    check(lib.cid_tiny_conv64_f16(_p(x), _p(out), _p(w), _p(bias), _p(res), B, H, W, int(bool(up)), int(bool(relu)), _stream()),
          "cid_tiny_conv64_f16")
    return out


def tiny_decode_in(z: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor):
    """AutoencoderTiny's decoder head (cid_tiny_decode_in_f16): ``z`` NCHW latents [B, 4, h, w] -> relu(conv(tanh(z / 3) * 3) +
    bias), token-major [B, h * w, 64]; ``w`` [64, 9, 4]."""
    lib = _lib.load()
    if z.dim() != 4 or z.shape[1] != 4:
        raise _lib.CidError(f"tiny_decode_in.z: expected [B, 4, h, w], got {tuple(z.shape)}")
    _req_shape(z, "tiny_decode_in.z", z.shape)
    B, _, H, W = z.shape
    _req_shape(out, "tiny_decode_in.out", (B, H * W, 64))
    _req_shape(w, "tiny_decode_in.w", (64, 9, 4))
    _req_shape(bias, "tiny_decode_in.bias", (64,))
    if not z.is_cuda:       # (the NCHW latents need no alignment: a batch slice at an odd size is read as it is)
        raise _lib.CidError(f"tiny_decode_in.z: tensor must live on the GPU (got {z.device}); libcid has no CPU path")
    for name, t in (("out", out), ("w", w), ("bias", bias)):
        _req(t, f"tiny_decode_in.{name}")
    check(lib.cid_tiny_decode_in_f16(_p(z), _p(out), _p(w), _p(bias), B, H, W, _stream()), "cid_tiny_decode_in_f16")
    return out


def tiny_decode_out(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, clamp01: bool = False):
    """AutoencoderTiny's decoder tail (cid_tiny_decode_out_f16): ``x`` token-major [B, H * W, 64] -> v = conv + bias; ``out``
    NCHW [B, 3, H, W] = 2 v - 1, or clamp(v, 0, 1) with ``clamp01`` (decode_latents' range); ``w`` [3, 9, 64]."""
    lib = _lib.load()
    if out.dim() != 4 or out.shape[1] != 3:
        raise _lib.CidError(f"tiny_decode_out.out: expected [B, 3, H, W], got {tuple(out.shape)}")
    _req_shape(out, "tiny_decode_out.out", out.shape)
    B, _, H, W = out.shape
    _req_shape(x, "tiny_decode_out.x", (B, H * W, 64))
    _req_shape(w, "tiny_decode_out.w", (3, 9, 64))
    _req_shape(bias, "tiny_decode_out.bias", (3,))
    for name, t in (("x", x), ("out", out), ("w", w), ("bias", bias)):
        _req(t, f"tiny_decode_out.{name}")
    check(lib.cid_tiny_decode_out_f16(_p(x), _p(out), _p(w), _p(bias), B, H, W, int(bool(clamp01)), _stream()),
          "cid_tiny_decode_out_f16")
    return out


# --------------------------------------------------------------------------- AutoencoderTiny encoder (csrc/taesd.hip)
def tiny_conv64_s2_tile():
    """(tile_h, tile_w, grid_cap) of cid_tiny_conv64_s2_f16: its output tile and the most workgroups a launch has"""
    v = [C.c_int32() for _ in range(3)]
    _lib.load().cid_tiny_conv64_s2_tile(*(C.byref(i) for i in v))
    return tuple(i.value for i in v)


def tiny_conv64_s2(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, *, B: int, H: int, W: int):
    """AutoencoderTiny's stride-2, pad-1, bias-less 64 -> 64 convolution (cid_tiny_conv64_s2_f16): ``x`` token-major
    [B, H * W, 64] -> ``out`` [B, ceil(H / 2) * ceil(W / 2), 64]; ``w`` [64, 9, 64] = [cout, tap, cin]."""
    lib = _lib.load()
    _req_shape(x, "tiny_conv64_s2.x", (B, H * W, 64))
    _req_shape(out, "tiny_conv64_s2.out", (B, ((H + 1) // 2) * ((W + 1) // 2), 64))
    _req_shape(w, "tiny_conv64_s2.w", (64, 9, 64))
    for name, t in (("x", x), ("out", out), ("w", w)):
        _req(t, f"tiny_conv64_s2.{name}")
    check(lib.cid_tiny_conv64_s2_f16(_p(x), _p(out), _p(w), B, H, W, _stream()), "cid_tiny_conv64_s2_f16")
    return out


def tiny_encode_in(image: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *,
                   mask: Optional[torch.Tensor] = None, normalize: bool = False, blocks: int = 1,
                   mask_latents: Optional[torch.Tensor] = None):
    """AutoencoderTiny's encoder head with the inpaint pre-processing folded in (cid_tiny_encode_in_f16): ``image`` fp32
    [Bi, 3, H, W], ``mask`` fp32 [Bm, 1, H, W] (Bm in {1, Bi}) or None; ``blocks`` bit 0 = the image, bit 1 = image *
    (mask < 0.5); ``out`` token-major [nblk * Bi, H * W, 64] = conv(half(v + 1) / 2) + bias; ``w`` [64, 9, 3];
    ``mask_latents`` fp16 [Bm, 1, H / 8, W / 8] or None."""
    lib = _lib.load()
    if image.dim() != 4 or image.shape[1] != 3:
        raise _lib.CidError(f"tiny_encode_in.image: expected [B, 3, H, W], got {tuple(image.shape)}")
    _req_shape(image, "tiny_encode_in.image", image.shape, torch.float32)
    Bi, _, H, W = image.shape
    if blocks not in (1, 2, 3):
        raise _lib.CidError(f"tiny_encode_in.blocks: 1 (image), 2 (masked image) or 3 (both), got {blocks!r}")
    _req_shape(out, "tiny_encode_in.out", (Bi * (2 if blocks == 3 else 1), H * W, 64))
    _req_shape(w, "tiny_encode_in.w", (64, 9, 3))
    _req_shape(bias, "tiny_encode_in.bias", (64,))
    if mask is not None:
        if mask.dim() != 4 or mask.shape[0] not in (1, Bi) or tuple(mask.shape[1:]) != (1, H, W):
            raise _lib.CidError(f"tiny_encode_in.mask: expected [1 or {Bi}, 1, {H}, {W}], got {tuple(mask.shape)}")
        _req_shape(mask, "tiny_encode_in.mask", mask.shape, torch.float32)
    elif blocks & 2 or mask_latents is not None:
        raise _lib.CidError("tiny_encode_in.mask: the masked image and mask_latents need a mask")
    if mask_latents is not None:
        if H % 8 or W % 8:
            raise _lib.CidError(f"tiny_encode_in.mask_latents: H and W must be multiples of 8 (got {H} x {W})")
        _req_shape(mask_latents, "tiny_encode_in.mask_latents", (mask.shape[0], 1, H // 8, W // 8))
    if not image.is_cuda:   # (the fp32 NCHW planes need no alignment)
        raise _lib.CidError(f"tiny_encode_in.image: tensor must live on the GPU (got {image.device}); libcid has no CPU path")
    if mask is not None and not mask.is_cuda:
        raise _lib.CidError(f"tiny_encode_in.mask: tensor must live on the GPU (got {mask.device}); libcid has no CPU path")
    if mask_latents is not None and not mask_latents.is_cuda:
        raise _lib.CidError(f"tiny_encode_in.mask_latents: tensor must live on the GPU (got {mask_latents.device}); "
                            "libcid has no CPU path")
    for name, t in (("out", out), ("w", w), ("bias", bias)):
        _req(t, f"tiny_encode_in.{name}")
    check(lib.cid_tiny_encode_in_f16(_p(image), Bi, _p(mask), mask.shape[0] if mask is not None else 0, _p(out), _p(w),
                                     _p(bias), H, W, int(bool(normalize)), blocks, _p(mask_latents), _stream()),
          "cid_tiny_encode_in_f16")
    return out


def tiny_encode_out(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, scale: float = 1.0):
    """AutoencoderTiny's encoder tail (cid_tiny_encode_out_f16): ``x`` token-major [B, H * W, 64] -> ``out`` NCHW [B, 4, H, W]
    = (conv + bias) * scale; ``w`` [4, 9, 64]."""
    lib = _lib.load()
    if out.dim() != 4 or out.shape[1] != 4:
        raise _lib.CidError(f"tiny_encode_out.out: expected [B, 4, H, W], got {tuple(out.shape)}")
    _req_shape(out, "tiny_encode_out.out", out.shape)
    B, _, H, W = out.shape
    _req_shape(x, "tiny_encode_out.x", (B, H * W, 64))
    _req_shape(w, "tiny_encode_out.w", (4, 9, 64))
    _req_shape(bias, "tiny_encode_out.bias", (4,))
    if not out.is_cuda:     # (the NCHW planes need no alignment)
        raise _lib.CidError(f"tiny_encode_out.out: tensor must live on the GPU (got {out.device}); libcid has no CPU path")
    for name, t in (("x", x), ("w", w), ("bias", bias)):
        _req(t, f"tiny_encode_out.{name}")
    check(lib.cid_tiny_encode_out_f16(_p(x), _p(out), _p(w), _p(bias), B, H, W, float(scale), _stream()),
          "cid_tiny_encode_out_f16")
    return out


# --------------------------------------------------------------------------- face parser (csrc/parsing.hip)
def parse_stem(img: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: torch.Tensor):
    """BiSeNet stem (cid_parse_stem_f16): ``img`` uint8 [B, H, W, 3] -> ImageNet normalisation -> conv 7x7/2 (fp32 ``w``
    [64, 7, 7, 3], BN folded, fp32 ``bias`` [64]) -> ReLU -> maxpool 3x3/2 -> ``out`` fp16 [B, H/4 * W/4, 64]."""
    lib = _lib.load()
    _req(img, "parse_stem.img", torch.uint8)
    _req(out, "parse_stem.out")
    _req(w, "parse_stem.w", torch.float32)
    _req(bias, "parse_stem.bias", torch.float32)
    B, H, W, _ = img.shape
    check(lib.cid_parse_stem_f16(_p(img), _p(out), _p(w), _p(bias), B, H, W, _stream()), "cid_parse_stem_f16")
    return out


def chan_mean(x: torch.Tensor, out: torch.Tensor, *, B: int, HW: int, C_: int, ld: Optional[int] = None):
    """fp32 ``out`` [B, C] = the mean over the HW tokens of ``x`` [B, HW, ld] (cid_chan_mean_f16)."""
    lib = _lib.load()
    _req(x, "chan_mean.x")
    _req(out, "chan_mean.out", torch.float32)
    check(lib.cid_chan_mean_f16(_p(x), _p(out), B, HW, C_, ld if ld is not None else C_, _stream()), "cid_chan_mean_f16")
    return out


def chan_gate(mean: torch.Tensor, out: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor] = None,
              w2: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None, *, act: int):
    """fp32 ``out`` [B, N] = act(W1 m + b1), or act(W2 ReLU(W1 m + b1) + b2) with ``w2``; act 0 none, 1 ReLU, 2 sigmoid
    (cid_chan_gate_f32).  Every tensor fp32, weights [out, in]."""
    lib = _lib.load()
    for name, t in (("mean", mean), ("out", out), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if t is not None:
            _req(t, f"chan_gate.{name}", torch.float32)
    B, K = mean.shape
    N1 = w1.shape[0]
    N = w2.shape[0] if w2 is not None else N1
    check(lib.cid_chan_gate_f32(_p(mean), _p(out), _p(w1), _p(b1), _p(w2), _p(b2), B, K, N1, N, act, _stream()),
          "cid_chan_gate_f32")
    return out


def chan_affine(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor, *, B: int, HW: int, C_: int,
                t: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None):
    """``out`` = x * s[b][c] + (t[b][c] | res | x) (cid_chan_affine_f16); ``s`` / ``t`` fp32 [B, C]."""
    lib = _lib.load()
    _req(x, "chan_affine.x")
    _req(out, "chan_affine.out")
    _req(s, "chan_affine.s", torch.float32)
    if t is not None:
        _req(t, "chan_affine.t", torch.float32)
    if res is not None:
        _req(res, "chan_affine.res")
    check(lib.cid_chan_affine_f16(_p(x), _p(s), _p(t), _p(res), _p(out), B, HW, C_, _stream()), "cid_chan_affine_f16")
    return out


def parse_head(logits: torch.Tensor, labels: torch.Tensor, *, ncls: int, B: int, h: int, w: int, H: int, W: int,
               ld: Optional[int] = None, logits_out: Optional[torch.Tensor] = None):
    """bilinear (align_corners=True) upsampling of ``logits`` fp16 [B, h * w, ld] to H x W and the first-maximum argmax over
    the first ``ncls`` channels -> ``labels`` uint8 [B, H, W]; ``logits_out`` fp32 [B, ncls, H, W] or None
    (cid_parse_head_f16)."""
    lib = _lib.load()
    _req(logits, "parse_head.logits")
    _req(labels, "parse_head.labels", torch.uint8)
    if logits_out is not None:
        _req(logits_out, "parse_head.logits_out", torch.float32)
    check(lib.cid_parse_head_f16(_p(logits), ld if ld is not None else logits.shape[-1], ncls, B, h, w, H, W, _p(labels),
                                 _p(logits_out), _stream()), "cid_parse_head_f16")
    return labels


def sincos_embed(v: torch.Tensor, out: torch.Tensor, *, rows: int, dim: int):
    lib = _lib.load()
    _req(v, "sincos_embed.v", torch.float32)
    _req(out, "sincos_embed.out")
    check(lib.cid_sincos_embed_f16(_p(v), _p(out), rows, dim, _stream()), "cid_sincos_embed_f16")
    return out


def linear_small(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], out: torch.Tensor, *, M: int, N: int,
                 K: int, ldx: Optional[int] = None, ldo: Optional[int] = None, add: Optional[torch.Tensor] = None,
                 ldadd: int = 0, act_in: int = 0, act_out: int = 0):
    lib = _lib.load()
    for name, t in (("x", x), ("w", w), ("out", out)):
        _req(t, f"linear_small.{name}")
    check(lib.cid_linear_small_f16(_p(x), ldx if ldx is not None else K, _p(w), _p(b), _p(add), ldadd, _p(out),
                                   ldo if ldo is not None else N, M, N, K, act_in, act_out, _stream()),
          "cid_linear_small_f16")
    return out


def cfg_rescale(eps: torch.Tensor, guidance: float, rescale: float, escale: torch.Tensor, *, B: int, per_sample: int):
    """guidance_rescale's per-sample factor (cid.h, cid_cfg_rescale_f16): ``eps`` fp16 [2B, per_sample] (uncond first) ->
    ``escale`` fp32 [B] = 1 - rescale + rescale * std(cond) / std(guided); one launch, deterministic"""
    lib = _lib.load()
    _req(eps, "cfg_rescale.eps")
    _req(escale, "cfg_rescale.escale", torch.float32)
    if eps.numel() != 2 * B * per_sample or escale.numel() != B:
        raise _lib.CidError(f"cfg_rescale: eps / escale hold {eps.numel()} / {escale.numel()} elements; B = {B}, per_sample = "
                            f"{per_sample} need {2 * B * per_sample} / {B}")
    check(lib.cid_cfg_rescale_f16(_p(eps), float(guidance), float(rescale), _p(escale), B, per_sample, _stream()),
          "cid_cfg_rescale_f16")
    return escale


def _req_escale(escale: torch.Tensor, B: int, what: str):
    _req(escale, f"{what}.escale", torch.float32)
    if escale.numel() != B:
        raise _lib.CidError(f"{what}.escale: {escale.numel()} elements, B = {B}")


def cfg_ddim_step(eps: torch.Tensor, latents: torch.Tensor, coef: torch.Tensor, guidance: float, *, B: int,
                  per_sample: int, mask: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
                  noise: Optional[torch.Tensor] = None, escale: Optional[torch.Tensor] = None):
    """``escale`` fp32 [B] (``cfg_rescale``): the guided prediction of sample b is multiplied by escale[b]
    (cid_cfg_ddim_step_scaled_f16); None is the unscaled entry"""
    lib = _lib.load()
    _req(eps, "cfg_ddim_step.eps")
    _req(latents, "cfg_ddim_step.latents")
    _req(coef, "cfg_ddim_step.coef", torch.float32)
    if escale is not None:
        _req_escale(escale, B, "cfg_ddim_step")
        check(lib.cid_cfg_ddim_step_scaled_f16(_p(eps), _p(latents), _p(coef), float(guidance), _p(mask), _p(init), _p(noise),
                                               B, per_sample, _p(escale), _stream()), "cid_cfg_ddim_step_scaled_f16")
        return latents
    check(lib.cid_cfg_ddim_step_f16(_p(eps), _p(latents), _p(coef), float(guidance), _p(mask), _p(init), _p(noise),
                                    B, per_sample, _stream()), "cid_cfg_ddim_step_f16")
    return latents


def cfg_multistep_step(eps: torch.Tensor, latents: torch.Tensor, hist: torch.Tensor, saved: torch.Tensor, row: torch.Tensor,
                       guidance: float, *, B: int, per_sample: int, z: Optional[torch.Tensor] = None,
                       mask: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
                       noise: Optional[torch.Tensor] = None, escale: Optional[torch.Tensor] = None):
    """CFG + one step of PNDM / DPM-Solver++ 2M / DDIM with eta (cid.h, "multistep row").  ``row``: 16 fp32 words on the
    device (the integer words bit-cast), ``hist`` fp32 [4, B * per_sample], ``saved`` fp16 [B * per_sample], ``z`` fp16
    [rows, B * per_sample] or None; ``escale`` fp32 [B] or None as in ``cfg_ddim_step``."""
    lib = _lib.load()
    n = B * per_sample
    _req(eps, "cfg_multistep_step.eps")
    _req(latents, "cfg_multistep_step.latents")
    _req(hist, "cfg_multistep_step.hist", torch.float32)
    _req(saved, "cfg_multistep_step.saved")
    _req(row, "cfg_multistep_step.row", torch.float32)
    if eps.numel() != 2 * n or latents.numel() != n or hist.numel() != 4 * n or saved.numel() != n or row.numel() != 16:
        raise _lib.CidError(f"cfg_multistep_step: eps / latents / hist / saved / row hold {eps.numel()} / {latents.numel()} / "
                            f"{hist.numel()} / {saved.numel()} / {row.numel()} elements; B * per_sample = {n} needs "
                            f"{2 * n} / {n} / {4 * n} / {n} / 16")
    z_rows = 0
    if z is not None:
        _req(z, "cfg_multistep_step.z")
        if z.numel() == 0 or z.numel() % n:
            raise _lib.CidError(f"cfg_multistep_step.z: {z.numel()} elements are not rows of B * per_sample = {n}")
        z_rows = z.numel() // n
    for name, t in (("mask", mask), ("init", init), ("noise", noise)):
        if t is not None:
            _req(t, f"cfg_multistep_step.{name}")
            if t.numel() != n:
                raise _lib.CidError(f"cfg_multistep_step.{name}: {t.numel()} elements, B * per_sample = {n}")
    if escale is not None:
        _req_escale(escale, B, "cfg_multistep_step")
        check(lib.cid_cfg_multistep_step_scaled_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row),
                                                    float(guidance), _p(mask), _p(init), _p(noise), B, per_sample,
                                                    _p(escale), _stream()), "cid_cfg_multistep_step_scaled_f16")
        return latents
    check(lib.cid_cfg_multistep_step_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row), float(guidance),
                                         _p(mask), _p(init), _p(noise), B, per_sample, _stream()),
          "cid_cfg_multistep_step_f16")
    return latents


def multistep_step(eps: torch.Tensor, latents: torch.Tensor, hist: torch.Tensor, saved: torch.Tensor, row: torch.Tensor, *,
                   B: int, per_sample: int, z: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                   init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
    """``cfg_multistep_step`` without classifier-free guidance (cid_multistep_step_f16, the single pass): ``eps`` fp16
    [B, per_sample] is the model output itself; every other argument as there."""
    lib = _lib.load()
    n = B * per_sample
    _req(eps, "multistep_step.eps")
    _req(latents, "multistep_step.latents")
    _req(hist, "multistep_step.hist", torch.float32)
    _req(saved, "multistep_step.saved")
    _req(row, "multistep_step.row", torch.float32)
    if eps.numel() != n or latents.numel() != n or hist.numel() != 4 * n or saved.numel() != n or row.numel() != 16:
        raise _lib.CidError(f"multistep_step: eps / latents / hist / saved / row hold {eps.numel()} / {latents.numel()} / "
                            f"{hist.numel()} / {saved.numel()} / {row.numel()} elements; B * per_sample = {n} needs "
                            f"{n} / {n} / {4 * n} / {n} / 16")
    z_rows = 0
    if z is not None:
        _req(z, "multistep_step.z")
        if z.numel() == 0 or z.numel() % n:
            raise _lib.CidError(f"multistep_step.z: {z.numel()} elements are not rows of B * per_sample = {n}")
        z_rows = z.numel() // n
    for name, t in (("mask", mask), ("init", init), ("noise", noise)):
        if t is not None:
            _req(t, f"multistep_step.{name}")
            if t.numel() != n:
                raise _lib.CidError(f"multistep_step.{name}: {t.numel()} elements, B * per_sample = {n}")
    check(lib.cid_multistep_step_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row), _p(mask), _p(init),
                                     _p(noise), B, per_sample, _stream()), "cid_multistep_step_f16")
    return latents


def _req_pag(pag: torch.Tensor, what: str):
    _req(pag, f"{what}.pag", torch.float32)
    if pag.numel() != 1:
        raise _lib.CidError(f"{what}.pag: {pag.numel()} elements; one DEVICE fp32 value (the step's PAG scale)")


def _req_step_blend(what: str, n: int, mask, init, noise):
    for name, t in (("mask", mask), ("init", init), ("noise", noise)):
        if t is not None:
            _req(t, f"{what}.{name}")
            if t.numel() != n:
                raise _lib.CidError(f"{what}.{name}: {t.numel()} elements, B * per_sample = {n}")


def cfg_pag_ddim_step(eps: torch.Tensor, latents: torch.Tensor, coef: torch.Tensor, guidance: float, pag: torch.Tensor, *,
                      B: int, per_sample: int, mask: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
                      noise: Optional[torch.Tensor] = None):
    """``cfg_ddim_step`` with perturbed-attention guidance (cid_cfg_pag_ddim_step_f16): ``eps`` fp16 [3B, per_sample] =
    [uncond | cond | perturbed], e = u + g (c - u) + s (c - p) with s = ``pag`` -- ONE fp32 value on the device, so that a
    captured launch follows the step table; at s == 0 the perturbed rows are not read and the bits are ``cfg_ddim_step``'s"""
    lib = _lib.load()
    n = B * per_sample
    _req(eps, "cfg_pag_ddim_step.eps")
    _req(latents, "cfg_pag_ddim_step.latents")
    _req(coef, "cfg_pag_ddim_step.coef", torch.float32)
    _req_pag(pag, "cfg_pag_ddim_step")
    if eps.numel() != 3 * n or latents.numel() != n or coef.numel() < 4:
        raise _lib.CidError(f"cfg_pag_ddim_step: eps / latents / coef hold {eps.numel()} / {latents.numel()} / {coef.numel()} "
                            f"elements; B * per_sample = {n} needs {3 * n} / {n} / at least 4")
    _req_step_blend("cfg_pag_ddim_step", n, mask, init, noise)
    check(lib.cid_cfg_pag_ddim_step_f16(_p(eps), _p(latents), _p(coef), float(guidance), _p(pag), _p(mask), _p(init), _p(noise),
                                        B, per_sample, _stream()), "cid_cfg_pag_ddim_step_f16")
    return latents


def _pag_multistep(what: str, eps_rows: int, eps, latents, hist, saved, row, pag, B, per_sample, z, mask, init, noise) -> int:
    """the shared checks of the two PAG multistep entries -> z_rows"""
    n = B * per_sample
    _req(eps, f"{what}.eps")
    _req(latents, f"{what}.latents")
    _req(hist, f"{what}.hist", torch.float32)
    _req(saved, f"{what}.saved")
    _req(row, f"{what}.row", torch.float32)
    _req_pag(pag, what)
    if eps.numel() != eps_rows * n or latents.numel() != n or hist.numel() != 4 * n or saved.numel() != n or row.numel() != 16:
        raise _lib.CidError(f"{what}: eps / latents / hist / saved / row hold {eps.numel()} / {latents.numel()} / "
                            f"{hist.numel()} / {saved.numel()} / {row.numel()} elements; B * per_sample = {n} needs "
                            f"{eps_rows * n} / {n} / {4 * n} / {n} / 16")
    z_rows = 0
    if z is not None:
        _req(z, f"{what}.z")
        if z.numel() == 0 or z.numel() % n:
            raise _lib.CidError(f"{what}.z: {z.numel()} elements are not rows of B * per_sample = {n}")
        z_rows = z.numel() // n
    _req_step_blend(what, n, mask, init, noise)
    return z_rows


def cfg_pag_multistep_step(eps: torch.Tensor, latents: torch.Tensor, hist: torch.Tensor, saved: torch.Tensor,
                           row: torch.Tensor, guidance: float, pag: torch.Tensor, *, B: int, per_sample: int,
                           z: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                           init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
    """``cfg_multistep_step`` with perturbed-attention guidance (cid_cfg_pag_multistep_step_f16): ``eps`` fp16
    [3B, per_sample] = [uncond | cond | perturbed], ``pag`` as in ``cfg_pag_ddim_step``"""
    z_rows = _pag_multistep("cfg_pag_multistep_step", 3, eps, latents, hist, saved, row, pag, B, per_sample, z, mask, init, noise)
    check(_lib.load().cid_cfg_pag_multistep_step_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row),
                                                     float(guidance), _p(pag), _p(mask), _p(init), _p(noise), B, per_sample,
                                                     _stream()), "cid_cfg_pag_multistep_step_f16")
    return latents


def pag_multistep_step(eps: torch.Tensor, latents: torch.Tensor, hist: torch.Tensor, saved: torch.Tensor, row: torch.Tensor,
                       pag: torch.Tensor, *, B: int, per_sample: int, z: Optional[torch.Tensor] = None,
                       mask: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
                       noise: Optional[torch.Tensor] = None):
    """``multistep_step`` (the single pass) with perturbed-attention guidance (cid_pag_multistep_step_f16): ``eps`` fp16
    [2B, per_sample] = [cond | perturbed], e = c + s (c - p); at s == 0 the bits are ``multistep_step``'s"""
    z_rows = _pag_multistep("pag_multistep_step", 2, eps, latents, hist, saved, row, pag, B, per_sample, z, mask, init, noise)
    check(_lib.load().cid_pag_multistep_step_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row), _p(pag),
                                                 _p(mask), _p(init), _p(noise), B, per_sample, _stream()),
          "cid_pag_multistep_step_f16")
    return latents


def _req_eps_d(eps_d: torch.Tensor, n: int, what: str):
    _req(eps_d, f"{what}.eps_d")
    if eps_d.numel() != n:
        raise _lib.CidError(f"{what}.eps_d: {eps_d.numel()} elements, B * per_sample = {n}")


def cfg_sag_ddim_step(eps: torch.Tensor, latents: torch.Tensor, coef: torch.Tensor, guidance: float, eps_d: torch.Tensor,
                      sag: float, *, B: int, per_sample: int, mask: Optional[torch.Tensor] = None,
                      init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
    """``cfg_ddim_step`` with self-attention guidance (cid_cfg_sag_ddim_step_f16): ``eps`` fp16 [2B, per_sample], ``eps_d``
    fp16 [B, per_sample] the prediction on the degraded latents, e = u + g (c - u) + sag (u - e_d); at sag == 0 ``eps_d`` is
    not read and the bits are ``cfg_ddim_step``'s"""
    lib = _lib.load()
    n = B * per_sample
    _req(eps, "cfg_sag_ddim_step.eps")
    _req(latents, "cfg_sag_ddim_step.latents")
    _req(coef, "cfg_sag_ddim_step.coef", torch.float32)
    _req_eps_d(eps_d, n, "cfg_sag_ddim_step")
    if eps.numel() != 2 * n or latents.numel() != n or coef.numel() < 4:
        raise _lib.CidError(f"cfg_sag_ddim_step: eps / latents / coef hold {eps.numel()} / {latents.numel()} / {coef.numel()} "
                            f"elements; B * per_sample = {n} needs {2 * n} / {n} / at least 4")
    _req_step_blend("cfg_sag_ddim_step", n, mask, init, noise)
    check(lib.cid_cfg_sag_ddim_step_f16(_p(eps), _p(latents), _p(coef), float(guidance), _p(eps_d), float(sag), _p(mask),
                                        _p(init), _p(noise), B, per_sample, _stream()), "cid_cfg_sag_ddim_step_f16")
    return latents


def _sag_multistep(what: str, eps_rows: int, eps, latents, hist, saved, row, eps_d, B, per_sample, z, mask, init, noise) -> int:
    """the shared checks of the two SAG multistep entries -> z_rows"""
    n = B * per_sample
    _req(eps, f"{what}.eps")
    _req(latents, f"{what}.latents")
    _req(hist, f"{what}.hist", torch.float32)
    _req(saved, f"{what}.saved")
    _req(row, f"{what}.row", torch.float32)
    _req_eps_d(eps_d, n, what)
    if eps.numel() != eps_rows * n or latents.numel() != n or hist.numel() != 4 * n or saved.numel() != n or row.numel() != 16:
        raise _lib.CidError(f"{what}: eps / latents / hist / saved / row hold {eps.numel()} / {latents.numel()} / "
                            f"{hist.numel()} / {saved.numel()} / {row.numel()} elements; B * per_sample = {n} needs "
                            f"{eps_rows * n} / {n} / {4 * n} / {n} / 16")
    z_rows = 0
    if z is not None:
        _req(z, f"{what}.z")
        if z.numel() == 0 or z.numel() % n:
            raise _lib.CidError(f"{what}.z: {z.numel()} elements are not rows of B * per_sample = {n}")
        z_rows = z.numel() // n
    _req_step_blend(what, n, mask, init, noise)
    return z_rows


def cfg_sag_multistep_step(eps: torch.Tensor, latents: torch.Tensor, hist: torch.Tensor, saved: torch.Tensor,
                           row: torch.Tensor, guidance: float, eps_d: torch.Tensor, sag: float, *, B: int, per_sample: int,
                           z: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                           init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
    """``cfg_multistep_step`` with self-attention guidance (cid_cfg_sag_multistep_step_f16): ``eps`` fp16 [2B, per_sample],
    ``eps_d`` and ``sag`` as in ``cfg_sag_ddim_step``"""
    z_rows = _sag_multistep("cfg_sag_multistep_step", 2, eps, latents, hist, saved, row, eps_d, B, per_sample, z, mask, init, noise)
    check(_lib.load().cid_cfg_sag_multistep_step_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row),
                                                     float(guidance), _p(eps_d), float(sag), _p(mask), _p(init), _p(noise), B,
                                                     per_sample, _stream()), "cid_cfg_sag_multistep_step_f16")
    return latents


def sag_multistep_step(eps: torch.Tensor, latents: torch.Tensor, hist: torch.Tensor, saved: torch.Tensor, row: torch.Tensor,
                       eps_d: torch.Tensor, sag: float, *, B: int, per_sample: int, z: Optional[torch.Tensor] = None,
                       mask: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
                       noise: Optional[torch.Tensor] = None):
    """``multistep_step`` (the single pass) with self-attention guidance (cid_sag_multistep_step_f16): ``eps`` fp16
    [B, per_sample], e = c + sag (c - e_d); at sag == 0 the bits are ``multistep_step``'s"""
    z_rows = _sag_multistep("sag_multistep_step", 1, eps, latents, hist, saved, row, eps_d, B, per_sample, z, mask, init, noise)
    check(_lib.load().cid_sag_multistep_step_f16(_p(eps), _p(latents), _p(hist), _p(saved), _p(z), z_rows, _p(row), _p(eps_d),
                                                 float(sag), _p(mask), _p(init), _p(noise), B, per_sample, _stream()),
          "cid_sag_multistep_step_f16")
    return latents


def add_inplace(y: torch.Tensor, a: torch.Tensor):
    lib = _lib.load()
    _req(y, "add_inplace.y")
    _req(a, "add_inplace.a")
    if hasattr(y, "_gn_stats"):
        del y._gn_stats              # the epilogue statistics describe the tensor BEFORE this in-place update
    check(lib.cid_add_inplace_f16(_p(y), _p(a), y.numel(), a.numel(), _stream()), "cid_add_inplace_f16")
    return y


def freeu_ws_bytes(B: int, c_skip: int, H: int, W: int) -> int:
    """scratch :func:`freeu` needs for this shape (0 for a shape it refuses); grows with H * W only up to a bound, so
    ``freeu_ws_bytes(B, c, 1024, 1024)`` serves every H x W"""
    return int(_lib.load().cid_freeu_ws_bytes(B, c_skip, H, W))


def freeu(x: torch.Tensor, skip: torch.Tensor, ws: torch.Tensor, *, B: int, H: int, W: int, c_x: int, c_skip: int,
          s: float, b: float, out: Optional[torch.Tensor] = None):
    """FreeU on the two inputs of an up-block resnet (cid.h, cid_freeu_f16): ``x`` fp16 [B * H * W, c_x], its first
    c_x / 2 channels times ``b`` in place; ``skip`` fp16 [B * H * W, c_skip] through diffusers' ``fourier_filter(threshold=1,
    scale=s)`` into ``out`` (default: in place).  ``ws``: >= ``freeu_ws_bytes`` bytes of device scratch.  Two launches,
    deterministic.  Returns the filtered tensor."""
    lib = _lib.load()
    out = skip if out is None else out
    if H < 2 or W < 2:
        raise _lib.CidError(f"freeu: H x W = {H} x {W}; both sides must be at least 2 (the filter's box is empty on a side of 1)")
    if c_x <= 0 or c_x % 16 or c_skip <= 0 or c_skip % 8:
        raise _lib.CidError(f"freeu: c_x = {c_x} must be a positive multiple of 16 and c_skip = {c_skip} of 8")
    if x.numel() != B * H * W * c_x or skip.numel() != B * H * W * c_skip or out.numel() != skip.numel():
        raise _lib.CidError(f"freeu: x / skip / out hold {x.numel()} / {skip.numel()} / {out.numel()} elements; B = {B}, "
                            f"H x W = {H} x {W}, c_x = {c_x}, c_skip = {c_skip}")
    for name, t in (("x", x), ("skip", skip), ("out", out)):
        _req(t, f"freeu.{name}")
        if not t.is_contiguous():
            raise _lib.CidError(f"freeu.{name}: not contiguous")
    if not ws.is_cuda or ws.data_ptr() % 16 or ws.numel() * ws.element_size() < freeu_ws_bytes(B, c_skip, H, W):
        raise _lib.CidError(f"freeu.ws: {freeu_ws_bytes(B, c_skip, H, W)} bytes of 16-byte aligned device scratch needed")
    for t in (x, out):
        if hasattr(t, "_gn_stats"):
            del t._gn_stats          # the epilogue statistics describe the tensor BEFORE this update
    check(lib.cid_freeu_f16(_p(x), c_x, float(b), _p(skip), _p(out), c_skip, float(s), B, H, W, ws.data_ptr(), _stream()),
          "cid_freeu_f16")
    return out


def residual_accum(ys, rs, scales: torch.Tensor):
    """cid_residual_accum_f16: ``ys[j] += sum_k scales[k] * rs[k][j]`` (fp32 sum in net order, one rounding) for up to 16
    destinations and up to 4 nets in ONE launch.  ``rs[k]`` holds net k's residual of every destination -- ``rs[k][j]`` with
    ``ys[j].numel() % rs[k][j].numel() == 0``, the B-row residual repeating under a 2B-row batch -- or is None for a net that
    did not run: its ``scales[k]`` must then be 0 on the device; the kernel does not read the residuals of such a net, and its
    slots carry the destination's own address only because the ABI takes no null.  ``scales``: DEVICE fp32, at least
    ``len(rs)`` values (the launch reads the first ``len(rs)``), so a captured launch follows the step table."""
    lib = _lib.load()
    if not 1 <= len(ys) <= 16 or not 1 <= len(rs) <= _lib.MAX_CONTROLNETS:
        raise _lib.CidError(f"residual_accum: {len(ys)} destinations (1..16), {len(rs)} nets (1..{_lib.MAX_CONTROLNETS})")
    _req(scales, "residual_accum.scales", torch.float32)
    if scales.numel() < len(rs) or not scales.is_contiguous():
        raise _lib.CidError(f"residual_accum.scales: {scales.numel()} values for {len(rs)} nets")
    segs = (_lib.AccumSeg * len(ys))()
    for j, y in enumerate(ys):
        _req(y, f"residual_accum.ys[{j}]")
        if not y.is_contiguous():
            raise _lib.CidError(f"residual_accum.ys[{j}]: not contiguous")
        if hasattr(y, "_gn_stats"):
            del y._gn_stats          # the epilogue statistics describe the tensor BEFORE this in-place update
        segs[j].y, segs[j].n = y.data_ptr(), y.numel()
        nr = None
        for k, net in enumerate(rs):
            if net is None:
                segs[j].r[k] = y.data_ptr()
                continue
            if len(net) != len(ys):
                raise _lib.CidError(f"residual_accum.rs[{k}]: {len(net)} residuals for {len(ys)} destinations")
            r = net[j]
            _req(r, f"residual_accum.rs[{k}][{j}]")
            if not r.is_contiguous() or (nr is not None and r.numel() != nr):
                raise _lib.CidError(f"residual_accum.rs[{k}][{j}]: {r.numel()} elements (contiguous, {nr} like the other nets')")
            nr = r.numel()
            segs[j].r[k] = r.data_ptr()
        segs[j].nr = y.numel() if nr is None else nr
    check(lib.cid_residual_accum_f16(segs, len(ys), len(rs), scales.data_ptr(), _stream()), "cid_residual_accum_f16")
    return ys


class StepTable:
    """Per-step values of one generation as ONE device table + the buffers the captured step reads (cid_step_select):
    ``columns`` = [(destination tensor, per-step values [S, ...] of the same dtype / trailing shape)].  ``select()`` is
    the first launch of a step: row ``counter`` -> destinations, ``counter`` += 1.  The destinations keep their addresses
    (the captured graph stays valid); the table is rebuilt per generation."""

    def __init__(self, columns, device, alloc=None):
        """``alloc(name, tensor, dtype)`` -> a persistent device tensor holding ``tensor`` (the denoise engine's static-buffer
        pool: stable addresses across generations, so a captured step stays valid); default: fresh tensors."""
        # (exceptions, not asserts: the columns are built from run-time tensors, and a mismatch would let cid_step_select copy
        #  the wrong byte ranges into the buffers the captured graph reads -- python -O must not remove the check)
        if not 0 < len(columns) <= 8:
            raise ValueError(f"StepTable takes 1..8 columns (got {len(columns)})")
        S = columns[0][1].shape[0]
        rows, segs, off = [], [], 0
        for j, (dst, vals) in enumerate(columns):
            if vals.dtype != dst.dtype:
                raise TypeError(f"StepTable column {j}: values are {vals.dtype}, the destination is {dst.dtype}")
            if vals.shape[0] != S or vals[0].numel() != dst.numel():
                raise ValueError(f"StepTable column {j}: values {tuple(vals.shape)} do not match {S} rows of the destination "
                                 f"{tuple(dst.shape)}")
            _req(dst, "StepTable.dst", dst.dtype)
            b = vals.to(device).contiguous().view(S, -1).view(torch.uint8)
            if b.shape[1] % 4 != 0:
                raise ValueError(f"StepTable column {j}: {b.shape[1]} bytes per row (columns are multiples of 4 bytes)")
            pad = -b.shape[1] % 16          # columns start on 16-byte boundaries of a 16-byte-multiple row: cid_step_select
            rows.append(b)                  # moves 16 bytes per lane where source and destination allow it
            segs.append((dst, off, b.shape[1]))
            off += b.shape[1] + pad
            if pad:
                rows.append(torch.zeros(S, pad, dtype=torch.uint8, device=b.device))
        table = torch.cat(rows, dim=1).contiguous()
        counter = torch.zeros(1, dtype=torch.int32, device=device)
        self.table = alloc("step_table", table, torch.uint8) if alloc else table
        self.counter = alloc("step_counter", counter, torch.int32) if alloc else counter
        self.n_rows, self.row_bytes = S, off
        self._segs = (_lib.StepSeg * len(segs))(*[_lib.StepSeg(d.data_ptr(), o, n) for d, o, n in segs])
        self._keep = [d for d, _, _ in segs]

    def reset(self, step: int = 0):
        self.counter.fill_(int(step))

    def select(self):
        lib = _lib.load()
        check(lib.cid_step_select(self.table.data_ptr(), self.row_bytes, self.n_rows, self.counter.data_ptr(), self._segs,
                                  len(self._keep), _stream()), "cid_step_select")


# --------------------------------------------------------------------------- fp32 (SDXL VAE decode)
def gemm_f32(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, M: int, N: int, c: int, bias: Optional[torch.Tensor] = None,
             res: Optional[torch.Tensor] = None, taps: int = 1, Hi: int = 0, Wi: int = 0, up: int = 0, ldx: Optional[int] = None,
             ldo: Optional[int] = None, ldr: Optional[int] = None):
    lib = _lib.load()
    for name, t in (("x", x), ("w", w), ("out", out)) + ((("bias", bias),) if bias is not None else ()) \
            + ((("res", res),) if res is not None else ()):
        _req(t, f"gemm_f32.{name}", torch.float32)
    check(lib.cid_gemm_f32(_p(x), _p(w), _p(bias), _p(res), _p(out), M, N, c, taps, ldx if ldx is not None else c,
                           ldo if ldo is not None else N, ldr if ldr is not None else N, Hi, Wi, Hi << up, Wi << up, up,
                           _stream()), "cid_gemm_f32")
    return out


def groupnorm_f32(x: torch.Tensor, out: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, ws: torch.Tensor, *, B: int,
                  HW: int, C_: int, groups: int = 32, eps: float = 1e-6, silu: bool = True):
    lib = _lib.load()
    for name, t in (("x", x), ("out", out), ("gamma", gamma), ("beta", beta)):
        _req(t, f"groupnorm_f32.{name}", torch.float32)
    if ws.numel() * ws.element_size() < int(lib.cid_groupnorm_f32_ws_bytes(B, HW, C_)):
        raise _lib.CidError("groupnorm_f32: workspace too small")
    check(lib.cid_groupnorm_f32(_p(x), _p(out), _p(gamma), _p(beta), B, HW, C_, groups, eps, 1 if silu else 0, ws.data_ptr(),
                                _stream()), "cid_groupnorm_f32")
    return out


def groupnorm_f32_ws_bytes(B: int, HW: int, C_: int) -> int:
    return int(_lib.load().cid_groupnorm_f32_ws_bytes(B, HW, C_))


def softmax_rows_f32(x: torch.Tensor, *, rows: int, cols: int, ld: int):
    lib = _lib.load()
    _req(x, "softmax_rows_f32.x", torch.float32)
    check(lib.cid_softmax_rows_f32(_p(x), rows, cols, ld, _stream()), "cid_softmax_rows_f32")
    return x
