"""The HIP kernels across the input range, not only at randn scale: GELU / GEGLU over every finite fp16 value, the
normalizations at large mean / std ratios and on constant rows / groups, softmax and attention at wide logit ranges.
Every reference is computed in fp64 from the same fp16 (fp32) inputs; the criteria are the ones of the neighbouring tests
in test_gpu_kernels.py / test_gpu_vae.py, or stricter."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_close, check_vs_fp16_arm
from test_gpu_kernels import _xattn_reference, _xattn_weights, rnd

pytestmark = pytest.mark.gpu

RATIOS = [8, 32, 64, 128]                  # mean / std of a row or group
CONSTS = [0.0, 1.0, -37.5, 100.0]          # values of the constant rows / groups mixed into the same launch
TOL32 = dict(tol_l2=5e-5, tol_max=5e-4)    # test_gpu_vae.py: fp32 kernels


def _finite_fp16():
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    h = h[torch.isfinite(h)]
    assert h.numel() == 63488
    return h


def _assert_within_ulp16(got, ref64, what):
    """every element of the fp16 result finite and within one fp16 ulp of the fp64 reference rounded to fp16, plus 1e-6:
    about twice the absolute error of the fp32 formula itself (<= 5.8e-7, tools/fit_gelu.py), which is several fp16 ulps in
    the far negative tail (gelu(-4.2) = -5.6e-5 has an ulp of 6e-8)"""
    got = got.detach().cpu().float().numpy().astype(np.float64)
    r16 = ref64.detach().cpu().double().numpy().astype(np.float16).astype(np.float64)
    ulp = np.where(r16 == 0, 2.0 ** -24, np.ldexp(1.0, np.maximum(np.frexp(np.abs(r16))[1] - 11, -24)))
    err = np.abs(got - r16)
    bad = ~np.isfinite(got) | (err > ulp + 1e-6)
    print(f"[parity] {what}: {got.size} values, max err {np.nanmax(err):.2e}, max err / ulp {np.nanmax(err / ulp):.2f}, "
          f"{int(bad.sum())} bad")
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        raise AssertionError(f"{what}: {int(bad.sum())} values off by more than one fp16 ulp + 1e-6, first: got {got.ravel()[i]!r}, "
                             f"want {r16.ravel()[i]!r}")


# ----------------------------------------------------------------------------- GELU / GEGLU over every fp16 value
def test_gelu_every_fp16_value(dev):
    h = _finite_fp16()
    y = h.to(dev).clone()
    from consistentid_amd import ops
    ops.gelu_(y)
    torch.cuda.synchronize()
    _assert_within_ulp16(y, F.gelu(h.double()), "gelu_ over every finite fp16 value")


def _routes_to_linear_h32(M, C):
    """The planner's rule for the GEGLU launch of linear_h32.hip (gemm_plan.hip, route_linear_h32): one source,
    no LayerNorm fold, N % 160 == 0, M % 256 == 0, at least 16 channel slabs of 64, >= 256 tiles of 256 x 160.  The library
    has no query for the kernel it picked, so the tests assert the route through this mirror of the rule.
    Keep in sync with route_linear_h32 in consistentid_amd/csrc/gemm_plan.hip; CID_GEGLU_H32=0 turns it off."""
    N = 8 * C
    return N % 160 == 0 and M % 256 == 0 and C // 64 >= 16 and (M // 256) * (N // 160) >= 256


@pytest.mark.parametrize("M,C,h32", [(2048, 1280, True),      # linear_h32.hip
                                     (2048 + 64, 1280, False),  # same channels, rows off the 256 grid: igemm mode 1
                                     (320 + 64, 320, False)])   # igemm mode 1 at K = 320
def test_geglu_every_fp16_gate(dev, M, C, h32):
    """One-hot rows (x[m, m % C] = 1), value half of W = 1, no bias: out[m, n] = gelu(W_gate[n, m % C]) exactly in fp32.
    Every finite fp16 value sits somewhere in W_gate (zero padding elsewhere)."""
    from consistentid_amd import ops, weights
    assert _routes_to_linear_h32(M, C) == h32
    assert M >= C and 4 * C * C >= 63488
    x = torch.zeros(M, C, dtype=torch.float16)
    x[torch.arange(M), torch.arange(M) % C] = 1
    wg = torch.zeros(4 * C * C, dtype=torch.float16)
    wg[:63488] = _finite_fp16()[torch.randperm(63488, generator=torch.Generator().manual_seed(C))]
    wg = wg.view(4 * C, C)
    w = torch.cat([torch.ones(4 * C, C, dtype=torch.float16), wg])
    out = torch.full((M, 4 * C), float("nan"), dtype=torch.float16, device=dev)
    ops.gemm(x.to(dev), weights._geglu_interleave(w).contiguous().to(dev), out, M=M, N=8 * C, c1=C, mode=1)
    torch.cuda.synchronize()
    ref = F.gelu(wg.double().T[torch.arange(M) % C])
    _assert_within_ulp16(out, ref, f"GEGLU ({'linear_h32' if h32 else 'igemm mode 1'}) M={M} C={C}, every fp16 gate")


def test_layernorm_folded_geglu_large_gates(dev):
    """The LayerNorm-folded GEGLU (igemm mode 1 with ln): the large gate values come through the folded bias ln_b, the gate
    weights are small and the value half is exactly 1 (zero weights, bias 1)."""
    from consistentid_amd import ops, weights
    M, C = 512, 320
    big = torch.tensor([0, 8, 12, 20, 25.5, 25.7, 26, 30, 100, 1000, 30000, 65504], dtype=torch.float64)
    listed = torch.cat([big, -big[1:]])
    gates = torch.cat([listed, torch.linspace(-64, 64, 4 * C - listed.numel(), dtype=torch.float64)])
    gates = gates.half().float()
    x = rnd(M, C, seed=1)
    wv, wg = torch.zeros(4 * C, C), rnd(4 * C, C, seed=2, scale=1e-3).float()
    w = torch.cat([wv, wg])
    bias = torch.cat([torch.ones(4 * C), gates])
    g, be = torch.ones(C, dtype=torch.float16), torch.zeros(C, dtype=torch.float16)
    wi, bi = weights._geglu_interleave(w), weights._geglu_interleave(bias)
    wl, s_, b_ = weights.fold_ln(wi.to(dev), g.to(dev), be.to(dev), bi.to(dev))
    out = torch.full((M, 4 * C), float("nan"), dtype=torch.float16, device=dev)
    ops.gemm(x.to(dev), wl, out, M=M, N=8 * C, c1=C, mode=1, ln=(s_.view(torch.float32), b_.view(torch.float32), 1e-5))
    torch.cuda.synchronize()
    ln = F.layer_norm(x.double(), (C,), eps=1e-5)
    gate = ln @ wg.half().double().T + gates.double()
    ref = F.gelu(gate)
    got = out.double().cpu()
    assert torch.isfinite(got).all(), "LN-folded GEGLU: non-finite output"
    err = ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    print(f"[parity] LN-folded GEGLU, gates up to 65504: max err / max(1, |ref|) = {err:.3e}")
    assert err <= 2e-3, err
    check_close(out, ref, "LN-folded GEGLU, large gates")


# ----------------------------------------------------------------------------- normalizations at large offsets
def _rows_with_offsets(M, C, ratio, seed, std=1.0):
    """rows of std `std` and mean ±ratio * std (sign alternating per row); every 16th row constant at one of CONSTS"""
    x = rnd(M, C, seed=seed).float() * std
    sign = 1.0 - 2.0 * (torch.arange(M) % 2).float()
    x = x + (ratio * std * sign)[:, None]
    for i, r in enumerate(range(3, M, 16)):
        x[r] = CONSTS[i % len(CONSTS)]
    return x.half()


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("M,C", [(1000, 320), (32768, 320)])     # one row per wave / several rows per wave
def test_layernorm_offsets_and_constant_rows(dev, M, C, ratio):
    from consistentid_amd import ops
    x = _rows_with_offsets(M, C, ratio, seed=1)
    g, b = (1 + 0.1 * rnd(C, seed=2).float()).half(), rnd(C, seed=3, scale=0.1)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    out = torch.empty(M, C, dtype=torch.float16, device=dev)
    ops.layernorm(x.to(dev), out, g.to(dev), b.to(dev), M=M, C_=C)
    torch.cuda.synchronize()
    check_close(out, ref, f"layernorm {M}x{C} mean/std={ratio}")


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("M,C,mode,heads", [(2048, 320, 0, 0), (512, 1280, 0, 0), (2048, 320, 1, 0), (2 * 1024, 320, 2, 8)])
def test_gemm_layernorm_fold_offsets(dev, M, C, mode, heads, ratio):
    """test_gemm_layernorm_fold's check on rows of mean / std = ratio, with constant rows in the same launch (their LayerNorm
    is exactly beta: the output is the beta path W beta + bias)"""
    from consistentid_amd import ops, weights
    x = _rows_with_offsets(M, C, ratio, seed=1)
    g, be = (1 + 0.2 * rnd(C, seed=2).float()).half(), rnd(C, seed=3, scale=0.2)
    N = {0: C, 1: 8 * C, 2: 3 * C}[mode]
    w = rnd(N, C, seed=4, scale=C ** -0.5)
    bias = rnd(N, seed=5, scale=0.3) if mode != 2 else None
    lin = F.layer_norm(x.double(), (C,), g.double(), be.double(), 1e-5) @ w.double().T + (bias.double() if bias is not None else 0)
    xh = x.to(dev)
    linh = F.layer_norm(xh, (C,), g.to(dev), be.to(dev), 1e-5) @ w.to(dev).T + (bias.to(dev) if bias is not None else 0)
    what = f"M={M} C={C} mean/std={ratio}"
    if mode == 1:
        wi, bi = weights._geglu_interleave(w.float()), weights._geglu_interleave(bias.float())
        wl, s_, b_ = weights.fold_ln(wi.to(dev), g.to(dev), be.to(dev), bi.to(dev))
        out = torch.empty(M, 4 * C, dtype=torch.float16, device=dev)
        ops.gemm(xh, wl, out, M=M, N=N, c1=C, mode=1, ln=(s_.view(torch.float32), b_.view(torch.float32), 1e-5))
        torch.cuda.synchronize()
        h_, gate = lin.chunk(2, -1)
        ha, ga = linh.chunk(2, -1)
        check_vs_fp16_arm(out, h_ * F.gelu(gate), ha * F.gelu(ga), f"LN-folded GEGLU {what}")
        return
    wl, s_, b_ = weights.fold_ln(w.float().to(dev), g.to(dev), be.to(dev), bias.to(dev) if bias is not None else None)
    lnp = (s_.view(torch.float32), b_.view(torch.float32), 1e-5)
    if mode == 0:
        out = torch.empty(M, N, dtype=torch.float16, device=dev)
        ops.gemm(xh, wl, out, M=M, N=N, c1=C, ln=lnp)
        torch.cuda.synchronize()
        check_vs_fp16_arm(out, lin, linh, f"LN-folded linear {what}")
        return
    d = C // heads
    B, Ntok = 2, M // 2
    qk = torch.empty(M, 2 * C, dtype=torch.float16, device=dev)
    vt = torch.zeros(B * heads * ops.dvp_of(d) * Ntok, dtype=torch.float16, device=dev)
    ops.gemm(xh, wl, qk, M=M, N=N, c1=C, mode=2, vt=vt, n_vt0=2 * C, heads=heads, dhead=d, ntok=Ntok, ln=lnp)
    torch.cuda.synchronize()
    check_vs_fp16_arm(qk, lin[:, :2 * C], linh[:, :2 * C], f"LN-folded q/k projection {what}")
    v = lin[:, 2 * C:].reshape(B, Ntok, heads, d).transpose(1, 2)
    va = linh[:, 2 * C:].reshape(B, Ntok, heads, d).transpose(1, 2)
    t = torch.arange(Ntok)
    pos = (t & ~15) | (8 * ((t >> 2) & 1) + 4 * ((t >> 3) & 1) + (t & 3))
    got_v = vt.reshape(B, heads, ops.dvp_of(d), Ntok)[:, :, :d, :].cpu()[..., pos].transpose(-1, -2)
    check_vs_fp16_arm(got_v, v, va, f"LN-folded v^T image {what}")


def _run_xattn3(dev, x, ehs, W, ln, residual, B, N, n_ip):
    """cid_id_xattn3_f16 as test_id_cross_attention_v3 drives it; returns (out, fp32 reference, stock fp16 arm)"""
    from consistentid_amd import ops, xattn_pack
    from consistentid_amd.weights import LOG2E
    C, heads, Dc, L, ip_scale = 320, 8, 768, 81, 0.8
    n_txt = L - n_ip
    kvrow = torch.tensor([(i + 1) % (B + 1) for i in range(B)], dtype=torch.int32)
    ref = _xattn_reference(x, ehs[kvrow.long()], W, heads, n_ip, ip_scale, ln, residual=residual)
    arm = _xattn_reference(x, ehs[kvrow.long()], W, heads, n_ip, ip_scale, ln, residual=residual, arm_device=dev)
    d = C // heads
    mq = (W["q"] + W["q_up"] @ W["q_down"]) * (d ** -0.5 * LOG2E)
    mk, mv = W["k"] + W["k_up"] @ W["k_down"], W["v"] + W["v_up"] @ W["v_down"]
    mo = W["o"] + W["out_up"] @ W["out_down"]
    R = B + 1
    kv_txt = torch.empty(R * L, 2 * C, dtype=torch.float16, device=dev)
    kv_ip = torch.empty(R * L, 2 * C, dtype=torch.float16, device=dev)
    e = ehs.to(dev)
    ops.gemm(e, torch.cat([mk, mv]).half().to(dev), kv_txt, M=R * L, N=2 * C, c1=Dc)
    ops.gemm(e, torch.cat([W["kip"], W["vip"]]).half().to(dev), kv_ip, M=R * L, N=2 * C, c1=Dc)
    ke, ve = ops.kv_pack2_elems(C, heads)
    kp = torch.empty(R * ke, dtype=torch.float16, device=dev)
    vp = torch.empty(R * ve, dtype=torch.float16, device=dev)
    ops.kv_pack2(kv_txt, kv_ip, kp, vp, R=R, L=L, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip, order="reg")
    wq_f, qs, qb = xattn_pack.fold_layernorm(mq.to(dev), ln[0].to(dev) if ln else None, ln[1].to(dev) if ln else None)
    wq_p, wo_p = xattn_pack.pack_w3(wq_f), xattn_pack.pack_w3(mo.half().to(dev).contiguous())
    out = torch.full((B, N, C), float("nan"), dtype=torch.float16, device=dev)
    ops.id_xattn3(x.to(dev), out, wq_p=wq_p, q_rowsum=qs, q_bias=qb, wo_p=wo_p, bo=W["bo"].half().to(dev),
                  kp=kp, vp=vp, kvrow=kvrow.to(dev), B=B, N=N, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip,
                  ip_scale=ip_scale, has_ln=ln is not None, add_residual=residual)
    torch.cuda.synchronize()
    return out, ref, arm


@pytest.mark.parametrize("ratio", RATIOS)
def test_id_xattn3_layernorm_offsets(dev, ratio):
    """cid_id_xattn3_f16 with has_ln (statistics traded through LDS) on rows of mean / std = ratio and constant rows; the
    criterion of test_id_cross_attention_v3"""
    B, N, n_ip, C = 3, 64, 4, 320
    W = _xattn_weights(C, 768, 8, seed=C + 8)
    x = _rows_with_offsets(B * N, C, ratio, seed=1, std=1.5).view(B, N, C)
    ln = ((1 + 0.1 * rnd(C, seed=3).float()).half(), rnd(C, seed=4, scale=0.1))
    out, ref, arm = _run_xattn3(dev, x, rnd(B + 1, 81, 768, seed=2), W, ln, True, B, N, n_ip)
    check_vs_fp16_arm(out, ref, arm, f"id-xattn3 LN mean/std={ratio}")


@pytest.mark.parametrize("high", ["text", "id"])
def test_id_xattn3_streams_far_apart(dev, high):
    """the two-stream (text / ID) softmax of cid_id_xattn3_f16 with one stream's logits ~100 above the other's: the key
    weights of the high stream are scaled until the median gap of the per-query maxima is ~100 (natural units)"""
    B, N, n_ip, C, heads, L = 2, 128, 4, 320, 8, 81
    n_txt, d = L - n_ip, C // heads
    W = _xattn_weights(C, 768, 8, seed=C + 8)
    x = rnd(B, N, C, seed=1, scale=1.5)
    ehs = rnd(B + 1, L, 768, seed=2)
    ln = ((1 + 0.1 * rnd(C, seed=3).float()).half(), rnd(C, seed=4, scale=0.1))
    kvrow = torch.tensor([(i + 1) % (B + 1) for i in range(B)])
    e = ehs[kvrow].double()

    def maxima(W):
        q = F.layer_norm(x.double(), (C,), ln[0].double(), ln[1].double(), 1e-5) @ (W["q"] + W["q_up"] @ W["q_down"]).double().T
        kt = e[:, :n_txt] @ (W["k"] + W["k_up"] @ W["k_down"]).double().T
        ki = e[:, n_txt:] @ W["kip"].double().T
        sc = lambda k: torch.einsum("bnhd,bkhd->bnhk", q.view(B, N, heads, d), k.view(B, -1, heads, d)) / d ** 0.5
        return sc(kt).amax(-1), sc(ki).amax(-1)

    mt, mi = maxima(W)
    hi, lo = (mt, mi) if high == "text" else (mi, mt)
    alpha = float((100 + lo.median()) / hi.median())
    for name in (("k", "k_up") if high == "text" else ("kip",)):
        W[name] = (W[name] * alpha).half().float()
    mt, mi = maxima(W)
    gap = float(((mt - mi) if high == "text" else (mi - mt)).median())
    assert 70 <= gap <= 130, f"median gap {gap:.1f}"
    out, ref, arm = _run_xattn3(dev, x, ehs, W, ln, False, B, N, n_ip)
    check_vs_fp16_arm(out, ref, arm, f"id-xattn3, {high} stream ~{gap:.0f} above")


def _groups_with_offsets(B, HW, C, ratio, seed, std=1.0, dtype=torch.float16):
    """[B, HW, C], 32 groups: each (sample, group) slice has std `std` and mean ±ratio * std; four slices constant"""
    x = torch.randn(B, HW, C, generator=torch.Generator().manual_seed(seed)) * std
    cg = C // 32
    sign = torch.tensor([1.0 if (b + g) % 2 == 0 else -1.0 for b in range(B) for g in range(32)]).view(B, 1, 32, 1)
    x = (x.view(B, HW, 32, cg) + ratio * std * sign).view(B, HW, C)
    for i, v in enumerate(CONSTS):
        b, g = i % B, 5 + 7 * i
        x[b, :, g * cg:(g + 1) * cg] = v
    return x.to(dtype)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("B,HW,C1,C2", [(2, 4096, 320, 0),        # statistics partials + fold (two launches)
                                        (8, 256, 1280, 1280),     # single-launch path (a slice in one workgroup's registers)
                                        (8, 1024, 640, 0)])       # ... its largest slice
def test_groupnorm_offsets_and_constant_groups(dev, B, HW, C1, C2, ratio):
    from consistentid_amd import ops
    C = C1 + C2
    x = _groups_with_offsets(B, HW, C, ratio, seed=1)
    x1, x2 = x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None)
    g, b = (1 + 0.1 * rnd(C, seed=3).float()).half(), rnd(C, seed=4, scale=0.1)
    ref = F.silu(F.group_norm(x.double().transpose(1, 2), 32, g.double(), b.double(), 1e-5)).transpose(1, 2)
    out = torch.empty(B * HW, C, dtype=torch.float16, device=dev)
    ws = torch.zeros(ops.groupnorm_ws_bytes(B, C), dtype=torch.uint8, device=dev)
    ops.groupnorm(x1.to(dev), out, g.to(dev), b.to(dev), ws, B=B, HW=HW, c1=C1, x2=x2.to(dev) if C2 else None,
                  c2=C2, groups=32, eps=1e-5, silu=True)
    torch.cuda.synchronize()
    check_close(out.reshape(B, HW, C), ref, f"groupnorm B{B} HW{HW} C{C1}+{C2} mean/std={ratio}")


@pytest.mark.parametrize("ratio", RATIOS)
def test_groupnorm_on_epilogue_statistics_offsets(dev, ratio):
    """statistics emitted by the GEMM epilogue (test_gemm_emits_groupnorm_statistics) on a conv output with a large bias:
    every group's mean is ±ratio x its std; two groups are constant (zero weights, equal bias)"""
    from consistentid_amd import ops
    B, C, H = 8, 640, 32
    HW, M, cg = H * H, B * H * H, 640 // 32
    x, res = rnd(M, C, seed=1), rnd(M, C, seed=5)
    w = rnd(C, C, seed=3, scale=C ** -0.5)
    sign = torch.tensor([1.0 if g % 2 == 0 else -1.0 for g in range(32)]).repeat_interleave(cg)
    bias = ratio * 2 ** 0.5 * sign + 0.1 * rnd(C, seed=4).float()      # conv output + residual: std ~ sqrt(2)
    constant = ((6, 100.0), (11, -37.5))
    for g, v in constant:
        w[g * cg:(g + 1) * cg] = 0
        res[:, g * cg:(g + 1) * cg] = 0
        bias[g * cg:(g + 1) * cg] = v
    bias = bias.half()
    out = torch.empty(M, C, dtype=torch.float16, device=dev)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    ops.gemm(x.to(dev), w.to(dev), out, M=M, N=C, c1=C, bias=bias.to(dev), res=res.to(dev), ldr=C, ws=ws, gn_hw=HW)
    torch.cuda.synchronize()
    assert hasattr(out, "_gn_stats"), "this launch was expected to emit statistics"
    o = out.double().cpu().reshape(B, HW, C)
    gs = o.reshape(B, HW, 32, cg)
    ratio_seen = gs.mean((1, 3)).abs() / gs.std((1, 3)).clamp_min(1e-30)
    assert float(ratio_seen.median()) >= 0.8 * ratio                 # the offset really is in the tensor
    assert all((gs[:, :, g] == v).all() for g, v in constant)
    g, be = (1 + 0.1 * rnd(C, seed=6).float()).half(), rnd(C, seed=7, scale=0.1)
    ref = F.silu(F.group_norm(o.transpose(1, 2), 32, g.double(), be.double(), 1e-5)).transpose(1, 2)
    gws = torch.zeros(ops.groupnorm_ws_bytes(B, C), dtype=torch.uint8, device=dev)
    y = torch.empty_like(out)
    ops.groupnorm(out, y, g.to(dev), be.to(dev), gws, B=B, HW=HW, c1=C, groups=32, eps=1e-5, silu=True)
    torch.cuda.synchronize()
    check_close(y.reshape(B, HW, C), ref, f"GroupNorm on epilogue statistics mean/std={ratio}")


@pytest.mark.parametrize("ratio", [8, 128, 1000])
def test_groupnorm_f32_offsets(dev, ratio):
    from consistentid_amd import ops
    B, HW, C = 2, 300, 128
    x = _groups_with_offsets(B, HW, C, ratio, seed=4, std=3.0, dtype=torch.float32)
    gen = torch.Generator().manual_seed(5)
    gm, bt = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    ref = F.silu(F.group_norm(x.double().transpose(1, 2), 32, gm.double(), bt.double(), 1e-6)).transpose(1, 2)
    out = torch.empty(B * HW, C, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.groupnorm_f32_ws_bytes(B, HW, C), dtype=torch.uint8, device=dev)
    ops.groupnorm_f32(x.reshape(-1, C).to(dev), out, gm.to(dev), bt.to(dev), ws, B=B, HW=HW, C_=C)
    torch.cuda.synchronize()
    check_close(out.view(B, HW, C), ref, f"groupnorm_f32 + SiLU mean/std={ratio}", **TOL32)


# ----------------------------------------------------------------------------- softmax / attention at wide logit ranges
def _wide_softmax_rows(rows, cols, pad, dtype):
    """log2-unit rows: dominant entry first / last / last before the pad, constant rows, a [-60000, 60000] ramp, scale 100"""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(rows, cols + pad, generator=g) * 4
    x[0:3, 0] = 60.0
    x[3:6, cols - 1] = 60.0
    x[6:9, cols + pad - 1] = 1e4 if pad else 60.0      # beyond `cols`: the untouched pad must not count
    for i, v in enumerate(CONSTS + [-60000.0, 60000.0]):
        x[9 + i, :cols] = v
    x[15] = torch.linspace(-60000, 60000, cols + pad)
    x[16] = torch.linspace(60000, -60000, cols + pad)
    x[17:] = torch.randn(rows - 17, cols + pad, generator=g) * 100
    return x.to(dtype), list(range(9, 15))


def test_softmax_rows_wide_range(dev):
    from consistentid_amd import ops
    rows, cols, pad = 40, 256, 8
    x, const_rows = _wide_softmax_rows(rows, cols, pad, torch.float16)
    y = x.to(dev).clone()
    ops.softmax_rows(y, rows=rows, cols=cols, ld=cols + pad)
    torch.cuda.synchronize()
    ref = torch.softmax(x[:, :cols].double() * np.log(2.0), dim=-1)
    check_close(y[:, :cols], ref, "softmax_rows, wide range")
    assert torch.equal(y[:, cols:].cpu(), x[:, cols:])
    assert (y[const_rows, :cols].cpu().double() == 1.0 / cols).all(), "constant rows must give exactly 1 / cols"


def test_softmax_rows_f32_wide_range(dev):
    from consistentid_amd import ops
    rows, cols, pad = 40, 1024, 16
    x, const_rows = _wide_softmax_rows(rows, cols, pad, torch.float32)
    y = x.to(dev).clone()
    ops.softmax_rows_f32(y, rows=rows, cols=cols, ld=cols + pad)
    torch.cuda.synchronize()
    ref = torch.softmax(x[:, :cols].double() * np.log(2.0), dim=-1)
    check_close(y[:, :cols], ref, "softmax_rows_f32, wide range", **TOL32)
    assert torch.equal(y[:, cols:].cpu(), x[:, cols:])
    assert (y[const_rows, :cols].cpu().double() == 1.0 / cols).all(), "constant rows must give exactly 1 / cols"


def _planted_queries(q, k, plants):
    """q[i] <- the combination of k[j] rows that gives the scores s_j (log2 units) against them: plants = {i: {j: s_j}}"""
    for i, js in plants.items():
        kj = torch.stack([k[j].double() for j in js])
        coef = torch.linalg.solve(kj @ kj.T, torch.tensor(list(js.values()), dtype=torch.float64))
        q[i] = (coef @ kj).to(q.dtype)
    return q


@pytest.mark.parametrize("smax", [50.0, 500.0, 4000.0])
@pytest.mark.parametrize("d,n_keys", [(40, 320), (64, 320), (160, 320), (40, 257), (64, 257)])
def test_self_attention_wide_logits(dev, d, n_keys, smax):
    """ops.self_attn (d = 40: the BIAS path with an fp16 running max) with scores up to ~smax in log2 units: dominant keys in
    the first and the last key tile and in the ragged tail (n_keys = 257: the MASK path, a planted score above everything in
    the padding must not count), and rows whose max rises by just under and just over 8 in a later tile."""
    from consistentid_amd import ops
    B, heads, N = 1, 2, 320
    C = heads * d
    g = torch.Generator().manual_seed(d + n_keys)
    k = torch.randn(N, C, generator=g).half()
    q = (torch.randn(N, C, generator=g) * (smax / (4 * d ** 0.5))).half()
    v = torch.randn(N, C, generator=g).half()
    last = n_keys - 1
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        plants = {0: {5: smax}, 1: {last - 40: smax}, 2: {last: smax}, 5: {70: smax, last: smax + 8.5},
                  6: {40: smax, 250: smax - 20}}
        if smax == 50.0:        # where the fp16 rounding of q moves a score by ~0.03: the rise stays on its side of 8
            plants.update({3: {10: smax, 200: smax + 7.8}, 4: {10: smax, 200: smax + 8.2}})
        if n_keys < N:
            plants[7] = {20: smax, N - 1: smax + 100}          # a padding key: masked, whatever its score
        qh = _planted_queries(q[:, sl].clone(), k[:, sl], plants)
        q[:, sl] = qh
    kd, qd, vd = k.double().view(N, heads, d), q.double().view(N, heads, d), v.double().view(N, heads, d)
    s = torch.einsum("ihd,jhd->hij", qd, kd)
    s[:, :, n_keys:] = -float("inf")
    if smax == 50.0:            # realized rise of the running max at key tile 3, from the fp16 q actually used
        rise = s[:, [3, 4], 192:256].amax(-1) - s[:, [3, 4], :192].amax(-1)
        assert (rise[:, 0] > 7.5).all() and (rise[:, 0] < 8).all() and (rise[:, 1] > 8).all() and (rise[:, 1] < 8.5).all(), rise
    print(f"[scores] d={d} n_keys={n_keys}: largest |score| {s[torch.isfinite(s)].abs().max():.1f} (log2 units)")
    ref = torch.einsum("hij,jhd->ihd", torch.softmax(s * np.log(2.0), -1), vd).reshape(N, C)
    t = torch.arange(N)
    pos = (t & ~15) | (8 * ((t >> 2) & 1) + 4 * ((t >> 3) & 1) + (t & 3))
    dvp = ops.dvp_of(d)
    vt = torch.zeros(B, heads, dvp, N, dtype=torch.float16)
    vt[0, :, :d][..., pos] = v.view(N, heads, d).permute(1, 2, 0)
    out = torch.full((N, C), float("nan"), dtype=torch.float16, device=dev)
    ops.self_attn(q.to(dev), k.to(dev), vt.to(dev), out, B=B, N=N, heads=heads, d=d, ldq=C, ldk=C, ldo=C,
                  n_keys=n_keys if n_keys != N else None)
    torch.cuda.synchronize()
    check_close(out, ref, f"self-attn d={d} n_keys={n_keys} scores ~{smax}", tol_l2=2e-3, tol_max=8e-3)


@pytest.mark.parametrize("high", ["first", "second"])
def test_small_attn_streams_far_apart(dev, high):
    """ops.small_attn over two key streams whose logits are ~100 apart (natural units), either stream on top"""
    from consistentid_amd import ops
    B, Lq, n1, n2, H = 2, 4, 257, 4, 3
    g = torch.Generator().manual_seed(11)
    e = torch.zeros(H * 64)
    e[::2] = 1.0                                            # common direction of every query and the high stream's keys
    q = (torch.randn(B * Lq, H * 64, generator=g) * 0.3 + 2.0 * e).half()
    k_hi = lambda n: torch.randn(B * n, H * 64, generator=g) * 0.3 + 12.5 * e       # q . k / 8 ~ 2 * 12.5 * 32 / 8 = 100
    k_lo = lambda n: torch.randn(B * n, H * 64, generator=g) * 0.3
    k1, k2 = (k_hi(n1), k_lo(n2)) if high == "first" else (k_lo(n1), k_hi(n2))
    kv1 = torch.cat([k1, torch.randn(B * n1, H * 64, generator=g)], -1).half()
    kv2 = torch.cat([k2, torch.randn(B * n2, H * 64, generator=g)], -1).half()
    out = torch.empty(B * Lq, H * 64, dtype=torch.float16, device=dev)
    ops.small_attn(q.to(dev), kv1.to(dev), kv2.to(dev), out, B=B, Lq=Lq, n1=n1, n2=n2, heads=H)
    torch.cuda.synchronize()
    qd = q.double().view(B, Lq, H, 64).transpose(1, 2)
    kv = torch.cat([kv1.double().view(B, n1, -1), kv2.double().view(B, n2, -1)], dim=1)
    kk, vv = kv.chunk(2, dim=-1)
    kk, vv = kk.view(B, n1 + n2, H, 64).transpose(1, 2), vv.view(B, n1 + n2, H, 64).transpose(1, 2)
    s = qd @ kk.transpose(-1, -2) / 8.0
    gap = (s[..., :n1].max(-1).values - s[..., n1:].max(-1).values).abs().min().item()
    assert gap >= 60, f"streams only {gap:.1f} apart"
    ref = (torch.softmax(s, dim=-1) @ vv).transpose(1, 2).reshape(B * Lq, H * 64)
    check_close(out, ref, f"small_attn, {high} stream ~100 above")
