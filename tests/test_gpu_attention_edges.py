"""The attention kernels along the key axis: every first-generation cross-attention instance at general contexts
(`STD = false` of csrc/xattn.hip / xattn_core.h: any n_txt + n_ip <= 96, no ID keys, one key, ID keys on and off a key-tile
boundary), the self-attention kernel at one / three / four key tiles with a ragged, a one-key and wholly masked tiles behind
hostile padding, odd head counts and three different pitches, the causal kernel at one visible key / one tile / a second
query workgroup, and cid_small_attn_f16 at its key-count and wave-count bounds with padded pitches.

Every reference is plain PyTorch in fp64 on the same fp16 inputs (tests/attention_ref.py); outputs are written into
sentinel-filled buffers with guard rows (and guard columns where the ABI takes an output pitch).  Criteria are the suite's own:
check_close(2e-3, 8e-3) for attention against fp64 (test_gpu_ranges.py), check_vs_fp16_arm for the fused processor
(test_gpu_kernels.test_id_cross_attention), the project defaults for cid_small_attn_f16."""
import pytest
import torch

import attention_ref as ar
from conftest import check_close, check_vs_fp16_arm
from test_gpu_kernels import _xattn_weights, rnd
from test_gpu_ranges import _planted_queries

pytestmark = pytest.mark.gpu

ATTN_TOL = dict(tol_l2=2e-3, tol_max=8e-3)
G = ar.GUARD

# ----------------------------------------------------------------------------- A. two-stream cross-attention, general context
XCFG = {      # (C, heads): (tokens per workgroup of its csrc/xattn.hip instance, context width the models pair it with)
    (64, 2): (64, 128), (128, 2): (64, 128), (320, 8): (128, 768), (640, 8): (64, 768), (1280, 8): (32, 768),
    (640, 10): (64, 2048), (1280, 20): (32, 2048),
}
CONTEXTS = [(81, 0),      # ControlNet
            (77, 0),      # text only
            (77, 16),     # 93 keys
            (92, 4),      # all 96 slots used
            (1, 0),       # one key
            (32, 4),      # ID keys start on a key-tile boundary
            (33, 3),      # text crosses the boundary by one
            (5, 1)]
WIDE_CONTEXTS = [(81, 0), (92, 4), (33, 3)]
CORE_CASES = [(C, h, *ctx) for (C, h) in ((64, 2), (128, 2)) for ctx in CONTEXTS] + \
             [(C, h, *ctx) for (C, h) in ((320, 8), (640, 8), (1280, 8), (640, 10), (1280, 20)) for ctx in WIDE_CONTEXTS]
PROPERTY_CONFIGS = [(128, 2), (640, 8), (320, 8)]
KVROW = [2, 0]
B_X, R_X = 2, 3
IP_SCALE = 0.8


def _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip):
    """cid_kv_pack_f16 into sentinel-filled operands: every slot written, every element the index formula's"""
    from consistentid_amd import ops
    ke, ve = ops.kv_pack_elems(C, heads)
    kp, vp = ar.sentinel_like(R_X * ke, dev), ar.sentinel_like(R_X * ve, dev)
    ops.kv_pack(kv_txt.to(dev), kv_ip.to(dev), kp, vp, R=R_X, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip)
    torch.cuda.synchronize()
    what = f"kv_pack C={C} heads={heads} n_txt={n_txt} n_ip={n_ip}"
    assert torch.isfinite(kp.float()).all() and torch.isfinite(vp.float()).all(), f"{what}: slots left unwritten"
    kp_ref, vp_ref = ar.kv_pack_ref(kv_txt, kv_ip, R_X, C, heads, n_txt, n_ip)
    assert torch.equal(kp.cpu().view(R_X, -1), kp_ref), f"{what}: K image differs (padding slots must be zero)"
    assert torch.equal(vp.cpu().view(R_X, -1), vp_ref), f"{what}: V^T image differs (padding slots must be zero)"
    return kp, vp


def _streams(kv_txt, kv_ip, C, heads, n_txt, n_ip):
    """the rows cid_kv_pack_f16 takes, per sample (through KVROW) and head: k_txt, v_txt, k_ip, v_ip [B, n, heads, d]"""
    L, d = n_txt + n_ip, C // heads
    t, i = (x.view(R_X, L, 2 * C)[KVROW] for x in (kv_txt, kv_ip))
    sp = lambda x: x.reshape(B_X, -1, heads, d)
    return sp(t[:, :n_txt, :C]), sp(t[:, :n_txt, C:]), sp(i[:, n_txt:, :C]), sp(i[:, n_txt:, C:])


def _core(dev, q, kp, vp, C, heads, n_txt, n_ip, ip_scale, what):
    """cid_id_xattn_core_f16 twice into guarded outputs: guards intact, second launch bit-identical; returns [B * N, C]"""
    from consistentid_amd import ops
    M = q.shape[0]
    qd, kvrow = q.to(dev), torch.tensor(KVROW, dtype=torch.int32, device=dev)
    bufs = []
    for _ in range(2):
        buf = ar.guarded(M, C, dev)
        ops.id_xattn_core(qd, buf[G:G + M], kp=kp, vp=vp, kvrow=kvrow, B=B_X, N=M // B_X, C_=C, heads=heads, n_txt=n_txt,
                          n_ip=n_ip, ip_scale=ip_scale)
        torch.cuda.synchronize()
        bufs.append(buf)
    ar.guards_intact(bufs[0], M, C, what)
    assert torch.equal(bufs[0].view(torch.int16), bufs[1].view(torch.int16)), f"{what}: the second launch differs"
    return bufs[0][G:G + M]


@pytest.mark.parametrize("C,heads,n_txt,n_ip", CORE_CASES)
def test_xattn_core_general_context(dev, C, heads, n_txt, n_ip):
    """cid_kv_pack_f16 + cid_id_xattn_core_f16 on random fp16 [K | V] rows (no GEMM: the reference reads the same values),
    |score| <~ 20 log2 units, two workgroups per sample, context rows through kvrow"""
    d, L, N = C // heads, n_txt + n_ip, 2 * XCFG[C, heads][0]
    what = f"xattn core n_txt={n_txt} n_ip={n_ip} C={C} d={d}"
    print(f"[case] n_txt={n_txt} n_ip={n_ip} C={C} d={d} (N={N})")
    kv_txt, kv_ip = rnd(R_X * L, 2 * C, seed=C + L), rnd(R_X * L, 2 * C, seed=C + L + 1)
    q = rnd(B_X * N, C, seed=C + L + 2, scale=4.0 * d ** -0.5)
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    out = _core(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, what)
    ref = ar.two_stream_ref(q.view(B_X, N, heads, d), *_streams(kv_txt, kv_ip, C, heads, n_txt, n_ip), IP_SCALE)
    check_close(out, ref.reshape(B_X * N, C), what, **ATTN_TOL)


@pytest.mark.parametrize("n_txt,n_ip", [(77, 16), (33, 3), (92, 4)])
@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_core_zero_ip_scale_is_the_text_context(dev, C, heads, n_txt, n_ip):
    """context (n_txt, n_ip) with ip_scale = 0.0 is bit-identical to context (n_txt, 0) on the same text rows: the ID
    probabilities are multiplied by an exact zero and padding probabilities are zero, so both feed the same P^T.  (Both
    sides are the general instance.  (77, 4) is not in the list: it selects the separately compiled 77 + 4 instance, whose
    output is within an fp16 ulp of the general one's but not bit for bit -- measured 6.1e-5 / 1.2e-4 at outputs of ~0.1.)"""
    d, L, N = C // heads, n_txt + n_ip, 2 * XCFG[C, heads][0]
    kv_txt, kv_ip = rnd(R_X * L, 2 * C, seed=3), rnd(R_X * L, 2 * C, seed=4)
    q = rnd(B_X * N, C, seed=5, scale=4.0 * d ** -0.5)
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    both = _core(dev, q, kp, vp, C, heads, n_txt, n_ip, 0.0, f"ip_scale 0 ({n_txt}, {n_ip}) C={C}")
    txt_rows = kv_txt.view(R_X, L, 2 * C)[:, :n_txt].reshape(R_X * n_txt, 2 * C).contiguous()
    kp0, vp0 = _pack(dev, txt_rows, txt_rows, C, heads, n_txt, 0)
    text = _core(dev, q, kp0, vp0, C, heads, n_txt, 0, IP_SCALE, f"text only ({n_txt}, 0) C={C}")
    assert torch.equal(both.view(torch.int16), text.view(torch.int16)), \
        f"C={C} ({n_txt}, {n_ip}) at ip_scale 0 differs from ({n_txt}, 0): {(both.float() - text.float()).abs().max():.3e}"


@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_core_one_key_returns_its_value_row(dev, C, heads):
    """(1, 0): the softmax of one key is 1.0, so every query gets exactly the fp16 V row of its head"""
    N = 2 * XCFG[C, heads][0]
    kv = rnd(R_X, 2 * C, seed=6)
    q = rnd(B_X * N, C, seed=7, scale=4.0 * (C // heads) ** -0.5)
    kp, vp = _pack(dev, kv, kv, C, heads, 1, 0)
    out = _core(dev, q, kp, vp, C, heads, 1, 0, IP_SCALE, f"one key C={C}")
    want = kv[KVROW, C:].to(dev)[:, None, :].expand(B_X, N, C).reshape(B_X * N, C)
    assert torch.equal(out, want)


@pytest.mark.parametrize("high", ["id", "text", "padding"])
@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_core_streams_far_apart(dev, C, heads, high):
    """the two softmaxes are independent: the scores of one key range lie >= 100 log2 units above the other's (either way
    round, at (33, 3)), or the text scores lie >= 100 below the zero scores of the padding slots (at (33, 0)); neither the
    neighbouring range nor the padding may leak into a range's maximum.  The gap is a condition on the fp64 scores."""
    d, N = C // heads, 2 * XCFG[C, heads][0]
    n_txt, n_ip = (33, 0) if high == "padding" else (33, 3)
    L = n_txt + n_ip
    g = torch.Generator().manual_seed(C + len(high))
    e = torch.zeros(heads, d)
    e[:, :8] = 1.0                                            # common direction of every query and the shifted keys
    e = e.reshape(C)
    q = (torch.randn(B_X * N, C, generator=g) * 0.3 + 2.0 * e).half()
    shift = {"id": (0.0, 12.5), "text": (12.5, 0.0), "padding": (-12.5, 0.0)}[high]     # q . k ~ 2 * 12.5 * 8 = 200
    kv_txt = torch.randn(R_X * L, 2 * C, generator=g)
    kv_ip = torch.randn(R_X * L, 2 * C, generator=g)
    kv_txt[:, :C] = kv_txt[:, :C] * 0.3 + shift[0] * e
    kv_ip[:, :C] = kv_ip[:, :C] * 0.3 + shift[1] * e
    kv_txt, kv_ip = kv_txt.half(), kv_ip.half()
    k_txt, v_txt, k_ip, v_ip = _streams(kv_txt, kv_ip, C, heads, n_txt, n_ip)
    qh = q.view(B_X, N, heads, d)
    s_txt = torch.einsum("bihd,bjhd->bhij", qh.double(), k_txt.double())
    if high == "padding":
        gap = float(-s_txt.max())
    else:
        s_ip = torch.einsum("bihd,bjhd->bhij", qh.double(), k_ip.double())
        lo, hi_ = (s_txt, s_ip) if high == "id" else (s_ip, s_txt)
        gap = float((hi_.amin(-1) - lo.amax(-1)).min())
    print(f"[scores] C={C} d={d} {high} on top: gap {gap:.1f} log2 units")
    assert gap >= 100, f"ranges only {gap:.1f} apart"
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    what = f"xattn core, {high} scores on top, C={C} d={d}"
    out = _core(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, what)
    ref = ar.two_stream_ref(qh, k_txt, v_txt, k_ip, v_ip, IP_SCALE)
    check_close(out, ref.reshape(B_X * N, C), what, **ATTN_TOL)


@pytest.mark.parametrize("ln_res", [False, True])
@pytest.mark.parametrize("n_txt,n_ip", [(81, 0), (33, 3)])
@pytest.mark.parametrize("C,heads", list(XCFG))
def test_id_xattn_fused_general_context(dev, C, heads, n_txt, n_ip, ln_res):
    """cid_id_xattn_f16 (and, for C >= 640, the split path LayerNorm -> GEMM -> core -> GEMM) at a general context, with and
    without LayerNorm + residual, K / V from the projection GEMMs: against the restated processor in fp64, held to the
    same processor in stock fp16 on the GPU"""
    from consistentid_amd import ops
    (BT, Dc), d, L = XCFG[C, heads], C // heads, n_txt + n_ip
    N, M = 2 * BT, 2 * B_X * BT
    what = f"id-xattn n_txt={n_txt} n_ip={n_ip} C={C} d={d} ln+res={ln_res}"
    print(f"[case] n_txt={n_txt} n_ip={n_ip} C={C} d={d} (N={N}, fused)")
    W = _xattn_weights(C, Dc, 8, seed=C + heads)
    x, ehs = rnd(B_X, N, C, seed=1, scale=1.5), rnd(R_X, L, Dc, seed=2)
    ln = ((1 + 0.1 * rnd(C, seed=3).float()).half(), rnd(C, seed=4, scale=0.1)) if ln_res else None
    ref = ar.xattn_block_ref(x, ehs[KVROW], W, heads, n_txt, n_ip, IP_SCALE, ln, ln_res, torch.float64, "cpu")
    arm = ar.xattn_block_ref(x, ehs[KVROW], W, heads, n_txt, n_ip, IP_SCALE, ln, ln_res, torch.float16, dev)
    mq, mk, mv, mo = ar.merged_xattn_weights(W, d)
    wq, wo, bo = mq.half().to(dev).contiguous(), mo.half().to(dev).contiguous(), W["bo"].half().to(dev)
    kv_txt = torch.empty(R_X * L, 2 * C, dtype=torch.float16, device=dev)
    kv_ip = torch.empty(R_X * L, 2 * C, dtype=torch.float16, device=dev)
    ops.gemm(ehs.to(dev), torch.cat([mk, mv]).half().to(dev), kv_txt, M=R_X * L, N=2 * C, c1=Dc)
    ops.gemm(ehs.to(dev), torch.cat([W["kip"], W["vip"]]).half().to(dev), kv_ip, M=R_X * L, N=2 * C, c1=Dc)
    torch.cuda.synchronize()
    kp, vp = _pack(dev, kv_txt.cpu(), kv_ip.cpu(), C, heads, n_txt, n_ip)
    xd, kvrow = x.to(dev), torch.tensor(KVROW, dtype=torch.int32, device=dev)
    g, b = (ln[0].to(dev), ln[1].to(dev)) if ln_res else (None, None)
    buf = ar.guarded(M, C, dev)
    ops.id_xattn(xd, buf[G:G + M], wq=wq, wo=wo, bo=bo, kp=kp, vp=vp, kvrow=kvrow, B=B_X, N=N, C_=C, heads=heads,
                 n_txt=n_txt, n_ip=n_ip, ip_scale=IP_SCALE, residual=xd if ln_res else None, ln_gamma=g, ln_beta=b)
    torch.cuda.synchronize()
    check_vs_fp16_arm(buf[G:G + M].view(B_X, N, C), ref, arm, what)
    ar.guards_intact(buf, M, C, what)
    if ln_res and C >= 640:
        ln2 = torch.empty(M, C, dtype=torch.float16, device=dev)
        ops.layernorm(xd, ln2, g, b, M=M, C_=C)
        q2 = torch.empty(M, C, dtype=torch.float16, device=dev)
        ops.gemm(ln2, wq, q2, M=M, N=C, c1=C)
        o2 = ar.guarded(M, C, dev)
        ops.id_xattn_core(q2, o2[G:G + M], kp=kp, vp=vp, kvrow=kvrow, B=B_X, N=N, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip,
                          ip_scale=IP_SCALE)
        out2 = torch.empty(B_X, N, C, dtype=torch.float16, device=dev)
        ops.gemm(o2[G:G + M], wo, out2, M=M, N=C, c1=C, bias=bo, res=xd, ldr=C)
        torch.cuda.synchronize()
        check_vs_fp16_arm(out2, ref, arm, what + " (split path)")
        ar.guards_intact(o2, M, C, what + " (split path)")


# ----------------------------------------------------------------------------- B. self-attention: tiles, waves, masks, pitches
HEAD_DIMS = [32, 40, 64, 80, 160]
PAD_FILL = 1000.0        # what the columns between a row's end and the pitch hold


def _wide(t, ld, dev):
    """[rows, width] -> the same rows as a view into a [rows, ld] buffer whose other columns hold PAD_FILL"""
    buf = torch.full((t.shape[0], ld), PAD_FILL, dtype=torch.float16)
    buf[:, :t.shape[1]] = t
    return buf.to(dev)[:, :t.shape[1]]


def _self_attn_case(dev, d, N, n_keys, heads, B=2):
    """cid_self_attn_f16 (n_keys == N) / cid_self_attn_keys_f16 with ldq != ldk != ldo, a guarded output, and -- behind
    n_keys -- hostile but finite padding: K rows that outscore every real key by >= 64 log2 units, V^T columns of 60000"""
    from consistentid_amd import ops
    C = heads * d
    ldq, ldk, ldo = C + 8, C + 16, C + 8
    masked = n_keys < N
    what = f"self-attn d={d} N={N} n_keys={n_keys} heads={heads}"
    g = torch.Generator().manual_seed(1000 * d + N + n_keys)
    e = torch.zeros(d)
    e[:8] = 1.0
    q = (torch.randn(B, N, heads, d, generator=g) * 0.3 + e).half()
    k = (torch.randn(B, N, heads, d, generator=g) * 0.3).half()
    v = torch.randn(B, N, heads, d, generator=g).half()
    if masked:
        k[:, n_keys:] = (40.0 * e).half()
        s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())
        real, pad = s[..., :n_keys], s[..., n_keys:]
        gap = float((pad.amax(-1) - real.amax(-1)).min())
        print(f"[scores] {what}: padding above real by >= {gap:.0f}, real |score| <= {float(real.abs().max()):.1f} (log2 units)")
        assert gap >= 64, f"{what}: the padding keys only lead by {gap:.1f}"
    ref = ar.self_attn_ref(q, k, v, n_keys if masked else None).reshape(B * N, C)
    vt = ar.vt_image(v, ops.dvp_of(d), 60000.0, n_keys if masked else None).to(dev)
    qd, kd = _wide(q.reshape(B * N, C), ldq, dev), _wide(k.reshape(B * N, C), ldk, dev)
    buf = ar.guarded(B * N, ldo, dev)
    ops.self_attn(qd, kd, vt, buf[G:G + B * N], B=B, N=N, heads=heads, d=d, ldq=ldq, ldk=ldk, ldo=ldo,
                  n_keys=n_keys if masked else None)
    torch.cuda.synchronize()
    got = buf[G:G + B * N, :C]
    bad = int((~torch.isfinite(got.float())).sum())
    print(f"[finite] {what}: {bad} of {got.numel()} outputs non-finite")
    check_close(got, ref, what, **ATTN_TOL)
    ar.guards_intact(buf, B * N, C, what)


@pytest.mark.parametrize("N", [64, 192])          # one / three key tiles, two waves per workgroup
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_self_attention_tile_counts(dev, d, N):
    _self_attn_case(dev, d, N, N, heads=3)


@pytest.mark.parametrize("N,n_keys", [(64, 1), (64, 31), (64, 63),      # tile 0 itself holds padding
                                      (192, 64), (192, 65),             # two / one key tiles wholly masked
                                      (256, 255)])                      # four waves per workgroup
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_self_attention_masked_hostile_padding(dev, d, N, n_keys):
    _self_attn_case(dev, d, N, n_keys, heads=3)


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_self_attention_masked_with_xcd_remap(dev, d):
    """heads = 4, B = 2, N = 256: 16 workgroups, so the XCD renumbering is active (heads = 3 above never has it)"""
    _self_attn_case(dev, d, 256, 255, heads=4)


# ----------------------------------------------------------------------------- C. causal self-attention
@pytest.mark.parametrize("smax", [None, 50.0])
@pytest.mark.parametrize("N,n_keys", [(64, 1),       # one visible key
                                      (64, 64),      # one tile, one workgroup
                                      (256, 65),     # query workgroups 1 .. 3 stage two tiles, the second one key wide
                                      (256, 200)])   # later query workgroups skip tiles behind n_keys
def test_causal_attention_bounds(dev, N, n_keys, smax):
    """cid_self_attn_causal_f16 with randn logits (smax None) and with |score| up to ~smax log2 units plus planted scores of
    smax on the first and the last visible key; rows below n_keys against fp64, rows beyond finite, one key = its V row"""
    from consistentid_amd import ops
    B, heads, d = 2, 3, 64
    C = heads * d
    what = f"causal attn N={N} n_keys={n_keys} smax={smax}"
    g = torch.Generator().manual_seed(N + n_keys)
    k = torch.randn(B, N, C, generator=g).half()
    q = (torch.randn(B, N, C, generator=g) * (0.125 if smax is None else smax / (4 * d ** 0.5))).half()
    v = torch.randn(B, N, C, generator=g).half()
    if smax is not None:
        last = n_keys - 1
        plants = {last: {0: smax}}
        if last > 0:
            plants[last] = {0: smax, last: smax + 8.5}
            plants[last // 2] = {last // 2: smax}
        for b in range(B):
            for h in range(heads):
                sl = slice(h * d, (h + 1) * d)
                q[b, :, sl] = _planted_queries(q[b, :, sl].clone(), k[b, :, sl], plants)
    qh, kh, vh = (t.view(B, N, heads, d) for t in (q, k, v))
    ref = ar.self_attn_ref(qh, kh, vh, n_keys, causal=True).reshape(B, N, C)
    vt = ar.vt_image(vh, ops.dvp_of(d)).to(dev)
    buf = ar.guarded(B * N, C, dev)
    ops.self_attn_causal(q.to(dev), k.to(dev), vt, buf[G:G + B * N], B=B, N=N, heads=heads, d=d, ldq=C, ldk=C, ldo=C,
                         n_keys=n_keys)
    torch.cuda.synchronize()
    out = buf[G:G + B * N].view(B, N, C)
    assert torch.isfinite(out.float()).all(), "pad query rows must come out finite"
    check_close(out[:, :n_keys], ref[:, :n_keys], what, **ATTN_TOL)
    ar.guards_intact(buf, B * N, C, what)
    if n_keys == 1:
        assert torch.equal(out, v[:, :1].to(dev).expand(B, N, C)), "one visible key: every row is V row 0"


# ----------------------------------------------------------------------------- D. cid_small_attn_f16 at its bounds
@pytest.mark.parametrize("B,Lq,heads", [(1, 1, 1),       # one wave of the launch works, three leave
                                        (3, 5, 1)])      # 15 waves: not a multiple of the four per workgroup
@pytest.mark.parametrize("n1,n2", [(1, 0), (63, 1), (64, 0), (64, 1), (257, 4), (1020, 4)])
def test_small_attn_bounds(dev, lib, n1, n2, B, Lq, heads):
    """through the C ABI with every pitch 8 halfs wider than its rows, (1, 0) without a second key block at all"""
    from consistentid_amd import ops
    from consistentid_amd._lib import check
    inner = heads * 64
    ldq, ldkv, ldo = inner + 8, 2 * inner + 8, inner + 8
    what = f"small_attn n1={n1} n2={n2} B={B} Lq={Lq} heads={heads}"
    g = torch.Generator().manual_seed(n1 + n2 + Lq)
    q = torch.randn(B * Lq, inner, generator=g).half()
    kv1 = torch.randn(B * n1, 2 * inner, generator=g).half()
    kv2 = torch.randn(B * n2, 2 * inner, generator=g).half() if n2 else None
    qd, kv1d = _wide(q, ldq, dev), _wide(kv1, ldkv, dev)
    kv2d = _wide(kv2, ldkv, dev) if n2 else None
    buf = ar.guarded(B * Lq, ldo, dev)
    out = buf[G:G + B * Lq]
    check(lib.cid_small_attn_f16(qd.data_ptr(), ldq, kv1d.data_ptr(), n1, kv2d.data_ptr() if n2 else None, n2, ldkv,
                                 out.data_ptr(), ldo, B, Lq, heads, 64, 64 ** -0.5, ops._stream()), "cid_small_attn_f16")
    torch.cuda.synchronize()
    kv = kv1.double().view(B, n1, -1)
    if n2:
        kv = torch.cat([kv, kv2.double().view(B, n2, -1)], dim=1)
    kk, vv = (t.view(B, n1 + n2, heads, 64).transpose(1, 2) for t in kv.chunk(2, dim=-1))
    s = q.double().view(B, Lq, heads, 64).transpose(1, 2) @ kk.transpose(-1, -2) / 8.0
    ref = (torch.softmax(s, dim=-1) @ vv).transpose(1, 2).reshape(B * Lq, inner)
    check_close(out[:, :inner], ref, what)
    ar.guards_intact(buf, B * Lq, inner, what)
    if n1 + n2 == 1:
        want = kv1.view(B, 1, 2 * inner)[:, :, inner:].expand(B, Lq, inner).reshape(B * Lq, inner)
        assert torch.equal(out[:, :inner].cpu(), want), "one key: every query gets its V row"
