"""The long-context two-stream cross-attention core (csrc/xattn_long.hip: cid_kv_pack_long_f16 + cid_id_xattn_long_f16) past
the 96 key slots of the register-resident kernels: every head width at contexts on and off a key-tile boundary, with and
without ID keys, one key, 32 ID keys; the properties of tests/test_gpu_attention_edges.py carried over (ip_scale 0, one
key, scores planted >= 100 log2 units apart between text tiles, between the streams and below the padding's zeros); and
agreement with cid_id_xattn_core_f16 at (77, 4), which both take.

As test_xattn_core_general_context: B = 2 samples on R = 3 context rows through KVROW = [2, 0], N = 64 tokens (two token
tiles), random fp16 [K | V] rows (no GEMM: the fp64 reference reads the same values), the packed images compared element for
element with the numpy model (tests/long_attention_ref.py) in sentinel-filled buffers, the output written twice into
guarded buffers (guards intact, second launch bit-identical) and held to attention_ref.two_stream_ref at ATTN_TOL.

The same harness on other geometries (``_case``): at the caps (1024 text rows, 32 ID rows, a last text tile of one key, the
pack beyond its 2048-block grid) and on grids whose (sample, head, 32 tokens) units do not fill the last workgroup."""
import pytest
import torch

import attention_ref as ar
import long_attention_ref as lr
from conftest import check_close
from test_gpu_attention_edges import ATTN_TOL, _core
from test_gpu_kernels import rnd

pytestmark = pytest.mark.gpu

G = ar.GUARD
KVROW = [2, 0]
B_X, R_X, N_X = 2, 3, 64
IP_SCALE = 0.8
SMALL = [(64, 2), (128, 2)]                                                   # head widths 32, 64
WIDE = [(320, 8), (640, 8), (1280, 8), (640, 10), (1280, 20)]                 # 40, 80, 160, 64, 64
CONTEXTS = [(93, 4),      # the first context past the old cap
            (97, 0),
            (128, 4),     # text ends on a tile boundary
            (129, 3),     # the last text tile holds one key
            (154, 4), (231, 4),
            (231, 32),    # a full ID tile
            (235, 0),
            (1, 0),       # one key
            (77, 4)]      # the reference's context: cid_id_xattn_core_f16 takes it too
WIDE_CONTEXTS = [(154, 4), (129, 3), (235, 0)]
CASES = [(C, h, *ctx) for (C, h) in SMALL for ctx in CONTEXTS] + [(C, h, *ctx) for (C, h) in WIDE for ctx in WIDE_CONTEXTS]
PROPERTY_CONFIGS = [(128, 2), (640, 8), (320, 8)]


def _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip, R_X=R_X):
    """cid_kv_pack_long_f16 into sentinel-filled operands: every slot written, every element the model's"""
    from consistentid_amd import ops
    ke, ve = ops.kv_pack_long_elems(C, heads, n_txt, n_ip)
    assert (ke, ve) == lr.long_elems(C, heads, n_txt, n_ip)
    kp, vp = ar.sentinel_like(R_X * ke, dev), ar.sentinel_like(R_X * ve, dev)
    ops.kv_pack_long(kv_txt.to(dev), kv_ip.to(dev), kp, vp, R=R_X, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip)
    torch.cuda.synchronize()
    what = f"kv_pack_long C={C} heads={heads} n_txt={n_txt} n_ip={n_ip}"
    assert torch.isfinite(kp.float()).all() and torch.isfinite(vp.float()).all(), f"{what}: slots left unwritten"
    kp_ref, vp_ref = lr.kv_pack_long_ref(kv_txt, kv_ip, R_X, C, heads, n_txt, n_ip)
    assert torch.equal(kp.cpu().view(R_X, -1), kp_ref), f"{what}: K image differs (padding slots must be zero)"
    assert torch.equal(vp.cpu().view(R_X, -1), vp_ref), f"{what}: V^T image differs (padding slots must be zero)"
    return kp, vp


def _streams(kv_txt, kv_ip, C, heads, n_txt, n_ip, B_X=B_X, R_X=R_X, KVROW=KVROW):
    """the rows the pack takes, per sample (through KVROW) and head: k_txt, v_txt, k_ip, v_ip [B, n, heads, d]"""
    L, d = n_txt + n_ip, C // heads
    t, i = (x.view(R_X, L, 2 * C)[KVROW] for x in (kv_txt, kv_ip))
    sp = lambda x: x.reshape(B_X, -1, heads, d)
    return sp(t[:, :n_txt, :C]), sp(t[:, :n_txt, C:]), sp(i[:, n_txt:, :C]), sp(i[:, n_txt:, C:])


def _long(dev, q, kp, vp, C, heads, n_txt, n_ip, ip_scale, what, B_X=B_X, KVROW=KVROW):
    """cid_id_xattn_long_f16 twice into guarded outputs: guards intact, second launch bit-identical; returns [B * N, C]"""
    from consistentid_amd import ops
    M = q.shape[0]
    qd, kvrow = q.to(dev), torch.tensor(KVROW, dtype=torch.int32, device=dev)
    bufs = []
    for _ in range(2):
        buf = ar.guarded(M, C, dev)
        ops.id_xattn_long(qd, buf[G:G + M], kp=kp, vp=vp, kvrow=kvrow, B=B_X, N=M // B_X, C_=C, heads=heads, n_txt=n_txt,
                          n_ip=n_ip, ip_scale=ip_scale)
        torch.cuda.synchronize()
        bufs.append(buf)
    ar.guards_intact(bufs[0], M, C, what)
    assert torch.equal(bufs[0].view(torch.int16), bufs[1].view(torch.int16)), f"{what}: the second launch differs"
    return bufs[0][G:G + M]


@pytest.mark.parametrize("C,heads,n_txt,n_ip", CASES)
def test_xattn_long_contexts(dev, C, heads, n_txt, n_ip):
    d, L = C // heads, n_txt + n_ip
    what = f"xattn long n_txt={n_txt} n_ip={n_ip} C={C} d={d}"
    print(f"[case] n_txt={n_txt} n_ip={n_ip} C={C} d={d} (N={N_X}, key tiles {lr.tiles(n_txt, n_ip)})")
    kv_txt, kv_ip = rnd(R_X * L, 2 * C, seed=C + L), rnd(R_X * L, 2 * C, seed=C + L + 1)
    q = rnd(B_X * N_X, C, seed=C + L + 2, scale=4.0 * d ** -0.5)
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    out = _long(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, what)
    ref = ar.two_stream_ref(q.view(B_X, N_X, heads, d), *_streams(kv_txt, kv_ip, C, heads, n_txt, n_ip), IP_SCALE)
    check_close(out, ref.reshape(B_X * N_X, C), what, **ATTN_TOL)


def _case(dev, C, heads, n_txt, n_ip, B, N, R, kvrow, what):
    """one geometry through the module's harness: the pack against the numpy model in sentinel-filled buffers, the core twice
    into guarded buffers, the fp64 two-stream reference at ATTN_TOL"""
    d, L = C // heads, n_txt + n_ip
    print(f"[case] {what}: B={B} N={N} R={R} kvrow={kvrow}, {lr.units(B, heads, N)} units in {lr.core_blocks(B, heads, N)} "
          f"workgroups of {lr.XL_WAVES}, key tiles {lr.tiles(n_txt, n_ip)}, pack blocks "
          f"{lr.pack_blocks(*lr.long_elems(C, heads, n_txt, n_ip), R)} (grid cap {lr.PACK_GRID_CAP})")
    kv_txt, kv_ip = rnd(R * L, 2 * C, seed=C + L), rnd(R * L, 2 * C, seed=C + L + 1)
    q = rnd(B * N, C, seed=C + L + 2, scale=4.0 * d ** -0.5)
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip, R)
    out = _long(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, what, B, kvrow)
    ref = ar.two_stream_ref(q.view(B, N, heads, d), *_streams(kv_txt, kv_ip, C, heads, n_txt, n_ip, B, R, kvrow), IP_SCALE)
    return check_close(out, ref.reshape(B * N, C), what, **ATTN_TOL)


# The caps: 1024 text rows (cid_xattn_long_max_txt) -- the key loop runs 32 tiles, the packed images are 33 tiles deep with ID
# rows -- at ten K fragments per tile (d = 160) and at two (d = 32); (993, 4): the 32nd text tile holds ONE key; (1056, 0): the
# longest text stream without ID rows (a ControlNet's view of 1024 + up to 32 rows), 33 text tiles.  At 1280 channels on
# R = 2 context rows the pack has more chunks than its 2048-block grid covers in one pass: the grid-stride loop runs.
CAP_CONFIGS = [(1280, 8, 2, [1, 0]), (64, 2, R_X, KVROW)]          # (C, heads, R, kvrow)
CAP_CONTEXTS = [(1024, 32), (1024, 0), (993, 4), (1056, 0)]


@pytest.mark.parametrize("n_txt,n_ip", CAP_CONTEXTS)
@pytest.mark.parametrize("C,heads,R,kvrow", CAP_CONFIGS, ids=lambda v: str(v).replace(" ", ""))
def test_xattn_long_at_the_caps(dev, C, heads, R, kvrow, n_txt, n_ip):
    from consistentid_amd import ops
    cap = ops.xattn_long_max_txt()
    assert n_txt in (cap, cap - 31, cap + ops.XATTN_LONG_MAX_IP) and lr.tiles(n_txt, n_ip)[1] in (32, 33)
    if C == 1280:
        blocks = lr.pack_blocks(*ops.kv_pack_long_elems(C, heads, n_txt, n_ip), R)
        assert blocks > lr.PACK_GRID_CAP, f"{blocks} blocks: the pack's grid-stride loop would not run"
    _case(dev, C, heads, n_txt, n_ip, B_X, N_X, R, kvrow, f"xattn long at the cap n_txt={n_txt} n_ip={n_ip} C={C} d={C // heads}")


# Ragged grids: a unit is (sample, head, 32 tokens), a workgroup runs four.  Where the units are no multiple of four the last
# workgroup's idle waves must leave (``u >= units``): their unit index lies behind the last sample, so what they would write
# are the rows behind the output -- the guards.  R = B + 1 context rows through a selector that is no identity (and repeats
# a row where B > 1).
RAGGED = [(1, 32, 64, 2),       # 2 units: half a workgroup
          (1, 96, 640, 10),     # 30 units: the last workgroup half full, three token tiles
          (3, 32, 320, 8),      # 24 units: one token tile per sample
          (5, 160, 128, 2)]     # 50 units


@pytest.mark.parametrize("n_txt,n_ip", [(154, 4), (129, 0)])
@pytest.mark.parametrize("B,N,C,heads", RAGGED)
def test_xattn_long_ragged_grids(dev, B, N, C, heads, n_txt, n_ip):
    units = lr.units(B, heads, N)
    assert units == {(1, 32): 2, (1, 96): 30, (3, 32): 24, (5, 160): 50}[(B, N)]
    assert units % lr.XL_WAVES or N == 32, "every workgroup would be full and every sample have two token tiles"
    kvrow = [B - i for i in range(B)]
    if B > 1:
        kvrow[-1] = kvrow[0]
    _case(dev, C, heads, n_txt, n_ip, B, N, B + 1, kvrow, f"xattn long ragged B={B} N={N} C={C} d={C // heads} ({n_txt}, {n_ip})")


@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_long_zero_ip_scale_is_the_text_context(dev, C, heads):
    """(154, 4) at ip_scale = 0.0 is bit-identical to (154, 0) on the same text rows"""
    n_txt, n_ip = 154, 4
    d, L = C // heads, n_txt + n_ip
    kv_txt, kv_ip = rnd(R_X * L, 2 * C, seed=3), rnd(R_X * L, 2 * C, seed=4)
    q = rnd(B_X * N_X, C, seed=5, scale=4.0 * d ** -0.5)
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    both = _long(dev, q, kp, vp, C, heads, n_txt, n_ip, 0.0, f"ip_scale 0 ({n_txt}, {n_ip}) C={C}")
    txt_rows = kv_txt.view(R_X, L, 2 * C)[:, :n_txt].reshape(R_X * n_txt, 2 * C).contiguous()
    kp0, vp0 = _pack(dev, txt_rows, txt_rows, C, heads, n_txt, 0)
    text = _long(dev, q, kp0, vp0, C, heads, n_txt, 0, IP_SCALE, f"text only ({n_txt}, 0) C={C}")
    assert torch.equal(both.view(torch.int16), text.view(torch.int16)), \
        f"C={C} ({n_txt}, {n_ip}) at ip_scale 0 differs from ({n_txt}, 0): {(both.float() - text.float()).abs().max():.3e}"
    # ... and the ID stream is there when it is switched on
    on = _long(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, f"ip_scale {IP_SCALE} C={C}")
    assert not torch.equal(on, both)


@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_long_one_key_returns_its_value_row(dev, C, heads):
    """(1, 0): the softmax of one key is 1.0, so every query gets exactly the fp16 V row of its head"""
    kv = rnd(R_X, 2 * C, seed=6)
    q = rnd(B_X * N_X, C, seed=7, scale=4.0 * (C // heads) ** -0.5)
    kp, vp = _pack(dev, kv, kv, C, heads, 1, 0)
    out = _long(dev, q, kp, vp, C, heads, 1, 0, IP_SCALE, f"one key C={C}")
    want = kv[KVROW, C:].to(dev)[:, None, :].expand(B_X, N_X, C).reshape(B_X * N_X, C)
    assert torch.equal(out, want)


STEP = 8.0        # shift of the planted key direction per level: q . k moves by ~ 2 * 8 * STEP = 128 log2 units


@pytest.mark.parametrize("plan", ["tiles rising", "tiles falling", "id above", "id below", "padding above"])
@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_long_scores_far_apart(dev, C, heads, plan):
    """the online softmax across text tiles and the independence of the two streams: the scores of text tile t + 1 lie
    >= 100 log2 units above those of tile t (the running maximum rises in every tile and the accumulator is rescaled by
    2^-100) or below them (every later tile underflows against the first); the ID scores lie >= 100 above / below the text
    scores; at (129, 0) the text scores lie >= 100 below the zero scores of the 31 padding slots of the last tile.  Every
    gap is asserted on the fp64 scores."""
    _far_apart(dev, C, heads, plan, *((129, 0) if plan == "padding above" else (154, 4)))


def test_xattn_long_scores_far_apart_at_the_cap(dev):
    """"tiles rising" over the 32 text tiles of (1024, 4): the running maximum rises, and the accumulator is rescaled by
    <= 2^-100, 31 times in a row; what is left is the last tile's softmax (head width 80)"""
    from consistentid_amd import ops
    _far_apart(dev, 640, 8, "tiles rising", ops.xattn_long_max_txt(), 4)


def _far_apart(dev, C, heads, plan, n_txt, n_ip):
    d = C // heads
    L = n_txt + n_ip
    g = torch.Generator().manual_seed(C + len(plan))
    e = torch.zeros(heads, d)
    e[:, :8] = 1.0                                            # common direction of every query and the shifted keys
    e = e.reshape(C)
    q = (torch.randn(B_X * N_X, C, generator=g) * 0.1 + 2.0 * e).half()
    tile = torch.arange(n_txt) // 32                          # 0 .. 4 (0 .. 31 at the cap)
    level = {"tiles rising": tile.float(), "tiles falling": (tile.max() - tile).float(), "id above": torch.zeros(n_txt),
             "id below": torch.ones(n_txt), "padding above": -torch.ones(n_txt)}[plan]
    ip_level = {"id above": 1.0, "id below": 0.0}.get(plan, 0.0)
    kv_txt = torch.randn(R_X, L, 2 * C, generator=g)
    kv_ip = torch.randn(R_X, L, 2 * C, generator=g)
    kv_txt[:, :n_txt, :C] = kv_txt[:, :n_txt, :C] * 0.3 + STEP * level[None, :, None] * e
    kv_ip[:, :, :C] = kv_ip[:, :, :C] * 0.3 + STEP * ip_level * e
    kv_txt, kv_ip = kv_txt.half().view(R_X * L, 2 * C), kv_ip.half().view(R_X * L, 2 * C)
    k_txt, v_txt, k_ip, v_ip = _streams(kv_txt, kv_ip, C, heads, n_txt, n_ip)
    qh = q.view(B_X, N_X, heads, d)
    s_txt = torch.einsum("bihd,bjhd->bhij", qh.double(), k_txt.double())
    if plan.startswith("tiles"):
        per_tile = [s_txt[..., tile == t] for t in range(int(tile.max()) + 1)]
        pairs = zip(per_tile[:-1], per_tile[1:]) if plan == "tiles rising" else zip(per_tile[1:], per_tile[:-1])
        gap = min(float((hi_.amin(-1) - lo.amax(-1)).min()) for lo, hi_ in pairs)
    elif plan == "padding above":
        gap = float(-s_txt.max())
    else:
        s_ip = torch.einsum("bihd,bjhd->bhij", qh.double(), k_ip.double())
        lo, hi_ = (s_txt, s_ip) if plan == "id above" else (s_ip, s_txt)
        gap = float((hi_.amin(-1) - lo.amax(-1)).min())
    print(f"[scores] C={C} d={d} {plan}: gap {gap:.1f} log2 units, |score| <= {float(s_txt.abs().max()):.0f}")
    assert gap >= 100, f"{plan}: only {gap:.1f} apart"
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    what = f"xattn long, {plan}, C={C} d={d}"
    out = _long(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, what)
    ref = ar.two_stream_ref(qh, k_txt, v_txt, k_ip, v_ip, IP_SCALE)
    check_close(out, ref.reshape(B_X * N_X, C), what, **ATTN_TOL)


@pytest.mark.parametrize("C,heads", PROPERTY_CONFIGS)
def test_xattn_long_agrees_with_the_core_at_77_4(dev, C, heads):
    """(77, 4) is in both kernels' range: the long entry against cid_id_xattn_core_f16 (the separately compiled 77 + 4
    instance of csrc/xattn.hip) on the same rows, N = 256 (a multiple of every instance's token tile)"""
    from consistentid_amd import ops
    n_txt, n_ip, N = 77, 4, 256
    d, L = C // heads, n_txt + n_ip
    kv_txt, kv_ip = rnd(R_X * L, 2 * C, seed=11), rnd(R_X * L, 2 * C, seed=12)
    q = rnd(B_X * N, C, seed=13, scale=4.0 * d ** -0.5)
    kp, vp = _pack(dev, kv_txt, kv_ip, C, heads, n_txt, n_ip)
    long_out = _long(dev, q, kp, vp, C, heads, n_txt, n_ip, IP_SCALE, f"long (77, 4) C={C}")
    ke, ve = ops.kv_pack_elems(C, heads)
    kp1 = torch.empty(R_X * ke, dtype=torch.float16, device=dev)
    vp1 = torch.empty(R_X * ve, dtype=torch.float16, device=dev)
    ops.kv_pack(kv_txt.to(dev), kv_ip.to(dev), kp1, vp1, R=R_X, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip)
    core_out = _core(dev, q, kp1, vp1, C, heads, n_txt, n_ip, IP_SCALE, f"core (77, 4) C={C}")
    check_close(long_out, core_out, f"long vs core at (77, 4), C={C} d={d}", **ATTN_TOL)
