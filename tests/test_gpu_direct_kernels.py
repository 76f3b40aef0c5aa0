"""The direct (non-GEMM) kernels of csrc/misc.hip, csrc/norm.hip and csrc/f32.hip at their shape and grid-cap edges.

Every case: fp16-representable inputs from a seeded generator, the same operation in fp64 on the CPU as the reference, the
output in a sentinel-filled buffer with guard rows in front and behind (guard columns where the launch takes a pitch), guards
bit-untouched afterwards, and a second launch bit-identical to the first (every kernel here has a fixed reduction order).
fp16 kernels are held to conftest.check_close's defaults, fp32 kernels to test_gpu_vae.TOL32.

The shapes are the smallest that reach the code in question; the grid caps they depend on (a change of a cap moves the
shape of section A with it):

    conv_in            512 blocks x 32 pixels             conv3x3_small   8192 blocks x 256 (pixel, channel octet) items
    conv_out          2048 blocks x 64 pixels             gelu / quick_gelu / text_embed   4096 blocks x 256 x 8 halfs
    cfg_ddim_step / cfg_multistep_step   1024 x 256 x 8   add_inplace     2048 blocks x 256 x 8 halfs
    residual_accum    2048 tiles of 256 x 8 halfs

Checked before writing section A: cfg_multistep_step already runs past its cap (test_gpu_multistep's BIG = 8 * 262403 halfs,
plain and inpaint, six rows that read, write, save, restore and add z) and residual_accum past its 2048 tiles
(test_gpu_multicontrolnet.test_residual_accum_more_tiles_than_the_grid, two segments, nr = n / 2), so neither has a row
here.  text_embed had no direct case at all -- the CLIP towers launch it at a few hundred rows -- and has both rows.

One shape is refused by a host check and is asserted as that refusal: add_inplace at n = 4 194 304 + 40 with na = n / 2 (the
half is not a multiple of 8); its neighbour n = 4 194 304 + 48 runs past the cap instead."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_close
from gemm_parity import GUARD, SENTINEL
from test_gpu_vae import TOL32

pytestmark = pytest.mark.gpu

SENT32 = 0x7fc5a5a5      # an fp32 NaN with a payload
PAD = 64                 # sentinel elements in front of and behind a flat output
LN2 = float(np.log(2.0))


# ----------------------------------------------------------------------------- helpers
def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def _sent(dtype):
    return (torch.int16, SENTINEL) if dtype == torch.float16 else (torch.int32, SENT32)


def _bits(t):
    return t.view(_sent(t.dtype)[0])


def _guarded(rows, ld, dev, dtype=torch.float16):
    """[GUARD + rows + GUARD, ld], every element the sentinel (GUARD rows keep row 0 16-byte aligned at any pitch)"""
    it, s = _sent(dtype)
    return torch.full(((rows + 2 * GUARD) * ld,), s, dtype=it, device=dev).view(dtype).view(rows + 2 * GUARD, ld)


def _intact(buf, rows, c0, width, what):
    """everything outside rows [GUARD, GUARD + rows) x columns [c0, c0 + width) still holds the sentinel"""
    b, s = _bits(buf), _sent(buf.dtype)[1]
    assert bool((b[:GUARD] == s).all()), f"{what}: rows in front of row 0 were written"
    assert bool((b[GUARD + rows:] == s).all()), f"{what}: rows behind the last row were written"
    assert bool((b[GUARD:GUARD + rows, :c0] == s).all()), f"{what}: columns in front of the block were written"
    assert bool((b[GUARD:GUARD + rows, c0 + width:] == s).all()), f"{what}: columns beyond the width were written"


def _flat(n, dev, dtype=torch.float16):
    it, s = _sent(dtype)
    return torch.full((n + 2 * PAD,), s, dtype=it, device=dev).view(dtype)


def _flat_intact(buf, n, what):
    b, s = _bits(buf), _sent(buf.dtype)[1]
    assert bool((b[:PAD] == s).all()) and bool((b[PAD + n:] == s).all()), f"{what}: elements outside the output were written"


def _twice(launch, what):
    """launch() -> the freshly filled buffer of one launch; the second launch must repeat the first bit for bit"""
    a = launch()
    b = launch()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b)), f"{what}: the second launch differs"
    return a


def _tok(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _wtap(w):
    """[cout, cin, 3, 3] -> the kernels' [cout][tap][cin]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def _wide(t, ld, dev, c0=0):
    """rows of ``t`` at pitch ``ld`` from column ``c0`` of a NaN-filled device buffer: a read outside a row's values poisons
    the result.  -> (the buffer, the [rows, width] view the launch is given)"""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=dev)
    buf[:, c0:c0 + t.shape[1]] = t.to(dev)
    return buf, buf[:, c0:c0 + t.shape[1]]


# ----------------------------------------------------------------------------- conv_in (sections A and D)
def _conv_in_case(dev, what, cin1, cin2, scale, cout, B, Bin, H, W, seed):
    from consistentid_amd import ops
    cin = cin1 + cin2
    s1 = _rnd(Bin, cin1, H, W, seed=seed)
    s2 = _rnd(Bin, cin2, H, W, seed=seed + 1) if cin2 else None
    w, b = _rnd(cout, cin, 3, 3, seed=seed + 2, scale=(9 * cin) ** -0.5), _rnd(cout, seed=seed + 3)
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32)
    x = s1.double() * (float(sc[0]) if sc is not None else 1.0)         # the scale multiplies the first source only
    if cin2:
        x = torch.cat([x, s2.double()], dim=1)
    ref = _tok(F.conv2d(x, w.double(), b.double(), padding=1))          # [Bin * H * W, cout]
    ref = ref.repeat(B // Bin, 1)                                       # batch row b reads sample b % Bin
    s1d, s2d, wd, bd = s1.to(dev), (s2.to(dev) if cin2 else None), _wtap(w).to(dev), b.to(dev)
    scd = sc.to(dev) if sc is not None else None
    M = B * H * W

    def launch():
        buf = _guarded(M, cout, dev)
        ops.conv_in(s1d, buf[GUARD:GUARD + M], wd, bd, B=B, Bin=Bin, cin=cin, H=H, W=W, cout=cout, in_scale=scd, extra=s2d)
        return buf
    buf = _twice(launch, what)
    out = buf[GUARD:GUARD + M]
    check_close(out, ref, what)
    _intact(buf, M, 0, cout, what)
    per = Bin * H * W
    for r in range(1, B // Bin):                                         # the rows that share a sample are stored copies
        assert torch.equal(out[r * per:(r + 1) * per], out[:per]), f"{what}: copy {r} of the shared rows differs"


@pytest.mark.parametrize("cin,H,W", [(4, 130, 127), (9, 130, 127),      # 16 510 pixels: a second trip with a ragged tail
                                     (4, 128, 128)])                    # 16 384: the cap exactly, no second trip
def test_conv_in_past_the_grid_cap(dev, cin, H, W):
    _conv_in_case(dev, f"A conv_in cin={cin} {H}x{W}", cin, 0, None, 64, 2, 1, H, W, seed=10 + cin)


_COUTS, _BATCHES, _IMAGES = (8, 64, 320), ((2, 2), (6, 2)), ((1, 40), (40, 1), (3, 3), (5, 7))
_SPLITS = [(c1, c2, sc) for (c1, c2) in ((1, 8), (3, 5), (5, 4), (4, 4), (2, 1)) for sc in (None, 0.37)] \
    + [(c, 0, sc) for c, sc in ((1, None), (3, 0.37), (7, None), (8, 0.37))]
CONV_IN_CASES = [(c1, c2, sc, _COUTS[i % 3], *_BATCHES[(i // 3 + i) % 2], *_IMAGES[i % 4]) for i, (c1, c2, sc) in enumerate(_SPLITS)]


@pytest.mark.parametrize("cin1,cin2,scale,cout,B,Bin,H,W", CONV_IN_CASES)
def test_conv_in_generic_splits(dev, cin1, cin2, scale, cout, B, Bin, H, W):
    """the runtime-split instance (odd pair counts, zeroed second halves of an odd K1 / K2), cout below the 256 staging
    threads, rep = 1 and 3, one-row and one-column images"""
    _conv_in_case(dev, f"D conv_in {cin1}+{cin2} scale={scale} cout={cout} B={B}/{Bin} {H}x{W}", cin1, cin2, scale, cout, B, Bin,
                  H, W, seed=100 + 10 * cin1 + cin2)


def test_conv_in_cases_cover_every_value():
    """(no GPU needed, but it belongs to the table above) every cout, batch pair and image of section D is in the table"""
    assert {c[3] for c in CONV_IN_CASES} == set(_COUTS)
    assert {c[4:6] for c in CONV_IN_CASES} == set(_BATCHES)
    assert {c[6:8] for c in CONV_IN_CASES} == set(_IMAGES)


# ----------------------------------------------------------------------------- conv3x3_small (A and E)
def _conv_small_case(dev, what, B, Hi, Wi, cin, cout, stride, silu, seed):
    from consistentid_amd import ops
    x, w, b = _rnd(B, cin, Hi, Wi, seed=seed), _rnd(cout, cin, 3, 3, seed=seed + 1, scale=(9 * cin) ** -0.5), _rnd(cout, seed=seed + 2)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1, stride=stride)
    if silu:
        ref = F.silu(ref)
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    assert tuple(ref.shape[-2:]) == (Ho, Wo)
    M = B * Ho * Wo
    xd, wd, bd = _tok(x).to(dev), _wtap(w).to(dev), b.to(dev)

    def launch():
        buf = _guarded(M, cout, dev)
        ops.conv3x3_small(xd, buf[GUARD:GUARD + M], wd, bd, B=B, Hi=Hi, Wi=Wi, cin=cin, cout=cout, stride=stride, silu=silu)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + M], _tok(ref), what)
    _intact(buf, M, 0, cout, what)


@pytest.mark.parametrize("Hi,Wi,cout,stride", [(420, 419, 96, 1),      # 2 111 760 items against 2 097 152: ragged second trip
                                               (840, 837, 96, 2),      # the same output from a stride-2 input
                                               (512, 256, 128, 1)])    # 2 097 152 items: the cap exactly
def test_conv3x3_small_past_the_grid_cap(dev, Hi, Wi, cout, stride):
    _conv_small_case(dev, f"A conv3x3_small {Hi}x{Wi} cout={cout} s{stride}", 1, Hi, Wi, 3, cout, stride, False, seed=20)


@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("Hi,Wi,cin,cout,stride", [(5, 6, 12, 16, 1),       # cin % 4 == 0 but not % 8: the scalar path
                                                   (6, 5, 8, 8, 1),         # the VAE encoder's second call; one channel octet
                                                   (7, 10, 3, 8, 2), (10, 7, 3, 16, 2),     # stride 2, odd x even and even x odd
                                                   (7, 10, 8, 8, 2),
                                                   (1, 1, 12, 8, 1), (1, 9, 8, 16, 1), (1, 9, 3, 8, 2)])
def test_conv3x3_small_edges(dev, Hi, Wi, cin, cout, stride, silu):
    _conv_small_case(dev, f"E conv3x3_small {Hi}x{Wi} {cin}->{cout} s{stride} silu={silu}", 2, Hi, Wi, cin, cout, stride, silu,
                     seed=30 + cin)


# ----------------------------------------------------------------------------- conv_out (A)
@pytest.mark.parametrize("H,W", [(368, 361),       # 132 848 pixels against 2048 x 64 = 131 072
                                 (512, 256)])      # the cap exactly
def test_conv_out_past_the_grid_cap(dev, H, W):
    """cin = 8 is one 16-byte chunk: seven of the eight lanes of a pixel group add zeros"""
    from consistentid_amd import ops
    what = f"A conv_out {H}x{W}"
    cin, cout = 8, 3
    x, w, b = _rnd(1, cin, H, W, seed=41), _rnd(cout, cin, 3, 3, seed=42, scale=(9 * cin) ** -0.5), _rnd(cout, seed=43)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    xd, wd, bd = _tok(x).to(dev), _wtap(w).to(dev), b.to(dev)
    n = cout * H * W

    def launch():
        buf = _flat(n, dev)
        ops.conv_out(xd, buf[PAD:PAD + n], wd, bd, B=1, H=H, W=W, cin=cin, cout=cout)
        return buf
    buf = _twice(launch, what)
    check_close(buf[PAD:PAD + n].view(1, cout, H, W), ref, what)
    _flat_intact(buf, n, what)


# ----------------------------------------------------------------------------- element-wise kernels (A)
CAP_4096 = 4096 * 256 * 8


@pytest.mark.parametrize("n", [CAP_4096 + 8 * 777, CAP_4096], ids=["past", "at_cap"])
@pytest.mark.parametrize("op", ["gelu_", "quick_gelu_"])
def test_gelu_past_the_grid_cap(dev, op, n):
    from consistentid_amd import ops
    what = f"A {op} n={n}"
    x = _rnd(n, seed=51, scale=3.0)
    xd = x.double()
    ref = F.gelu(xd) if op == "gelu_" else xd * torch.sigmoid(1.702 * xd)
    src = x.to(dev)

    def launch():
        buf = _flat(n, dev)
        buf[PAD:PAD + n] = src
        getattr(ops, op)(buf[PAD:PAD + n])
        return buf
    buf = _twice(launch, what)
    check_close(buf[PAD:PAD + n], ref, what)
    _flat_intact(buf, n, what)


@pytest.mark.parametrize("B,T,Tp,C", [(86, 77, 80, 1280),       # 1 100 800 items against 4096 x 256 = 1 048 576
                                      (64, 77, 128, 1024)])     # the cap exactly
def test_text_embed_past_the_grid_cap(dev, B, T, Tp, C):
    from consistentid_amd import ops
    what = f"A text_embed B={B} T={T} Tp={Tp} C={C}"
    V = 50
    g = torch.Generator().manual_seed(61)
    ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    ids[0, 0], ids[0, 1], ids[-1, -1], ids[-1, -2] = 0, V - 1, V - 1, 0
    tok, pos = _rnd(V, C, seed=62), _rnd(T, C, seed=63)
    ref = tok.double()[ids.long()] + pos.double()[None]
    idd, tokd, posd = ids.to(dev), tok.to(dev), pos.to(dev)
    n = B * Tp * C

    def launch():
        buf = _flat(n, dev)
        ops.text_embed(idd, tokd, posd, buf[PAD:PAD + n], B=B, T=T, Tp=Tp)
        return buf
    buf = _twice(launch, what)
    out = buf[PAD:PAD + n].view(B, Tp, C)
    check_close(out[:, :T], ref, what)
    assert bool((_bits(out[:, T:].contiguous()) == 0).all()), f"{what}: rows t >= T must be +0"
    _flat_intact(buf, n, what)


CAP_DDIM = 1024 * 256 * 8


@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
@pytest.mark.parametrize("B,per", [(1, CAP_DDIM + 8 * 33), (3, 699056),      # 3 x 699 056 = the cap + 16
                                   (1, CAP_DDIM)])
def test_cfg_ddim_step_past_the_grid_cap(dev, B, per, inpaint):
    from consistentid_amd import ops
    what = f"A cfg_ddim_step B={B} per={per} inpaint={inpaint}"
    n = B * per
    eps, lat = _rnd(2 * n, seed=71), _rnd(n, seed=72)
    coef, g = torch.tensor([1.01, -0.07, 0.9, 0.43]), 5.0
    cd = coef.double()
    e = eps[:n].double() + g * (eps[n:].double() - eps[:n].double())
    ref = cd[0] * lat.double() + cd[1] * e
    kw = {}
    if inpaint:
        mask = (torch.rand(n, generator=torch.Generator().manual_seed(73)) > 0.5).half()
        init, noise = _rnd(n, seed=74), _rnd(n, seed=75)
        ref = (1 - mask.double()) * (cd[2] * init.double() + cd[3] * noise.double()) + mask.double() * ref
        kw = dict(mask=mask.to(dev), init=init.to(dev), noise=noise.to(dev))
    epsd, latd, coefd = eps.to(dev), lat.to(dev), coef.to(dev)

    def launch():
        buf = _flat(n, dev)
        buf[PAD:PAD + n] = latd
        ops.cfg_ddim_step(epsd, buf[PAD:PAD + n], coefd, g, B=B, per_sample=per, **kw)
        return buf
    buf = _twice(launch, what)
    check_close(buf[PAD:PAD + n], ref, what)
    _flat_intact(buf, n, what)


CAP_ADD = 2048 * 256 * 8


def test_add_inplace_refuses_a_half_that_is_no_multiple_of_8(dev, lib):
    """n = 4 194 304 + 8 * 5 with na = n / 2: the half is 2 097 172 = 8 * 262 146 + 4, which the launch refuses (every lane
    moves 16 bytes of ``a`` from q % na)"""
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    n = CAP_ADD + 8 * 5
    y, a = torch.zeros(n, dtype=torch.float16, device=dev), torch.ones(n // 2, dtype=torch.float16, device=dev)
    with pytest.raises(CidError, match="cid_add_inplace_f16: sizes must be multiples of 8"):
        ops.add_inplace(y, a)
    torch.cuda.synchronize()
    assert not bool(y.any()), "a refused launch wrote"


@pytest.mark.parametrize("n", [CAP_ADD + 8 * 6, CAP_ADD], ids=["past", "at_cap"])
def test_add_inplace_past_the_grid_cap(dev, n):
    from consistentid_amd import ops
    what = f"A add_inplace n={n} na={n // 2}"
    y, a = _rnd(n, seed=81), _rnd(n // 2, seed=82)
    ref = y.double() + torch.cat([a, a]).double()
    yd, ad = y.to(dev), a.to(dev)

    def launch():
        buf = _flat(n, dev)
        buf[PAD:PAD + n] = yd
        ops.add_inplace(buf[PAD:PAD + n], ad)
        return buf
    buf = _twice(launch, what)
    check_close(buf[PAD:PAD + n], ref, what)
    _flat_intact(buf, n, what)


# ----------------------------------------------------------------------------- B. linear_small
# (M, K, N, bias, add pitch: None / 0 / "N", act_in, act_out, pitched): every pair of M x K, M x N and K x N values
LINEAR_CASES = [
    (1, 8, 4, True, None, 0, 0, False), (1, 320, 1002, False, 0, 1, 0, False), (1, 1280, 1013, True, "N", 0, 1, False),
    (1, 2816, 4, True, None, 1, 1, False),
    (8, 8, 1002, True, "N", 1, 1, False), (8, 320, 1013, True, None, 0, 0, True), (8, 1280, 4, False, 0, 0, 1, False),
    (8, 2816, 1013, True, 0, 1, 0, False),
    (9, 8, 1013, False, None, 0, 1, False), (9, 320, 4, True, "N", 1, 1, False), (9, 1280, 1002, True, None, 1, 0, False),
    (9, 2816, 1002, True, 0, 0, 0, False),
    (50, 8, 4, True, 0, 1, 0, False), (50, 320, 1002, True, None, 0, 1, False), (50, 1280, 1013, False, "N", 1, 1, True),
    (50, 2816, 1013, True, None, 0, 0, False),
    (64, 8, 1013, True, "N", 0, 0, False), (64, 320, 1013, True, 0, 1, 1, False), (64, 1280, 4, True, None, 0, 1, False),
    (64, 2816, 1002, False, None, 1, 0, False),
]


def test_linear_small_cases_are_pairwise():
    import itertools
    axes = ((1, 8, 9, 50, 64), (8, 320, 1280, 2816), (4, 1002, 1013))
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert {(c[i], c[j]) for c in LINEAR_CASES} == set(itertools.product(axes[i], axes[j]))
    assert {(c[5], c[6]) for c in LINEAR_CASES} == set(itertools.product((0, 1), (0, 1)))
    assert {c[4] for c in LINEAR_CASES} == {None, 0, "N"} and {c[3] for c in LINEAR_CASES} == {True, False}


@pytest.mark.parametrize("M,K,N,bias,add,act_in,act_out,pitched", LINEAR_CASES)
def test_linear_small_edges(dev, M, K, N, bias, add, act_in, act_out, pitched):
    """eight register slabs (M = 64), a ragged last slab (9, 50), idle lanes (K = 8, 320), 5.5 rounds (K = 2816), the ragged
    last wave (N = 1002) and the ragged last block (N = 4, 1013)"""
    from consistentid_amd import ops
    what = f"B linear_small M={M} K={K} N={N} bias={bias} add={add} act={act_in}{act_out} pitched={pitched}"
    x, w = _rnd(M, K, seed=M + K), _rnd(N, K, seed=N + K, scale=K ** -0.5)
    b = _rnd(N, seed=91) if bias else None
    a = None if add is None else _rnd(1 if add == 0 else M, N, seed=92)
    xr = F.silu(x.double()) if act_in else x.double()
    ref = xr @ w.double().T
    if b is not None:
        ref = ref + b.double()
    if a is not None:
        ref = ref + a.double()
    if act_out:
        ref = F.silu(ref)
    ldx, ldo = (K + 8, N + 3) if pitched else (K, N)
    xbuf, xv = _wide(x, ldx, dev)
    wd, bd, ad = w.to(dev), (b.to(dev) if bias else None), (a.to(dev) if a is not None else None)

    def launch():
        buf = _guarded(M, ldo, dev)
        ops.linear_small(xv, wd, bd, buf[GUARD:GUARD + M], M=M, N=N, K=K, ldx=ldx, ldo=ldo, add=ad,
                         ldadd=0 if add in (None, 0) else N, act_in=act_in, act_out=act_out)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + M, :N], ref, what)
    _intact(buf, M, 0, N, what)


# ----------------------------------------------------------------------------- C. small_attn
def _small_attn_case(dev, what, B, Lq, heads, n1, n2, q, kv1, kv2):
    from consistentid_amd import ops
    inner, n = heads * 64, n1 + n2
    kv = kv1.double().view(B, n1, -1)
    if n2:
        kv = torch.cat([kv, kv2.double().view(B, n2, -1)], dim=1)
    kk, vv = (t.view(B, n, heads, 64).transpose(1, 2) for t in kv.chunk(2, dim=-1))
    s = q.double().view(B, Lq, heads, 64).transpose(1, 2) @ kk.transpose(-1, -2) / 8.0
    ref = (torch.softmax(s, dim=-1) @ vv).transpose(1, 2).reshape(B * Lq, inner)
    qd, k1d, k2d = q.to(dev), kv1.to(dev), (kv2.to(dev) if n2 else None)

    def launch():
        buf = _guarded(B * Lq, inner, dev)
        ops.small_attn(qd, k1d, k2d, buf[GUARD:GUARD + B * Lq], B=B, Lq=Lq, n1=n1, n2=n2, heads=heads)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + B * Lq], ref, what)
    _intact(buf, B * Lq, 0, inner, what)
    return s


@pytest.mark.parametrize("B,Lq,heads", [(1, 1, 1), (3, 5, 3), (2, 4, 8)], ids=["1wave", "45waves", "64waves"])
@pytest.mark.parametrize("n1,n2", [(1, 0), (59, 4), (60, 4), (61, 4), (257, 4), (1020, 4), (1024, 0)])
def test_small_attn_key_and_wave_counts(dev, n1, n2, B, Lq, heads):
    """1, 63, 64, 65, 261, 1024 keys (with and without a second block) on 1, 45 and 64 waves: 45 leaves three waves of the
    last workgroup without work"""
    inner = heads * 64
    q, kv1 = _rnd(B * Lq, inner, seed=n1 + Lq), _rnd(B * n1, 2 * inner, seed=n1 + 1)
    kv2 = _rnd(B * n2, 2 * inner, seed=n1 + 2) if n2 else None
    _small_attn_case(dev, f"C small_attn n1={n1} n2={n2} B={B} Lq={Lq} heads={heads}", B, Lq, heads, n1, n2, q, kv1, kv2)


def test_small_attn_max_shift(dev):
    """one key's logit 40 above the rest: exp(40) against exp(0) only comes out right with the row maximum subtracted"""
    B, Lq, heads, n1, n2 = 1, 1, 1, 126, 4
    q = _rnd(1, 64, seed=5)
    kv1, kv2 = _rnd(n1, 128, seed=6, scale=0.1), _rnd(n2, 128, seed=7, scale=0.1)
    kv1[:, 64:], kv2[:, 64:] = _rnd(n1, 64, seed=8), _rnd(n2, 64, seed=9)
    kv1[70, :64] = (q[0].double() * (40.0 * 8.0 / float((q[0].double() ** 2).sum()))).half()
    s = _small_attn_case(dev, "C small_attn, one logit 40 above the rest", B, Lq, heads, n1, n2, q, kv1, kv2)
    s = s.flatten()
    rest = torch.cat([s[:70], s[71:]])
    assert 38.0 < float(s[70] - rest.max()) and float(s[70] - rest.mean()) < 42.0, "the case lost its outlier"


# ----------------------------------------------------------------------------- F. fp16 norms
def _gn_ref(x, groups, gm, bt, eps, silu):
    """x [B, HW, C] -> fp64 [B * HW, C]"""
    y = F.group_norm(x.double().transpose(1, 2), groups, gm.double(), bt.double(), eps)
    if silu:
        y = F.silu(y)
    return y.transpose(1, 2).reshape(-1, x.shape[-1])


GN_CASES = [(2, hw, 64, 0, 1, True) for hw in (255, 256, 257)] \
    + [(8, hw, 64, 0, 8, False) for hw in (255, 256, 257)] \
    + [(2, hw, 256, 0, 64, True) for hw in (255, 256, 257)] \
    + [(2, 64, 64, 0, 32, True),             # cg = 2: no 4-channel pieces, two launches although HW <= 256
       (2, 1, 320, 0, 32, True),             # HW = 1 on the two-launch path (cg = 10)
       (3, 1, 128, 0, 32, False),            # ... and on the single launch (cg = 4)
       (1, 16416, 64, 0, 32, True),          # gn_rows = 64: 257 partial blocks
       (1, 3080, 1280, 1280, 32, True)]      # 3 rows per apply block would be 1027 blocks: rpb is recomputed to 4; concat source


@pytest.mark.parametrize("B,HW,c1,c2,groups,silu", GN_CASES)
def test_groupnorm_selections(dev, B, HW, c1, c2, groups, silu):
    from consistentid_amd import ops
    what = f"F groupnorm B={B} HW={HW} C={c1}+{c2} groups={groups} silu={silu}"
    C = c1 + c2
    x = _rnd(B, HW, C, seed=HW + groups, scale=1.5) + _rnd(1, 1, C, seed=3)
    gm, bt = (1 + 0.2 * _rnd(C, seed=4).float()).half(), _rnd(C, seed=5, scale=0.2)
    ref = _gn_ref(x, groups, gm, bt, 1e-5, silu)
    x1 = x[..., :c1].reshape(-1, c1).contiguous().to(dev)
    x2 = x[..., c1:].reshape(-1, c2).contiguous().to(dev) if c2 else None
    gd, bd = gm.to(dev), bt.to(dev)
    ws = torch.empty(ops.groupnorm_ws_bytes(B, C), dtype=torch.uint8, device=dev)

    def launch():
        buf = _guarded(B * HW, C, dev)
        ops.groupnorm(x1, buf[GUARD:GUARD + B * HW], gd, bd, ws, B=B, HW=HW, c1=c1, x2=x2, c2=c2, groups=groups, silu=silu)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + B * HW], ref, what)
    _intact(buf, B * HW, 0, C, what)


def test_groupnorm_from_host_statistics(dev, lib):
    """cid_groupnorm_stats_f16 with the statistics a GEMM epilogue would have written, computed here in fp32: fp32
    [B * nb][32][2] per source, one (sum, sum of squares) per block of ``rows`` tokens and unit of c / 32 channels; the two
    sources at different block heights (256 and 128)"""
    from consistentid_amd import ops
    from consistentid_amd._lib import check
    what = "F groupnorm_stats B=2 HW=4096 320+320 rows 256/128"
    B, HW, c1, c2, groups, rows1, rows2 = 2, 4096, 320, 320, 32, 256, 128
    C = c1 + c2
    x = _rnd(B, HW, C, seed=11, scale=1.5) + _rnd(1, 1, C, seed=12)
    gm, bt = (1 + 0.2 * _rnd(C, seed=13).float()).half(), _rnd(C, seed=14, scale=0.2)
    ref = _gn_ref(x, groups, gm, bt, 1e-5, True)

    def stats(xs, rows):
        c = xs.shape[-1]
        blocks = xs.double().reshape(B * HW // rows, rows, 32, c // 32)
        return torch.stack([blocks.sum((1, 3)), (blocks * blocks).sum((1, 3))], -1).float().contiguous()
    st1, st2 = stats(x[..., :c1], rows1).to(dev), stats(x[..., c1:], rows2).to(dev)
    assert tuple(st1.shape) == (B * HW // rows1, 32, 2) and tuple(st2.shape) == (B * HW // rows2, 32, 2)
    x1, x2 = x[..., :c1].reshape(-1, c1).contiguous().to(dev), x[..., c1:].reshape(-1, c2).contiguous().to(dev)
    gd, bd = gm.to(dev), bt.to(dev)

    def launch():
        buf = _guarded(B * HW, C, dev)
        check(lib.cid_groupnorm_stats_f16(x1.data_ptr(), x2.data_ptr(), c1, c2, buf[GUARD:GUARD + B * HW].data_ptr(), gd.data_ptr(),
                                          bd.data_ptr(), B, HW, groups, 1e-5, 1, st1.data_ptr(), rows1, st2.data_ptr(), rows2,
                                          ops._stream()), "cid_groupnorm_stats_f16")
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + B * HW], ref, what)
    _intact(buf, B * HW, 0, C, what)


def _ln_inputs(M, C, seed):
    x = _rnd(M, C, seed=seed, scale=1.3) + _rnd(1, C, seed=seed + 1, scale=0.5)
    gm, bt = (1 + 0.2 * _rnd(C, seed=seed + 2).float()).half(), _rnd(C, seed=seed + 3, scale=0.2)
    return x, gm, bt, F.layer_norm(x.double(), (C,), gm.double(), bt.double(), 1e-5)


@pytest.mark.parametrize("M,C", [(5, 8), (7, 1536), (3, 1528)])
def test_layernorm_channel_range(dev, M, C):
    """one chunk on one lane, all three chunks of all 64 lanes, and a last chunk round that leaves one lane out"""
    from consistentid_amd import ops
    what = f"F layernorm M={M} C={C}"
    x, gm, bt, ref = _ln_inputs(M, C, seed=C)
    xd, gd, bd = x.to(dev), gm.to(dev), bt.to(dev)

    def launch():
        buf = _guarded(M, C, dev)
        ops.layernorm(xd, buf[GUARD:GUARD + M], gd, bd, M=M, C_=C)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + M], ref, what)
    _intact(buf, M, 0, C, what)


@pytest.mark.parametrize("M,C", [(32768, 320),      # eight lanes per row, five chunks per lane
                                 (8200, 1280)])     # sixteen lanes per row, ten chunks; 8200 = 512 x 16 + 8: a half-used last wave
def test_layernorm_rows_kernels_with_both_pitches(dev, M, C):
    """the several-rows-per-wave kernels (M * C >= 8 Mi) reading a column block of a 5 C wide buffer and writing one of a
    2 C wide guarded buffer; whatever surrounds the input block is NaN"""
    from consistentid_amd import ops
    what = f"F layernorm rows kernel M={M} C={C} ldx=5C ldo=2C"
    assert M * C >= 8 << 20
    x, gm, bt, ref = _ln_inputs(M, C, seed=C + 1)
    ldx, ldo, c0 = 5 * C, 2 * C, 8
    xbuf, xv = _wide(x, ldx, dev, c0=2 * C)
    gd, bd = gm.to(dev), bt.to(dev)

    def launch():
        buf = _guarded(M, ldo, dev)
        ops.layernorm(xv, buf[GUARD:GUARD + M, c0:c0 + C], gd, bd, M=M, C_=C, ldx=ldx, ldo=ldo)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + M, c0:c0 + C], ref, what)
    _intact(buf, M, c0, C, what)


def _softmax_case(dev, what, rows, cols, ld, dtype, tol):
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g) * 4
    x = x.half() if dtype == torch.float16 else x
    ref = torch.softmax(x.double() * LN2, dim=-1)
    xd = x.to(dev)
    op = ops.softmax_rows if dtype == torch.float16 else ops.softmax_rows_f32

    def launch():
        buf = _guarded(rows, ld, dev, dtype)
        buf[GUARD:GUARD + rows, :cols] = xd
        op(buf[GUARD:GUARD + rows], rows=rows, cols=cols, ld=ld)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + rows, :cols], ref, what, **tol)
    _intact(buf, rows, 0, cols, what)


@pytest.mark.parametrize("rows,cols,ld", [(1, 8, 8),             # one chunk on one lane, three waves of the workgroup leave
                                          (5, 520, 528),         # 65 chunks: lane 0 takes a second trip, rows % 4 != 0
                                          (3, 4096, 4096),       # eight trips per lane
                                          (37, 64, 72)])         # eight lanes busy; pad columns behind every row
def test_softmax_rows_geometries(dev, rows, cols, ld):
    _softmax_case(dev, f"F softmax_rows rows={rows} cols={cols} ld={ld}", rows, cols, ld, torch.float16, {})


# ----------------------------------------------------------------------------- G. fp32
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("B,HW,C,groups", [(2, 1, 64, 32),          # one pixel: the variance is between channels only
                                           (1, 63, 4, 1),           # one statistics block, one float4 per pixel
                                           (1, 65, 256, 64),        # two statistics blocks, the second of one row
                                           (1, 16450, 32, 8),       # gn32_rows = 65: 254 blocks
                                           (1, 70, 2048, 32)])      # the LDS ceiling of the finalize kernel
def test_groupnorm_f32_edges(dev, B, HW, C, groups, silu):
    from consistentid_amd import ops
    what = f"G groupnorm_f32 B={B} HW={HW} C={C} groups={groups} silu={silu}"
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(B, HW, C, generator=g) * 3 + torch.randn(1, 1, C, generator=g)
    gm, bt = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = _gn_ref(x, groups, gm, bt, 1e-6, silu)
    xd, gd, bd = x.reshape(-1, C).to(dev), gm.to(dev), bt.to(dev)
    ws = torch.empty(ops.groupnorm_f32_ws_bytes(B, HW, C), dtype=torch.uint8, device=dev)

    def launch():
        buf = _guarded(B * HW, C, dev, torch.float32)
        ops.groupnorm_f32(xd, buf[GUARD:GUARD + B * HW], gd, bd, ws, B=B, HW=HW, C_=C, groups=groups, silu=silu)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + B * HW], ref, what, **TOL32)
    _intact(buf, B * HW, 0, C, what)


@pytest.mark.parametrize("rows,cols,ld", [(3, 1, 4), (2, 255, 260), (2, 257, 257), (1, 5000, 5000)])
def test_softmax_rows_f32_geometries(dev, rows, cols, ld):
    """one column, one short of / one past a trip of the 256 threads with odd pitches, twenty trips"""
    _softmax_case(dev, f"G softmax_rows_f32 rows={rows} cols={cols} ld={ld}", rows, cols, ld, torch.float32, TOL32)


@pytest.mark.parametrize("M,N,c,ldx", [(70, 40, 20, 20),        # K = 20 on the vector path: the second k step holds one float4
                                       (70, 24, 32, 40)])       # a 1 x 1 call on a column block of a wider input
def test_gemm_f32_k_tail_and_input_pitch(dev, M, N, c, ldx):
    from consistentid_amd import ops
    what = f"G gemm_f32 M={M} N={N} c={c} ldx={ldx}"
    g = torch.Generator().manual_seed(c + ldx)
    x, w, b = torch.randn(M, c, generator=g), torch.randn(N, c, generator=g) * c ** -0.5, torch.randn(N, generator=g)
    ref = x.double() @ w.double().T + b.double()
    xbuf, xv = _wide(x, ldx, dev)
    wd, bd = w.to(dev), b.to(dev)
    ldo = N + 4

    def launch():
        buf = _guarded(M, ldo, dev, torch.float32)
        ops.gemm_f32(xv, wd, buf[GUARD:GUARD + M], M=M, N=N, c=c, bias=bd, ldx=ldx, ldo=ldo)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + M, :N], ref, what, **TOL32)
    _intact(buf, M, 0, N, what)
