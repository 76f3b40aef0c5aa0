"""The kernels that run once per generation, before the denoise loop or at its first launch, at their shape and grid-cap
edges: the face parser's kernels (csrc/parsing.hip), the two ends of the VAE encoder (csrc/vae_enc.hip), the time embedding
and the step table (csrc/misc.hip) and the two cross-attention packers (csrc/xattn.hip, csrc/xattn3.hip).

The conventions and helpers are those of tests/test_gpu_direct_kernels.py: seeded inputs (fp16-representable, or fp32 / uint8
where the kernel takes those), the same operation in fp64 on the CPU as the reference, the output in a sentinel-filled buffer
with guards in front and behind (guard columns where a pitch is given), guards bit-untouched afterwards, a second launch
bit-identical to the first, and read-only inputs between NaNs where the type has one.  fp16 outputs are held to
conftest.check_close's defaults, fp32 outputs to test_gpu_vae.TOL32, copies and index kernels bit for bit.

The grid caps the shapes of section A depend on (a change of a cap moves the shape with it):

    vae_encode_in   4096 blocks x 32 pixels           vae_encode_out   8192 blocks x 4 pixels
    chan_affine     4096 blocks x 256 octets          parse_head       8192 blocks x 256 pixels
    gather_pack     4096 blocks x 256 elements        pack_wfrag       2048 blocks x 256 octets

No listed shape is refused by a host check.  vae_encode_in at 363 x 362 takes no mask_latents (the image is no multiple of
8); that refusal is asserted beside the launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_close
from gemm_parity import GUARD, SENTINEL
from test_gpu_direct_kernels import PAD, _bits, _flat, _flat_intact, _guarded, _intact, _rnd, _tok, _twice, _wide
from test_gpu_vae import TOL32

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- helpers beyond test_gpu_direct_kernels'
def _nanpad(t, dev):
    """``t`` on the device with PAD NaNs in front of and behind it: a read outside it poisons the result"""
    n = t.numel()
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=t.dtype, device=dev)
    buf[PAD:PAD + n] = t.reshape(-1).to(dev)
    return buf[PAD:PAD + n].view(t.shape)


def _twice_all(launch, what):
    """_twice for a launch with several outputs: launch() -> a tuple of freshly filled buffers"""
    a = launch()
    b = launch()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: output {i} of the second launch differs"
    return a


def _bytes(n, dev):
    """n uint8 outputs inside a _flat fp16 buffer -> (the buffer, the [n] uint8 view)"""
    buf = _flat((n + 1) // 2, dev)
    return buf, buf.view(torch.uint8)[2 * PAD:2 * PAD + n]


def _bytes_intact(buf, n, what):
    _flat_intact(buf, (n + 1) // 2, what)
    if n & 1:          # the odd byte behind the last output is the high byte of a sentinel
        assert int(buf.view(torch.uint8)[2 * PAD + n]) == SENTINEL >> 8, f"{what}: the byte behind the output was written"


# ----------------------------------------------------------------------------- vae_encode_in (sections A and G)
MASK_VALUES = torch.tensor([0.0, 1.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(0.0)))])


def _encode_in_case(dev, what, Bi, Bm, H, W, cout, normalize, seed):
    """blocks = 3 with a mask (and mask_latents where the image allows them), blocks = 2 bit-equal to its second block,
    blocks = 1 without a mask"""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    img = torch.rand(Bi, 3, H, W, generator=g) * 6 - 3
    mask = MASK_VALUES[torch.randint(0, 4, (Bm, 1, H, W), generator=g)]
    w = (torch.randn(cout, 27, generator=g) * 0.2).half()
    b = (torch.randn(cout, generator=g) * 0.1).half()
    pix = ((img * 2 - 1) if normalize else img).half().double()          # the kernel rounds the fp32 pixel to fp16 once
    binm = mask >= 0.5                                                   # 0.5 itself repaints, the float below it keeps
    wk = w.double().view(cout, 3, 3, 3).permute(0, 3, 1, 2)              # [cout][ky][kx][ci] -> [cout][ci][ky][kx]
    conv = lambda t: _tok(F.conv2d(t, wk, b.double(), padding=1))
    ref_img, ref_msk = conv(pix), conv(pix * (~binm).double())           # Bm = 1: one mask for every sample
    with_ml = H % 8 == 0 and W % 8 == 0
    n_ml = Bm * (H // 8) * (W // 8)
    imgd, maskd, wd, bd = _nanpad(img, dev), _nanpad(mask, dev), _nanpad(w, dev), _nanpad(b, dev)

    def run(blocks, masked, ml_too):
        rows = (2 if blocks == 3 else 1) * Bi * HW

        def launch():
            buf = _guarded(rows, cout, dev)
            ml = _flat(n_ml, dev) if ml_too else None
            ops.vae_encode_in(imgd, buf[GUARD:GUARD + rows].view(-1, HW, cout), wd, bd, mask=maskd if masked else None,
                              normalize=normalize, blocks=blocks,
                              mask_latents=ml[PAD:PAD + n_ml].view(Bm, 1, H // 8, W // 8) if ml_too else None)
            return (buf, ml) if ml_too else (buf,)
        bufs = _twice_all(launch, f"{what} blocks={blocks}")
        _intact(bufs[0], rows, 0, cout, f"{what} blocks={blocks}")
        return bufs[0][GUARD:GUARD + rows], (bufs[1] if ml_too else None)

    both, ml = run(3, True, with_ml)
    check_close(both, torch.cat([ref_img, ref_msk]), f"{what} blocks=3")
    if with_ml:
        want = F.interpolate(binm.float(), size=(H // 8, W // 8)).half()
        assert torch.equal(ml[PAD:PAD + n_ml].cpu(), want.flatten()), f"{what}: mask_latents"
        _flat_intact(ml, n_ml, f"{what} mask_latents")
    only_masked, _ = run(2, True, False)
    assert torch.equal(only_masked, both[Bi * HW:]), f"{what}: blocks=2 differs from the second block of blocks=3"
    plain, _ = run(1, False, False)
    check_close(plain, ref_img, f"{what} blocks=1, no mask")


@pytest.mark.parametrize("H,W", [(363, 362),       # 131 406 pixels against 4096 x 32 = 131 072: a ragged second trip
                                 (512, 256)])      # the cap exactly, with mask_latents
def test_vae_encode_in_past_the_grid_cap(dev, lib, H, W):
    _encode_in_case(dev, f"A vae_encode_in {H}x{W}", 1, 1, H, W, 8, True, seed=H)
    if H % 8:
        rc = lib.cid_vae_encode_in_f16(64, 1, 64, 1, 64, 64, 64, H, W, 8, 1, 3, 64, None)
        assert rc == -22 and b"mask_latents need H and W multiples of 8 (got 363 x 362)" in lib.cid_last_error()


_EI_IMAGES, _EI_COUTS = ((1, 1), (1, 9), (9, 1), (8, 8), (16, 24)), (8, 136, 320)
# (H, W, cout, Bm, normalize) at Bi = 3: every image x cout; Bm and normalize alternate so that each image sees both of each
ENCODE_IN_CASES = [(*im, co, (1, 3)[(i + j) % 2], bool((i + j // 2) % 2)) for i, im in enumerate(_EI_IMAGES) for j, co in enumerate(_EI_COUTS)]


@pytest.mark.parametrize("H,W,cout,Bm,normalize", ENCODE_IN_CASES)
def test_vae_encode_in_edges(dev, H, W, cout, Bm, normalize):
    """cout of one octet, of 17 octets over the 8 threads of a pixel, and EI_MAXCO; one-pixel, one-row, one-column images; the
    mask of Bm = 1 serving three samples, its mask_latents [1, 1, H / 8, W / 8] between guards"""
    _encode_in_case(dev, f"G vae_encode_in {H}x{W} cout={cout} Bi=3 Bm={Bm} normalize={normalize}", 3, Bm, H, W, cout, normalize,
                    seed=H * 100 + W + cout)


def test_vae_encode_in_cases_cover_every_value():
    assert {c[:3] for c in ENCODE_IN_CASES} == {(*im, co) for im in _EI_IMAGES for co in _EI_COUTS}
    for im in ((8, 8), (16, 24)):          # the images with mask_latents
        assert {c[3] for c in ENCODE_IN_CASES if c[:2] == im} == {1, 3}
    assert {(c[3], c[4]) for c in ENCODE_IN_CASES} == {(1, True), (1, False), (3, True), (3, False)}


# ----------------------------------------------------------------------------- vae_encode_out (A and H)
def _encode_out_case(dev, what, B, H, W, cin, L, use_eps, use_mom, rot, seed):
    """``rot`` rotates the five kinds of logvar channel over the L channels: 0 exactly 20, 1 exactly -30 (zero weights, the
    bias alone), 2 past 20, 3 below -30, 4 inside the clamp"""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(seed)
    HW, scale = H * W, 0.18215
    x = torch.randn(B, cin, H, W, generator=g).half()
    w = (torch.randn(2 * L, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    bias = torch.randn(2 * L, generator=g) * 0.1
    eps = torch.randn(B, L, H, W, generator=g).half()
    kinds = [(rot + j) % 5 for j in range(L)]
    for j, k in enumerate(kinds):
        if k in (0, 1):
            w[L + j] = 0
        if k < 4:
            bias[L + j] = (20.0, -30.0, 45.0, -60.0)[k]
        if k in (0, 2):              # std = e^10: |eps| <= 2^-6 keeps the fp16 sample finite
            eps[:, j] = (eps[:, j].float() * 2.0 ** -8).clamp(-2.0 ** -6, 2.0 ** -6).half()
    m = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    mean, logvar = m.chunk(2, dim=1)
    std = torch.exp(0.5 * logvar.clamp(-30, 20))
    xd, epsd = _nanpad(_tok(x), dev), _nanpad(eps, dev)
    wd, bd = _nanpad(w.permute(0, 2, 3, 1).reshape(2 * L, 9 * cin), dev), _nanpad(bias, dev)
    n = B * L * HW

    def launch():
        buf = _flat(n, dev)
        mom = _flat(2 * n, dev, torch.float32) if use_mom else None
        ops.vae_encode_out(xd, buf[PAD:PAD + n].view(B, L, H, W), wd, bd, B=B, H=H, W=W, cin=cin, L=L, scale=scale,
                           eps=epsd if use_eps else None, moments=mom[PAD:PAD + 2 * n].view(B, 2 * L, H, W) if use_mom else None)
        return (buf, mom) if use_mom else (buf,)
    bufs = _twice_all(launch, what)
    out = bufs[0][PAD:PAD + n].view(B, L, H, W)
    _flat_intact(bufs[0], n, what)
    if use_mom:
        mom = bufs[1][PAD:PAD + 2 * n].view(B, 2 * L, H, W)
        _flat_intact(bufs[1], 2 * n, f"{what} moments")
        check_close(mom[:, :L], mean, f"{what} moments: mean")
        check_close(mom[:, L:], logvar, f"{what} moments: logvar (unclamped)")
        for j, k in enumerate(kinds):
            if k in (0, 1):          # nine taps of zero weights add +0 to the bias
                assert bool((mom[:, L + j] == (20.0, -30.0)[k]).all()), f"{what}: logvar channel {j} is not the bias itself"
    if use_eps:
        for c in range(L):
            check_close(out[:, c], scale * (mean + std * eps.double())[:, c], f"{what} sample, channel {c} (kind {kinds[c]})")
    else:
        check_close(out, scale * mean, f"{what} mode")


@pytest.mark.parametrize("H,W", [(182, 181),       # 32 942 pixels against 8192 x 4 = 32 768
                                 (128, 256)])      # the cap exactly
def test_vae_encode_out_past_the_grid_cap(dev, H, W):
    _encode_out_case(dev, f"A vae_encode_out {H}x{W}", 1, H, W, 8, 4, True, True, 0, seed=H)


# (L, cin, H, W, B, eps, moments, rot): cin = 8 one lane, 64 eight lanes, 512 one full trip of the c8 += 64 loop, 520 one lane
# on a second trip, 1024 two full trips
ENCODE_OUT_CASES = [(1, 8, 1, 1, 1, True, True, 0), (2, 64, 1, 7, 2, True, False, 1), (3, 512, 5, 1, 2, False, True, 2),
                    (4, 520, 12, 10, 1, True, True, 0), (4, 1024, 12, 10, 2, True, True, 1), (1, 1024, 1, 7, 1, False, False, 4),
                    (2, 520, 5, 1, 3, True, True, 3), (3, 8, 12, 10, 2, True, False, 2), (4, 64, 1, 1, 2, True, True, 3),
                    (3, 520, 1, 7, 1, True, True, 4), (2, 512, 12, 10, 1, True, True, 0)]


@pytest.mark.parametrize("L,cin,H,W,B,use_eps,use_mom,rot", ENCODE_OUT_CASES)
def test_vae_encode_out_edges(dev, L, cin, H, W, B, use_eps, use_mom, rot):
    _encode_out_case(dev, f"H vae_encode_out L={L} cin={cin} {H}x{W} B={B} eps={use_eps} moments={use_mom} rot={rot}", B, H, W, cin, L,
                     use_eps, use_mom, rot, seed=cin + 10 * L + H)


def test_vae_encode_out_cases_cover_every_value():
    assert {c[0] for c in ENCODE_OUT_CASES} == {1, 2, 3, 4} and {c[1] for c in ENCODE_OUT_CASES} == {8, 64, 512, 520, 1024}
    assert {c[2:4] for c in ENCODE_OUT_CASES} == {(1, 1), (1, 7), (5, 1), (12, 10)}
    assert {c[5:7] for c in ENCODE_OUT_CASES} == {(True, True), (True, False), (False, True), (False, False)}
    sampled = {(c[7] + j) % 5 for c in ENCODE_OUT_CASES if c[5] for j in range(c[0])}
    assert sampled == {0, 1, 2, 3, 4}, "every kind of logvar channel under a sampled output"
    assert any(c[1] >= 520 and {(c[7] + j) % 5 for j in range(c[0])} >= {0, 1, 2, 3} for c in ENCODE_OUT_CASES)


# ----------------------------------------------------------------------------- chan_affine (A and E)
def _affine_case(dev, what, B, HW, C, kind, seed):
    """out of place between NaN-padded inputs, then in place (out is x) as face_parsing.py calls it: bit-identical"""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(seed)
    x, res = _rnd(B, HW, C, seed=seed + 1), _rnd(B, HW, C, seed=seed + 2)
    s, t = torch.rand(B, C, generator=g) * 2, torch.randn(B, C, generator=g)       # a different row per sample
    add = {"t": t.double()[:, None, :], "res": res.double(), "self": x.double()}[kind]
    ref = (x.double() * s.double()[:, None, :] + add).flatten()
    xd, sd = _nanpad(x, dev), _nanpad(s, dev)
    kw = {"t": lambda: dict(t=_nanpad(t, dev)), "res": lambda: dict(res=_nanpad(res, dev)), "self": dict}[kind]()
    n = B * HW * C

    def out_of_place():
        buf = _flat(n, dev)
        ops.chan_affine(xd, sd, buf[PAD:PAD + n], B=B, HW=HW, C_=C, **kw)
        return buf

    def in_place():
        buf = _flat(n, dev)
        buf[PAD:PAD + n] = xd.flatten()
        ops.chan_affine(buf[PAD:PAD + n], sd, buf[PAD:PAD + n], B=B, HW=HW, C_=C, **kw)
        return buf
    a, b = _twice(out_of_place, what), _twice(in_place, f"{what} in place")
    check_close(a[PAD:PAD + n], ref, what)
    _flat_intact(a, n, what)
    _flat_intact(b, n, f"{what} in place")
    assert torch.equal(_bits(a), _bits(b)), f"{what}: the in-place result differs from the out-of-place one"


@pytest.mark.parametrize("B,HW,kind", [(3, 349527, "t"),            # 1 048 581 octets against 4096 x 256 = 1 048 576: the five
                                       (3, 349527, "res"),          # octets of the second trip belong to sample 2
                                       (1, 1048576, "self")])       # the cap exactly
def test_chan_affine_past_the_grid_cap(dev, B, HW, kind):
    _affine_case(dev, f"A chan_affine B={B} HW={HW} C=8 {kind}", B, HW, 8, kind, seed=HW % 1000)


@pytest.mark.parametrize("kind", ["t", "res", "self"])
@pytest.mark.parametrize("B,HW,C", [(3, 1, 8), (3, 37, 72), (2, 256, 512)])
def test_chan_affine_kinds(dev, B, HW, C, kind):
    _affine_case(dev, f"E chan_affine B={B} HW={HW} C={C} {kind}", B, HW, C, kind, seed=HW + C)


# ----------------------------------------------------------------------------- parse_head (A and F)
def _head_case(dev, what, B, h, w, H, W, ncls, ld, seed, ties=(), logits_too=True):
    """logits 3 * randn with NaN in the padding channels ncls .. ld - 1 and NaN rows behind the last image; labels between
    sentinels.  -> (labels, upsampled logits or None, the fp16 logits) on the CPU"""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(B, h * w, ld, generator=g) * 3).half()
    for b, p, c1, c2, v in ties:
        lg[b, p, c1] = lg[b, p, c2] = v
    lg[..., ncls:] = float("nan")
    ref = F.interpolate(lg[..., :ncls].double().reshape(B, h, w, ncls).permute(0, 3, 1, 2), (H, W), mode="bilinear",
                        align_corners=True)
    margin = 1e-4 * float(ref.abs().max())
    if ncls > 1:
        top2 = ref.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) > margin
    else:
        sure = torch.ones(B, H, W, dtype=torch.bool)
    left_out = 1.0 - float(sure.float().mean())
    print(f"[parse_head] {what}: {100 * left_out:.3f} % of the pixels within the margin {margin:.2e} of a tie")
    assert left_out <= 0.01, f"{what}: the margin leaves out {100 * left_out:.2f} % of the pixels (change the seed, not the cap)"
    lgd = _nanpad(lg, dev)
    n = B * H * W

    def launcher(give):
        def launch():
            lb, lab = _bytes(n, dev)
            up = _flat(n * ncls, dev, torch.float32) if give else None
            ops.parse_head(lgd, lab.view(B, H, W), ncls=ncls, B=B, h=h, w=w, H=H, W=W, ld=ld,
                           logits_out=up[PAD:PAD + n * ncls].view(B, ncls, H, W) if give else None)
            return (lb, up) if give else (lb,)
        return launch
    labels_of = lambda lb: lb.view(torch.uint8)[2 * PAD:2 * PAD + n].view(B, H, W).cpu().long()
    (lb,) = _twice_all(launcher(False), f"{what}, labels only")
    _bytes_intact(lb, n, f"{what}, labels only")
    lab = labels_of(lb)
    assert torch.equal(lab[sure], ref.argmax(1)[sure]), f"{what}: labels differ from the fp64 argmax outside the margin"
    assert int(lab.max()) < ncls
    up = None
    if logits_too:
        lb2, upb = _twice_all(launcher(True), what)
        _bytes_intact(lb2, n, what)
        _flat_intact(upb, n * ncls, f"{what} logits_out")
        up = upb[PAD:PAD + n * ncls].view(B, ncls, H, W).cpu()
        assert torch.isfinite(up).all(), f"{what}: non-finite logits (a source row or column past the image was read)"
        err = float((up.double() - ref).abs().max())
        print(f"[parity] {what}: max|err| = {err:.3e} against the margin {margin:.3e}")
        assert err <= margin, f"{what}: upsampled logits off by {err:.3e} > 1e-4 max|ref| = {margin:.3e}"
        assert torch.equal(labels_of(lb2), lab), f"{what}: labels with and without logits_out differ"
        assert torch.equal(lab, up.argmax(1)), f"{what}: labels are not the first-maximum argmax of the logits written"
    return lab, up, lg


def test_parse_head_past_the_grid_cap(dev):
    """3 x 3 logits to 1449 x 1448 = 2 098 152 pixels against 8192 x 256 = 2 097 152, labels only"""
    _head_case(dev, "A parse_head 3x3 -> 1449x1448 ncls=2", 1, 3, 3, 1449, 1448, 2, 8, seed=3, logits_too=False)


def test_parse_head_at_the_grid_cap(dev):
    _head_case(dev, "A parse_head B=2 4x4 -> 1024x1024 ncls=2", 2, 4, 4, 1024, 1024, 2, 8, seed=4)


def test_parse_head_identity(dev):
    """16 x 16 to 16 x 16: every weight is 1 or 0, so logits_out is the fp16 logits widened; two seeded exact ties"""
    ties = ((0, 0, 3, 7, 50.0), (2, 255, 0, 18, 40.0))
    lab, up, lg = _head_case(dev, "F parse_head identity 16x16 B=3", 3, 16, 16, 16, 16, 19, 32, seed=16, ties=ties)
    want = lg[..., :19].float().reshape(3, 16, 16, 19).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(up.view(torch.int32), want.view(torch.int32)), "identity: logits_out is not the widened fp16 logits"
    assert int(lab[0, 0, 0]) == 3 and int(lab[2, 15, 15]) == 0, "the first maximum wins an exact tie"


@pytest.mark.parametrize("B,h,w,H,W,ncls,ld", [(2, 32, 32, 8, 12, 19, 32),       # downsampling
                                               (2, 3, 5, 7, 1, 19, 32),          # W = 1: sw = 0
                                               (2, 3, 5, 1, 7, 19, 32),          # H = 1: sh = 0
                                               (2, 1, 1, 9, 9, 19, 32),          # one source pixel
                                               (2, 5, 6, 20, 23, 1, 8),          # one class: every label is 0
                                               (2, 6, 5, 23, 20, 19, 19),        # no padding channels
                                               (2, 24, 40, 96, 160, 19, 32)])    # the parser's x4, two samples
def test_parse_head_edges(dev, B, h, w, H, W, ncls, ld):
    lab, _, _ = _head_case(dev, f"F parse_head B={B} {h}x{w} -> {H}x{W} ncls={ncls} ld={ld}", B, h, w, H, W, ncls, ld,
                           seed=h * w + H)
    if ncls == 1:
        assert not bool(lab.any())


# ----------------------------------------------------------------------------- gather_pack and pack_wfrag (A and K)
def _gather_pack(src_a, src_b, idx, dst, R, src_row, n_idx):
    from consistentid_amd import _lib, ops
    _lib.check(_lib.load().cid_gather_pack_f16(src_a.data_ptr(), src_b.data_ptr(), idx.data_ptr(), dst.data_ptr(), R, src_row, n_idx,
                                               ops._stream()), "cid_gather_pack_f16")


def _pack_wfrag(w, wp, rows, K):
    from consistentid_amd import _lib, ops
    _lib.check(_lib.load().cid_pack_wfrag_f16(w.data_ptr(), wp.data_ptr(), rows, K, ops._stream()), "cid_pack_wfrag_f16")


@pytest.mark.parametrize("R,n_idx,src_row", [(3, 349527, 4099),        # 1 048 581 elements against 4096 x 256
                                             (1, 1048576, 4099),       # the cap exactly
                                             (1, 777, 96), (3, 777, 96)])
def test_gather_pack(dev, R, n_idx, src_row):
    """dst[r][e] = idx[e] < 0 ? 0 : (bit 30 of idx[e] ? src_b : src_a)[r * src_row + (idx[e] & 0x3fffffff)], bit for bit"""
    what = f"K gather_pack R={R} n_idx={n_idx} src_row={src_row}"
    g = torch.Generator().manual_seed(n_idx % 1000 + R)
    a, b = _rnd(R, src_row, seed=R), _rnd(R, src_row, seed=R + 10)
    idx = torch.randint(0, src_row, (n_idx,), generator=g, dtype=torch.int32)
    idx |= (torch.randint(0, 2, (n_idx,), generator=g, dtype=torch.int32) << 30)
    idx[torch.rand(n_idx, generator=g) < 0.1] = -1
    idx[:8] = torch.tensor([0, src_row - 1, 1 << 30, (1 << 30) + src_row - 1, -1, -(1 << 31), -(1 << 30), -5], dtype=torch.int32)
    idx[-2:] = torch.tensor([(1 << 30) + src_row - 1, src_row - 1], dtype=torch.int32)
    i64 = idx.long()
    off = i64 & 0x3fffffff
    picked = torch.where(((i64 >> 30) & 1).bool()[None], _bits(b)[:, off.clamp(max=src_row - 1)], _bits(a)[:, off.clamp(max=src_row - 1)])
    ref = torch.where((i64 < 0)[None], torch.zeros((), dtype=torch.int16), picked).flatten()
    ad, bd, idxd = _nanpad(a, dev), _nanpad(b, dev), idx.to(dev)
    n = R * n_idx

    def launch():
        buf = _flat(n, dev)
        _gather_pack(ad, bd, idxd, buf[PAD:PAD + n], R, src_row, n_idx)
        return buf
    buf = _twice(launch, what)
    assert torch.equal(_bits(buf[PAD:PAD + n]).cpu(), ref), what
    _flat_intact(buf, n, what)


@pytest.mark.parametrize("rows,K", [(2080, 2032),        # 528 320 octets against 2048 x 256 = 524 288
                                    (2048, 2048),        # the cap exactly
                                    (32, 16), (32, 48), (96, 16), (96, 1280), (32, 1280), (96, 48)])
def test_pack_wfrag(dev, rows, K):
    """wp[((rt * (K / 16) + kk) * 64 + lane) * 8 + i] = w[(rt * 32 + (lane & 31)) * K + kk * 16 + (lane >> 5) * 8 + i]"""
    what = f"K pack_wfrag rows={rows} K={K}"
    w = _rnd(rows, K, seed=rows + K)
    e = np.arange(rows * K, dtype=np.int64)
    i, q = e & 7, e >> 3
    lane, kk, rt = q & 63, (q >> 6) % (K // 16), (q >> 6) // (K // 16)
    src = (rt * 32 + (lane & 31)) * K + kk * 16 + (lane >> 5) * 8 + i
    assert np.array_equal(np.sort(src), e), "the formula is a permutation"
    ref = _bits(w).flatten()[torch.from_numpy(src)]
    wd = _nanpad(w, dev)
    n = rows * K

    def launch():
        buf = _flat(n, dev)
        _pack_wfrag(wd, buf[PAD:PAD + n], rows, K)
        return buf
    buf = _twice(launch, what)
    assert torch.equal(_bits(buf[PAD:PAD + n]).cpu(), ref), what
    _flat_intact(buf, n, what)


# ----------------------------------------------------------------------------- B. parse_stem
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("image", ["random", "zeros", "255s", "dead_channels"])
@pytest.mark.parametrize("B,H,W", [(1, 32, 32),         # one tile: all four sides are padding
                                   (1, 32, 96), (1, 96, 32),
                                   (3, 64, 64)])        # blockIdx.z >> 2 is the sample, & 3 the channel group
def test_parse_stem_per_element(dev, B, H, W, image):
    """|got - ref| <= 2^-11 |ref| + 2^-24 + 1e-5 S per element, S = the 3 x 3 / stride-2 max-pool of conv(|x_norm|, |w|) + |bias|:
    148 fp32 FMAs at 2^-24 each are 8.8e-6 of the magnitude sum (rounded up), the max-pool of values each within d_i of their
    reference is within max d_i of the pooled reference, and the fp16 store adds 2^-11 |ref| (2^-24: below the normal range).
    The zero padding lies in the normalised image, so a constant image still has borders that differ from its interior;
    "dead_channels": channels 16 .. 31 with zero weights and a negative bias come out as exactly 0 after the ReLU."""
    from consistentid_amd import ops
    what = f"B parse_stem B={B} {H}x{W} {image}"
    g = torch.Generator().manual_seed(H + 2 * W + B)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    if image in ("zeros", "255s"):
        img[:] = 0 if image == "zeros" else 255
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.1
    if image == "dead_channels":
        w[16:32] = 0
        b[16:32] = -b[16:32].abs() - 0.01
    x = img.permute(0, 3, 1, 2).double() / 255
    x = (x - torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    ref = _tok(F.max_pool2d(F.relu(F.conv2d(x, w.double(), b.double(), stride=2, padding=3)), 3, 2, 1))
    S = _tok(F.max_pool2d(F.conv2d(x.abs(), w.double().abs(), b.double().abs(), stride=2, padding=3), 3, 2, 1))
    tol = 2.0 ** -11 * ref.abs() + 2.0 ** -24 + 1e-5 * S
    # the image between bytes that are not its own border value: a read outside it is no zero padding
    n = img.numel()
    around = torch.full((n + 512,), 0 if image == "255s" else 255, dtype=torch.uint8, device=dev)
    around[256:256 + n] = img.flatten().to(dev)
    imgd = around[256:256 + n].view(B, H, W, 3)
    wd, bd = _nanpad(w.permute(0, 2, 3, 1).contiguous(), dev), _nanpad(b, dev)
    rows = B * (H // 4) * (W // 4)

    def launch():
        buf = _guarded(rows, 64, dev)
        ops.parse_stem(imgd, buf[GUARD:GUARD + rows].view(B, -1, 64), wd, bd)
        return buf
    buf = _twice(launch, what)
    _intact(buf, rows, 0, 64, what)
    got = buf[GUARD:GUARD + rows].cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    excess = ((got - ref).abs() / tol)
    print(f"[parity] {what}: max |err| / tol = {float(excess.max()):.3f}, max|err| = {float((got - ref).abs().max()):.3e}")
    assert float(excess.max()) <= 1.0, f"{what}: element {int(excess.argmax())} is off by {float(excess.max()):.2f} x its bound"
    if image == "dead_channels":
        assert not bool(ref[:, 16:32].any()) and not bool(got[:, 16:32].any()), f"{what}: dead channels are not exactly 0"


# ----------------------------------------------------------------------------- C. chan_mean
@pytest.mark.parametrize("B,HW,C,ld,c0,offset", [(1, 1, 8, 8, 0, 0.0),
                                                 (1, 31, 64, 64, 0, 0.0),             # fewer rows than the 32 row lanes
                                                 (2, 33, 72, 72, 0, 0.0),             # ragged row lanes, a second block of one octet
                                                 (2, 256, 512, 512, 0, 0.0),          # the parser's conv_avg input
                                                 (2, 256, 512, 512, 0, 100.0),        # 100 + 0.01 randn: nothing to cancel against
                                                 (2, 100, 128, 200, 40, 0.0)])        # a column block of a NaN-filled wider buffer
def test_chan_mean_edges(dev, B, HW, C, ld, c0, offset):
    from consistentid_amd import ops
    what = f"C chan_mean B={B} HW={HW} C={C} ld={ld} offset={offset}"
    g = torch.Generator().manual_seed(HW + C)
    x = (offset + (0.01 if offset else 1.0) * torch.randn(B * HW, C, generator=g)).half()
    ref = x.double().view(B, HW, C).mean(1)
    xbuf, xv = _wide(x, ld, dev, c0=c0)

    def launch():
        buf = _guarded(B, C, dev, torch.float32)
        ops.chan_mean(xv, buf[GUARD:GUARD + B], B=B, HW=HW, C_=C, ld=ld)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + B], ref, what, **TOL32)
    _intact(buf, B, 0, C, what)


# ----------------------------------------------------------------------------- D. chan_gate
# (B, K, N1, N or None without w2, b1, b2, act)
GATE_CASES = [(1, 1, 1, None, True, False, 0), (5, 64, 5, None, False, False, 1), (1, 65, 512, None, True, False, 2),
              (5, 512, 1, None, True, False, 1), (1, 512, 512, None, False, False, 2), (5, 65, 5, None, True, False, 0),
              (1, 64, 512, None, True, False, 1),
              (1, 1, 1, 1, True, True, 0), (5, 64, 5, 7, True, False, 1), (1, 65, 512, 512, False, True, 2),
              (5, 512, 512, 1, True, True, 2), (1, 512, 1, 7, True, True, 1), (5, 65, 5, 512, False, False, 0),
              (1, 64, 512, 7, True, True, 2), (5, 1, 1, 512, True, True, 1), (1, 512, 5, 1, True, False, 0)]


def _gate_case(dev, what, m, w1, b1, w2, b2, act):
    from consistentid_amd import ops
    d = lambda t: None if t is None else t.double()
    y = d(m) @ d(w1).T + (d(b1) if b1 is not None else 0.0)
    if w2 is not None:
        y = torch.relu(y) @ d(w2).T + (d(b2) if b2 is not None else 0.0)
    ref = (y, torch.relu(y), torch.sigmoid(y))[act]
    B, N = ref.shape
    p = lambda t: None if t is None else _nanpad(t, dev)
    md, w1d, b1d, w2d, b2d = p(m), p(w1), p(b1), p(w2), p(b2)

    def launch():
        buf = _guarded(B, N, dev, torch.float32)
        ops.chan_gate(md, buf[GUARD:GUARD + B], w1d, b1d, w2d, b2d, act=act)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + B], ref, what, **TOL32)
    _intact(buf, B, 0, N, what)
    return y


@pytest.mark.parametrize("B,K,N1,N,use_b1,use_b2,act", GATE_CASES)
def test_chan_gate_edges(dev, B, K, N1, N, use_b1, use_b2, act):
    g = torch.Generator().manual_seed(K + N1 + (N or 0))
    r = lambda *s: torch.randn(*s, generator=g)
    m, w1, b1 = r(B, K), r(N1, K) * K ** -0.5, (r(N1) * 0.3 if use_b1 else None)
    w2 = r(N, N1) * N1 ** -0.5 if N is not None else None
    b2 = r(N) * 0.3 if use_b2 else None
    _gate_case(dev, f"D chan_gate B={B} K={K} N1={N1} N={N} b1={use_b1} b2={use_b2} act={act}", m, w1, b1, w2, b2, act)


def test_chan_gate_cases_cover_every_value():
    plain, two = [c for c in GATE_CASES if c[3] is None], [c for c in GATE_CASES if c[3] is not None]
    for cases in (plain, two):
        assert {c[0] for c in cases} == {1, 5} and {c[1] for c in cases} == {1, 64, 65, 512} and {c[2] for c in cases} == {1, 5, 512}
        assert {c[6] for c in cases} == {0, 1, 2} and {c[4] for c in cases} == {True, False}
    assert {c[3] for c in two} == {1, 7, 512} and {c[5] for c in two} == {True, False}
    assert not any(c[5] for c in plain)          # (b2 without w2 is refused)


def test_chan_gate_sigmoid_saturates(dev):
    """pre-activations of exactly +/-30 and +/-90: exp(90) is past the fp32 range, and the result must still be finite"""
    m = torch.tensor([[1.0, 0.0], [-1.0, 0.0]])
    w1 = torch.tensor([[30.0, 5.0], [-30.0, 5.0], [90.0, 5.0], [-90.0, 5.0], [0.5, 5.0]])
    y = _gate_case(dev, "D chan_gate sigmoid at +/-30 and +/-90", m, w1, None, None, None, 2)
    assert y.flatten().tolist() == [30.0, -30.0, 90.0, -90.0, 0.5, -30.0, 30.0, -90.0, 90.0, -0.5]


# ----------------------------------------------------------------------------- I. sincos_embed
def _sincos64(v, dim):
    """oracle.unet.timestep_embedding ([cos | sin], frequencies exp(-ln(10000) i / half)) carried out in fp64"""
    half = dim // 2
    a = v.double()[:, None] * torch.exp(-np.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)[None]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=-1)


def test_sincos_reference_is_the_oracles():
    """(no GPU needed) the fp64 restatement above against the oracle's fp32 function: at an angle of 1024 rad the fp32 product
    alone is off by up to 1024 x 2^-24 = 6e-5 x a few ulps of the frequency"""
    from oracle.unet import timestep_embedding
    v = torch.tensor([0.0, 0.5, 1.0, 999.0, 1024.0])
    for dim in (2, 256, 320, 1280):
        assert float((timestep_embedding(v, dim).double() - _sincos64(v, dim)).abs().max()) < 1e-3


@pytest.mark.parametrize("rows", [1, 12, 257])
@pytest.mark.parametrize("dim", [2, 256, 320, 1280])
def test_sincos_embed_edges(dev, dim, rows):
    from consistentid_amd import ops
    what = f"I sincos_embed rows={rows} dim={dim}"
    v = torch.tensor([0.0, 0.5, 1.0, 999.0, 1024.0]).repeat(rows // 5 + 1)[:rows]
    if rows == 1:
        v = torch.tensor([1024.0])
    ref = _sincos64(v, dim)
    vd = _nanpad(v, dev)

    def launch():
        buf = _guarded(rows, dim, dev)
        ops.sincos_embed(vd, buf[GUARD:GUARD + rows], rows=rows, dim=dim)
        return buf
    buf = _twice(launch, what)
    check_close(buf[GUARD:GUARD + rows], ref, what, tol_l2=2e-3, tol_max=4e-3)
    _intact(buf, rows, 0, dim, what)


# ----------------------------------------------------------------------------- J. step_select
BYTE_SENTINEL, BYTE_GUARD = 0xa5, 64
# (offset in the row, bytes, misalignment of the destination).  0-2: sources 4 bytes off a 16-byte boundary (48 is on one,
# its destination is not): the narrow path.  3-5: the wide path with a 4-byte tail and no quad, a tail after two quads, and 2.5
# rounds of the 1024 lanes.  6: an aligned source with a destination 8 bytes off, 7: the reverse -- narrow both.
STEP_SEGS = [(4, 12, 4), (20, 24, 4), (48, 12, 4), (64, 4, 0), (80, 36, 0), (128, 40960, 0), (41088, 16, 8), (41108, 20, 0)]
STEP_ROW_BYTES = 41136          # a multiple of 16: every row keeps the alignments above


def _step_select(table, row_bytes, n_rows, counter, dsts, segs):
    from consistentid_amd import _lib, ops
    arr = (_lib.StepSeg * len(segs))(*[_lib.StepSeg(d.data_ptr(), o, n) for d, (o, n, _) in zip(dsts, segs)])
    _lib.check(_lib.load().cid_step_select(table.data_ptr(), row_bytes, n_rows, counter.data_ptr(), arr, len(segs), ops._stream()),
               "cid_step_select")


@pytest.mark.parametrize("n_rows", [5, 1])
def test_step_select_narrow_and_wide_paths(dev, n_rows):
    what = f"J step_select n_rows={n_rows}"
    assert STEP_ROW_BYTES % 16 == 0 and all(o % 4 == 0 and n % 4 == 0 and o + n <= STEP_ROW_BYTES for o, n, _ in STEP_SEGS)
    g = torch.Generator().manual_seed(n_rows)
    table = torch.randint(0, 256, (n_rows, STEP_ROW_BYTES), generator=g, dtype=torch.uint8)
    tabd = table.to(dev)
    assert tabd.data_ptr() % 16 == 0
    counter = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(start):
        bufs = [torch.full((2 * BYTE_GUARD + 16 + n,), BYTE_SENTINEL, dtype=torch.uint8, device=dev) for _, n, _ in STEP_SEGS]
        dsts = [b[BYTE_GUARD + mis:BYTE_GUARD + mis + n] for b, (_, n, mis) in zip(bufs, STEP_SEGS)]
        assert all(d.data_ptr() % 16 == mis for d, (_, _, mis) in zip(dsts, STEP_SEGS))
        counter.fill_(start)
        _step_select(tabd, STEP_ROW_BYTES, n_rows, counter, dsts, STEP_SEGS)
        torch.cuda.synchronize()
        return [b.cpu() for b in bufs], int(counter.item())

    for start in (-3, 0, n_rows - 1, n_rows + 4):
        row = min(max(start, 0), n_rows - 1)
        bufs, after = launch(start)
        again, after2 = launch(start)
        assert after == after2 == row + 1, f"{what}: counter {start} -> {after}, row {row} + 1 expected"
        for k, (b, b2, (o, n, mis)) in enumerate(zip(bufs, again, STEP_SEGS)):
            lo = BYTE_GUARD + mis
            assert torch.equal(b[lo:lo + n], table[row, o:o + n]), f"{what}: segment {k} from counter {start} is no copy of row {row}"
            assert bool((b[:lo] == BYTE_SENTINEL).all()) and bool((b[lo + n:] == BYTE_SENTINEL).all()), \
                f"{what}: bytes around the destination of segment {k} were written"
            assert torch.equal(b, b2), f"{what}: segment {k}: the second launch differs"
