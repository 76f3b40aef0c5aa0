"""Upsample2D's convolution as four 2x2 phase convolutions (cid_gemm_desc.w_up4): the native weight fold and the phase mode
of csrc/conv3x3.hip on the GPU, against the fp32 reference and against the nine-tap path on the same inputs."""
import pytest
import torch
import torch.nn.functional as F

from conftest import check_close, rel_l2
from upconv_ref import fold_ref

pytestmark = pytest.mark.gpu


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def _tok(x):   # NCHW -> [B*HW, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


@pytest.mark.parametrize("N,C", [(64, 64), (640, 320), (1280, 1280), (96, 32)])
def test_native_fold_equals_the_restatement_bit_for_bit(dev, N, C):
    from consistentid_amd import ops
    w9 = rnd(N, 9 * C, seed=11, scale=(9 * C) ** -0.5)
    w9[0, :9] = torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, 65504.0, 6e-8, -6e-8, 0.333])      # signed zeros, overflow, subnormals
    got = ops.upconv_fold(w9.to(dev))
    torch.cuda.synchronize()
    want = fold_ref(w9)
    assert got.shape == want.shape
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


# every up = 1 row of test_gpu_kernels.py::test_gemm_conv3x3 on the 160-channel grid, and SDXL's two Upsample2D convolutions
# at CFG batch 4; `folded`: the launch is expected on the phase mode (one source, tiles that fill the chip)
@pytest.mark.parametrize("B,C1,C2,Cout,H,folded", [
    (8, 640, 0, 640, 32, True),        # 32 -> 64: 512 tiles of 256 input pixels (eight input rows)
    (8, 1280, 0, 1280, 16, True),      # 16 -> 32: a tile = one whole input image of one parity
    (2, 320, 0, 640, 32, True),        # 128-token tiles (four input rows)
    (3, 320, 320, 320, 32, False),     # two sources: the nine-tap path serves
    (4, 640, 0, 640, 64, True),        # SDXL 64 -> 128 (396-row halo)
    (4, 1280, 0, 1280, 32, True),      # SDXL 32 -> 64
])
def test_upconv_phase_mode(dev, B, C1, C2, Cout, H, folded):
    from consistentid_amd import ops, weights
    Wd = H
    x1 = rnd(B, C1, H, Wd, seed=1)
    x2 = rnd(B, C2, H, Wd, seed=2) if C2 else None
    w = rnd(Cout, C1 + C2, 3, 3, seed=3, scale=(9 * (C1 + C2)) ** -0.5)
    b = rnd(Cout, seed=4)
    xin = torch.cat([x1, x2], 1).float() if C2 else x1.float()
    ref = F.conv2d(F.interpolate(xin, scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
    Ho, Wo = 2 * H, 2 * Wd
    M, HW = B * Ho * Wo, Ho * Wo
    w9 = weights._conv3(w, dev)
    w4 = ops.upconv_fold(w9)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    xa, xb, bd = _tok(x1).to(dev), (_tok(x2).to(dev) if C2 else None), b.to(dev)

    def run(fold, out2=None):
        out = torch.empty(M, Cout, dtype=torch.float16, device=dev)
        ops.gemm(xa, w9, out, M=M, N=Cout, c1=C1, x2=xb, c2=C2, bias=bd, taps=9, Hi=H, Wi=Wd, Ho=Ho, Wo=Wo, stride=1, up=1,
                 ws=ws, gn_hw=HW, out2=out2, w_up4=w4 if fold else None)
        return out

    nine = run(False)
    o2 = torch.zeros(M, Cout, dtype=torch.float16, device=dev)
    out = run(True, out2=o2)
    torch.cuda.synchronize()
    what = f"upconv fold B{B} C{C1}+{C2}->{Cout} H{H}"
    check_close(out, _tok(ref), what)
    check_close(nine, _tok(ref), what + " (nine taps)")
    d = rel_l2(out, nine)
    print(f"[parity] {what}: folded vs nine taps rel_l2={d:.3e}")
    # both sit within ~2.5e-4 of the reference (one fp16 rounding of the output, one of the summed weights)
    assert d <= 5e-4
    assert torch.equal(out, nine) == (not folded), "the launch did not take the expected path"
    assert torch.equal(o2, out), "out2 differs from out"
    for _ in range(3):                        # bit-stable (fixed summation order, no atomics)
        again = run(True)
        torch.cuda.synchronize()
        assert torch.equal(again, out)
    # GroupNorm statistics of the written tensor, as test_gpu_kernels.py checks them for the stride-1 convolutions
    if not folded and not hasattr(out, "_gn_stats"):
        return      # (the two-source row runs split-K from the nine taps, with or without w_up4: no statistics to check)
    assert hasattr(out, "_gn_stats"), "this launch was expected to emit statistics"
    st, rows = out._gn_stats
    u = Cout // 32
    o = out.double().cpu().reshape(M // rows, rows, 32, u)
    if folded:
        # a statistics block is a tile: `rows` outputs of ONE parity of one image (image-major: image, parity, block)
        o = out.double().cpu().reshape(B, H, 2, Wd, 2, Cout).permute(0, 2, 4, 1, 3, 5).reshape(M // rows, rows, 32, u)
    want = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
    err = ((st.double().cpu() - want).abs() / (want.abs() + rows * u * 1e-3)).max()
    assert err < 2e-5, f"statistics differ from the tensor they describe: {err:.2e}"
    g, be = (1 + 0.1 * rnd(Cout, seed=6).float()).half(), rnd(Cout, seed=7, scale=0.1)
    gref = F.silu(F.group_norm(out.double().cpu().reshape(B, HW, Cout).transpose(1, 2), 32, g.double(), be.double(), 1e-5)).transpose(1, 2)
    gws = torch.zeros(ops.groupnorm_ws_bytes(B, Cout), dtype=torch.uint8, device=dev)
    y = torch.empty_like(out)
    ops.groupnorm(out, y, g.to(dev), be.to(dev), gws, B=B, HW=HW, c1=Cout, groups=32, eps=1e-5, silu=True)
    torch.cuda.synchronize()
    check_close(y.reshape(B, HW, Cout), gref, f"GroupNorm on the statistics of {what}")
    for _ in range(3):
        again = run(True)
        torch.cuda.synchronize()
        assert torch.equal(again._gn_stats[0], st)
