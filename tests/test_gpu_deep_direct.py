"""The direct kernels of the 16 x 16 and 8 x 8 levels: cid_groupnorm_f16's single launch (gn_small_kernel,
csrc/norm.hip) on its 16-byte and 8-byte piece paths, and the self-attention dispatch's query-tile rule (csrc/attn.hip).

GroupNorm: every case against the fp64 reference at conftest.check_close's defaults (the tolerance of
test_gpu_direct_kernels.test_groupnorm_selections), launched twice for bit-identity, guard rows untouched, with and without
SiLU.  Self-attention: the cases of test_gpu_attention_edges (pitches ldq != ldk != ldo, guarded output, hostile padding
behind n_keys) at its ATTN_TOL, on grids below and above the device's CU count.

Two things the cases are NOT, and why:

* "just outside the single launch" is (1, 256, 1344, groups = 16), not (1, 256, 2688, groups = 32): both have cg = 84 and a
  slice of 21 504 elements at 256 pixels, but 2688 channels are above cid_groupnorm_f16's channel cap (GN_MAXC = 2560: the
  LDS arrays of the two-launch path), a refusal that tests/test_direct_kernels_host.py pins (2568 channels -> "bad
  groups/C").  test_groupnorm_refuses_2688_channels states that refusal for the shape itself.
* x = 30 + 0.5 randn does NOT separate a one-pass fp32 variance from the two-pass one at this tolerance.  Computed on the CPU
  before this file was written (B = 1, HW = 256, 1280 channels, cg = 40, 1024 lanes x 8 channels, wave butterfly, fp64 over the
  16 wave partials; rel_l2 / max_rel against the fp64 reference, fp16 outputs, tolerance 1e-3 / 4e-3):

      x = 30 + 0.5 randn    two-pass 2.07e-4 / 3.35e-4   one-pass, fp32 subtraction 2.59e-4 / 5.18e-4   fp64 subtraction 2.26e-4 / 4.20e-4
      ... with SiLU                  2.09e-4 / 3.67e-4                              2.78e-4 / 4.93e-4                    2.35e-4 / 4.45e-4
      x = 200 + 0.5 randn   two-pass 2.07e-4 / 3.59e-4   one-pass, fp32 subtraction 7.55e-3 / 1.58e-2   fp64 subtraction 3.81e-3 / 5.33e-3
      ... with SiLU                  2.09e-4 / 3.70e-4                              9.00e-3 / 1.44e-2                    4.55e-3 / 6.27e-3

  (mean / std)^2 x 2^-24 is 2e-4 at 30 / 0.5 -- the size of the output's own fp16 rounding -- and 1e-2 at 200 / 0.5.  The
  case at 30 stays (it is a valid input and must be right); the case at 200 is the one a single-pass variance fails."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from conftest import check_close
from gemm_parity import GUARD
from test_gpu_attention_edges import _self_attn_case
from test_gpu_direct_kernels import _gn_ref, _guarded, _intact, _rnd, _twice

pytestmark = pytest.mark.gpu

HEAD_DIMS = [160, 80, 40]


# ----------------------------------------------------------------------------- GroupNorm
def _gn_input(B, HW, C, seed):
    return _rnd(B, HW, C, seed=seed, scale=1.5) + _rnd(1, 1, C, seed=3)


def _gn_case(dev, what, x, c1, c2, groups, silu):
    from consistentid_amd import ops
    B, HW, C = x.shape
    assert C == c1 + c2
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


GN_DEEP_CASES = [
    # 16-byte pieces (cg % 8 == 0)
    (8, 256, 1280, 0, 32),          # the step's own shape, cg = 40: B % 8 == 0, the XCD-owning workgroup map
    (2, 64, 1280, 1280, 32),        # cg = 80, concat, slice of 5 120
    (1, 256, 2560, 0, 32),          # slice = 20 480 = GNS_MAXELEM exactly: every lane holds its last piece or none
    (2, 64, 1320, 1240, 32),        # cg = 80: group 16 (channels 1280 .. 1359) takes octets from both sources
    # 8-byte pieces
    (2, 64, 1280, 640, 32),         # cg = 60 (the 1280 + 640 concat)
    (3, 1, 128, 0, 32),             # cg = 4, one piece per slice; B % 8 != 0, the plain workgroup map
    (9, 16, 320, 320, 32),          # cg = 20
    # just outside the single launch: cg = 84, slice of 21 504 > GNS_MAXELEM at 256 pixels -> statistics + apply launches
    (1, 256, 1344, 0, 16),
    # partial last loads, cg = 40
    (2, 255, 1280, 0, 32),
    (2, 1, 1280, 0, 32),
]


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("B,HW,c1,c2,groups", GN_DEEP_CASES)
def test_groupnorm_deep_levels(dev, B, HW, c1, c2, groups, silu):
    what = f"deep groupnorm B={B} HW={HW} C={c1}+{c2} groups={groups} silu={silu}"
    _gn_case(dev, what, _gn_input(B, HW, c1 + c2, seed=HW + c1), c1, c2, groups, silu)


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("mean", [30.0, 200.0])
def test_groupnorm_mean_far_above_std(dev, mean, silu):
    """x = mean + 0.5 randn, cg = 40, HW = 256: the variance must come from a second pass over (x - mean).  The module
    docstring has the CPU figures: at mean = 200 a single fp32 pass of x and x^2 is 4 - 9 x over the tolerance, the two-pass
    form at 2.1e-4; at mean = 30 both forms are inside it, so that case checks the result only."""
    g = torch.Generator().manual_seed(7)
    x = (mean + 0.5 * torch.randn(2, 256, 1280, generator=g)).half()
    _gn_case(dev, f"deep groupnorm x = {mean:g} + 0.5 randn silu={silu}", x, 1280, 0, 32, silu)


def test_groupnorm_refuses_2688_channels(dev, lib):
    """(1, 256, 2688, groups = 32) -- cg = 84 at 32 groups -- is above the channel cap of cid_groupnorm_f16: refused on the
    host, nothing launched (tests/test_direct_kernels_host.py pins the cap at 2568 channels)"""
    from consistentid_amd import _lib, ops
    C = 2688
    x = torch.zeros(256, C, dtype=torch.float16, device=dev)
    buf = _guarded(256, C, dev)
    ws = torch.empty(ops.groupnorm_ws_bytes(1, C), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.CidError, match="bad groups/C"):
        ops.groupnorm(x, buf[GUARD:GUARD + 256], x[0], x[0], ws, B=1, HW=256, c1=C, groups=32)
    torch.cuda.synchronize()
    _intact(buf, 0, 0, 0, "refused groupnorm")


# ----------------------------------------------------------------------------- self-attention: 64 or 128 queries per workgroup
def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("N", [256, 128])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_self_attention_few_workgroups(dev, d, N):
    """B = heads = 1: one or two 128-query workgroups, far below the CU count -> the 64-query instance"""
    _self_attn_case(dev, d, N, N, heads=1, B=1)


def test_self_attention_step_shape(dev):
    """SD1.5's 16 x 16 level at CFG batch 8: 128 workgroups of 128 queries, 256 of 64"""
    assert (256 // 128) * 8 * 8 < _cus(dev), "this device has so few CUs that the step's shape stays on 128 queries"
    _self_attn_case(dev, 160, 256, 256, heads=8, B=8)


@pytest.mark.parametrize("n_keys", [128, 127], ids=["unmasked", "masked"])
@pytest.mark.parametrize("d", [32, 40, 64, 80, 160])
def test_self_attention_enough_workgroups(dev, d, n_keys):
    """N = 128, 8 heads and as many samples as give every CU a 128-query workgroup: that instance is still the one launched
    (the masked one too, at every head width: the cases of test_gpu_attention_edges at N = 256 have 12 - 16 workgroups and
    are on 64 queries now)"""
    B = -(-_cus(dev) // 8)
    _self_attn_case(dev, d, 128, n_keys, heads=8, B=B)


@pytest.mark.parametrize("N,n_keys", [(256, 255), (256, 65), (128, 127), (128, 65)])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_self_attention_masked_few_workgroups(dev, d, N, n_keys):
    _self_attn_case(dev, d, N, n_keys, heads=1, B=1)


@pytest.mark.parametrize("bq", ["64", "128"])
def test_self_attention_under_the_override(bq, dev):
    """CID_ATTN_BQ is read once per process: a fresh child per value.  64 takes the 64-query instance on a grid large enough
    for 128, 128 takes the 128-query instance on a grid too small for it (the parent rule); both at d = 160 and d = 80"""
    env = dict(os.environ, CID_ATTN_BQ=bq)
    p = subprocess.run([sys.executable, __file__, bq], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert f"override {bq} ok" in p.stdout


def _child(bq):
    assert os.environ.get("CID_ATTN_BQ") == bq
    from consistentid_amd import build
    build.build(verbose=False)
    dev = torch.device("cuda:0")
    big = -(-_cus(dev) // 8)
    for d in (160, 80):
        if bq == "64":
            _self_attn_case(dev, d, 128, 128, heads=8, B=big)
        else:
            _self_attn_case(dev, d, 256, 256, heads=1, B=1)
    print(f"override {bq} ok")


if __name__ == "__main__":
    _child(sys.argv[1])
