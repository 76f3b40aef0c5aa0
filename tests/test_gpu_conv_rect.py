"""The fast 3x3 convolution kernels (igemm_halo of csrc/gemm.hip, conv_h32 and conv_h32_phase of csrc/conv3x3.hip) on
non-square images.

The census (tests/golden/gemm_calls.json) reaches these families on square images only: its non-square workloads have image
rows of 96, 48, 24, 108, 54 or 27 pixels, which never satisfy the whole-row tile rule of route_halo / route_conv3x3, and the
variant key does not encode geometry.  A pipeline does reach them at ``H != W`` when the row width is a power of two (SD1.5
at 768 x 512: 96 x 64 latents), and every one of them derives halo geometry, tile-to-image mapping, the phase mode's output
scatter and the statistics-block order from W, H, HW, seg / W and y0 -- a swapped H and W there is invisible on a square.

``RECT`` lists, per fast variant key of the census, shapes ``(B, Hi, Wi)`` with Hi > Wi ("tall") and Wi > Hi ("wide").  A
case is the key's census record with only the geometry replaced (``rect_record``); it must still plan to the key (a case that
falls to the gather kernel fails), runs the census parity body (tests/gemm_parity.py) and, where the launch emits GroupNorm
statistics, feeds them to ops.groupnorm and compares with F.group_norm in fp64 of the tensor the kernel wrote.
tests/test_gemm_plan_host.py holds the table to the census without a GPU."""
import time

import pytest
import torch
import torch.nn.functional as F

import gemm_census
import gemm_parity
from conftest import check_close

pytestmark = pytest.mark.gpu

KEYS = gemm_census.keys_of(gemm_census.all_records(gemm_census.load()))

_H32, _PH, _HALO = "conv_h32-{}x160-nb0-m0-t9-s1-u0-p0-", "conv_h32_phase-{}x160-nb0-m0-t9-s1-u1-p0-folded-", "igemm_halo-256x160-nb0-m0-t9-s1-u0-p0-sk-"
# the halo kernel gets two shapes per orientation: with HW < 256 a tile holds several whole images, with HW >= 256 it is a run
# of whole rows of one image -- different index paths under one variant key
_HALO_TALL, _HALO_WIDE = ((8, 16, 4), (2, 32, 16)), ((8, 4, 16), (2, 16, 32))
# key: (tall shapes, wide shapes), each (B, Hi, Wi).  96 x 64 and 32 x 128 are the level-0 latents of SD1.5 at 768 x 512 and
# of SDXL at 256 x 1024; the largest case is M = 8 * 96 * 64 = 49152, 320 -> 320
RECT = {
    _H32.format(128) + "bias-res-stats": (((2, 96, 64),), ((4, 32, 128),)),                 # 640 -> 640
    _H32.format(128) + "bias-res-stats-out2": (((4, 96, 64),), ((4, 32, 128),)),            # 320 -> 320
    _H32.format(128) + "bias-rowbias": (((16, 32, 8),), ((16, 8, 32),)),                    # 640 -> 1280
    _H32.format(128) + "bias-rowbias-stats": (((8, 48, 32),), ((8, 16, 64),)),              # 320 -> 640
    _H32.format(256) + "bias-res-stats": (((8, 96, 64),), ((16, 32, 64),)),                 # 320 -> 320
    _H32.format(256) + "bias-res-stats-out2": (((8, 96, 64),), ((16, 32, 64),)),
    _H32.format(256) + "bias-rowbias-stats": (((4, 96, 64),), ((8, 32, 64),)),              # 320 -> 640
    _PH.format(128) + "bias-stats": (((2, 48, 32),), ((2, 16, 64),)),                       # 640 -> 640, Upsample2D
    _PH.format(256) + "bias-stats": (((8, 32, 8),), ((8, 8, 32),)),                         # 1280 -> 1280, Upsample2D
    _HALO + "bias-res": (_HALO_TALL, _HALO_WIDE),                                           # 1280 -> 1280
    _HALO + "bias-rowbias": (_HALO_TALL, _HALO_WIDE),
}


def rect_record(rec: dict, B: int, Hi: int, Wi: int) -> dict:
    """``rec`` at another geometry: Hi, Wi, Ho, Wo, M, gn_hw (where set) and the rows of the recorded number of samples per
    time row; channels, pitches, operand presence and ws_bytes as recorded"""
    assert rec["taps"] == 9 and rec["stride"] == 1 and rec["M"] % (rec["Ho"] * rec["Wo"]) == 0
    hw_old = rec["Ho"] * rec["Wo"]
    Ho, Wo = Hi << rec["up"], Wi << rec["up"]
    new = dict(rec, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, M=B * Ho * Wo)
    if rec["gn_hw"]:
        new["gn_hw"] = Ho * Wo
    if rec["has_rowbias"]:
        assert rec["rows_per_sample"] % hw_old == 0
        new["rows_per_sample"] = rec["rows_per_sample"] // hw_old * Ho * Wo
    return new


def rect_plan(key: str, shape) -> tuple:
    """-> (the derived record, its plan now, the variant key of that plan)"""
    rec = rect_record(KEYS[key][0], *shape)
    plan = dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(rec)))
    return rec, plan, gemm_census.variant_key(rec, plan)


CASES = [(key, shape) for key, (tall, wide) in RECT.items() for shape in tall + wide]


@pytest.mark.parametrize("key,shape", CASES, ids=[f"{k}-{b}x{h}x{w}" for k, (b, h, w) in CASES])
def test_rect_parity(dev, key, shape):
    from consistentid_amd import _lib, ops
    t0 = time.time()
    B, Hi, Wi = shape
    assert Hi != Wi
    rec, plan, now = rect_plan(key, shape)
    # 1. the derived geometry stays on this variant (family, tile, epilogue operands)
    assert now == key, f"(B, Hi, Wi) = {shape} leaves the variant: {now}\n{rec}\n{plan}"
    fam = gemm_census.families()[plan["family"]]
    print(f"[rect] {key} (B, Hi, Wi) = {shape}: family {fam}, {plan['bm']}x{plan['bn']} tiles, split-K {plan['splitk']}")
    # 2. the census parity body
    got, stats = gemm_parity.run_case(dev, key, rec, plan)
    # 3. the statistics through their consumer (as test_gpu_upconv_fold.test_upconv_phase_mode does on squares)
    if plan["stats"]:
        N, HW = rec["N"], rec["Ho"] * rec["Wo"]
        assert stats is not None and _lib.load().cid_groupnorm_stats_ok(N, 0, 32), "the GroupNorm would not read these statistics"
        x = got.contiguous()
        x._gn_stats = stats
        g, be = (1 + 0.1 * gemm_parity._rnd(N, seed=6).float()).half(), gemm_parity._rnd(N, seed=7, scale=0.1)
        gref = F.silu(F.group_norm(x.double().cpu().reshape(B, HW, N).transpose(1, 2), 32, g.double(), be.double(), 1e-5)).transpose(1, 2)
        gws = torch.zeros(ops.groupnorm_ws_bytes(B, N), dtype=torch.uint8, device=dev)
        y = torch.empty_like(x)
        ops.groupnorm(x, y, g.to(dev), be.to(dev), gws, B=B, HW=HW, c1=N, groups=32, eps=1e-5, silu=True)
        torch.cuda.synchronize()
        check_close(y.reshape(B, HW, N), gref, f"GroupNorm on the statistics of {key} {shape}")
    print(f"[rect] {key} {shape}: {time.time() - t0:.1f} s")
