"""Upsample2D as four 2x2 phase convolutions (cid_gemm_desc.w_up4, csrc/conv3x3.hip phase mode) -- what can be checked
without a GPU: the identity itself, the tile plan, and the loader / compute schedule for four taps per channel slab."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel, rel_l2
from upconv_ref import fold_ref, phase_conv_ref

# One fp16 rounding has a relative error of at most 2^-11, ~2^-11 / sqrt(3) = 2.8e-4 rms for a uniformly spread mantissa.
# Both arms round the output once; the folded arm also rounds the summed weights once (independent errors):
RMS1 = 2.0 ** -11 / 3 ** 0.5
TOL_NINE = 1.2 * RMS1                    # 3.4e-4: one rounding, 20 % slack for the non-uniform mantissa distribution
TOL_FOLD = 1.2 * (2 * RMS1 ** 2) ** 0.5  # 4.8e-4: two independent roundings


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 64, 8, 8), (2, 320, 640, 32, 32), (1, 640, 640, 32, 32), (1, 1280, 1280, 16, 16),
                                            (2, 64, 96, 6, 10), (1, 32, 64, 12, 4)])
def test_four_phase_convolutions_are_the_upsampled_convolution(B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Cin, H, W, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).half()
    bias = torch.randn(Cout, generator=g).half()
    w9 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), bias.double(), padding=1)
    # folded weights kept in fp32: the decomposition is exact up to fp32 round-off
    exact = phase_conv_ref(x, fold_ref(w9, round_fp16=False), bias)
    e = rel_l2(exact, ref)
    print(f"[fold] fp32 fold {Cin}->{Cout} {H}x{W}: rel_l2={e:.3e}")
    assert e < 2e-6
    # rounded to fp16 once (what the kernel multiplies), output rounded to fp16: the arithmetic of the GPU path
    nine = rel_l2(F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), bias.float(), padding=1).half(), ref)
    got = phase_conv_ref(x, fold_ref(w9), bias).half()
    e2, em = rel_l2(got, ref), max_rel(got, ref)
    print(f"[fold] fp16 fold {Cin}->{Cout} {H}x{W}: nine taps rel_l2={nine:.3e}, folded rel_l2={e2:.3e} max_rel={em:.3e}")
    assert nine <= TOL_NINE and e2 <= TOL_FOLD and em <= 4e-3


def test_fold_sums_in_the_documented_order():
    w9 = torch.arange(9, dtype=torch.float32).reshape(1, 9, 1).repeat(2, 1, 3).reshape(2, 27).half()      # tap t holds the value t
    w4 = fold_ref(w9).float().reshape(2, 2, 2, 2, 2, 3)[..., 0]       # [py][px][n][ry][rx]
    assert w4[0, 0, 0].tolist() == [[0, 1 + 2], [3 + 6, 4 + 5 + 7 + 8]]
    assert w4[1, 1, 1].tolist() == [[0 + 1 + 3 + 4, 2 + 5], [6 + 7, 8]]
    assert w4[0, 1, 0].tolist() == [[0 + 1, 2], [3 + 4 + 6 + 7, 5 + 8]]
    assert w4[1, 0, 0].tolist() == [[0 + 3, 1 + 2 + 4 + 5], [6, 7 + 8]]


def test_tile_plan_with_folded_weights(lib):
    from consistentid_amd._lib import GemmDesc
    assert lib.cid_version() >= 103
    assert C.sizeof(GemmDesc) % 8 == 0 and GemmDesc.w_up4.offset == C.sizeof(GemmDesc) - 8      # the trailing pointer

    def desc(B, side, cin, cout, fold=True, **kw):
        d = GemmDesc()
        d.x1, d.w, d.out = 64, 64, 64
        d.c1, d.ld1, d.ldo, d.N, d.taps = cin, cin, cout, cout, 9
        d.M = B * 4 * side * side
        d.Hi, d.Wi, d.Ho, d.Wo, d.stride, d.up = side, side, 2 * side, 2 * side, 1, 1
        d.ws, d.ws_bytes = 64, 64 << 20
        if fold:
            d.w_up4 = 64
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    rows = lambda *a, **kw: lib.cid_gemm_stats_rows(C.byref(desc(*a, **kw)))
    assert rows(8, 32, 640, 640) == 256 and rows(8, 32, 640, 640, fold=False) == 256
    assert rows(8, 16, 1280, 1280) == 256 and rows(8, 16, 1280, 1280, fold=False) == 256
    assert rows(4, 64, 640, 640) == 256          # SDXL 64 -> 128: a 396-row halo
    assert rows(4, 32, 1280, 1280) == 256        # SDXL 32 -> 64
    assert rows(2, 32, 320, 640) == 128          # 128-token tiles, five channel slabs
    assert rows(8, 8, 1280, 1280) == 0           # 8 -> 16: 64 tiles, split-K from the nine taps
    # w_up4 is refused off the Upsample2D convolution (the plan fails: no statistics, and cid_gemm_f16 returns -22)
    for bad in (dict(up=0, Ho=32, Wo=32, M=8 * 1024), dict(mode=2), dict(res=64, ldr=640)):
        d = desc(8, 32, 640, 640, **bad)
        assert lib.cid_gemm_stats_rows(C.byref(d)) == 0
        assert lib.cid_gemm_f16(C.byref(d), None) == -22
        assert b"w_up4" in lib.cid_last_error()


# ---- loader / compute schedule of the phase mode, replayed as tests/test_conv3x3_schedule.py does for nine taps -------------
# Four slabs per channel slab; the ring stage of slab k = cs * 4 + tap is k % 3 (the kernel unrolls three channel slabs so
# that it is a compile-time number); the 13 halo slots of a loader are issued seven per window in windows 0 and 1.
WQ, NSTG, NT, HQ = 5, 3, 4, 13
HPW = (HQ + NT - 3) // (NT - 2)


def hcount(nq, tap):
    return 0 if tap > NT - 3 else max(0, min(HPW, nq - HPW * tap))


def loader_program(ncs, nq, miscount=0, ahead=2):
    ev = [("dma", "halo", 0, ("hbuf", 0))] * nq
    for tap in (0, 1):
        ev += [("dma", "w", tap, ("stage", tap % NSTG))] * WQ
    ev += [("wait_vm", WQ), ("bar",)]
    for cs in range(ncs):
        last = cs + 1 >= ncs
        for tap in range(NT):
            k = cs * NT + tap + ahead
            tgt = k if k < ncs * NT else None
            if tgt is not None:
                ev += [("dma", "w", tgt, ("stage", tgt % NSTG))] * WQ
            if not last and tap <= NT - 3:
                for q in range(HPW * tap, HPW * tap + HPW):
                    if q < min(nq, HQ):
                        ev.append(("dma", "halo", cs + 1, ("hbuf", (cs + 1) & 1)))
            n = (WQ if (tap + 2 < NT or not last) else 0) + (0 if last else hcount(nq, tap))
            if tap >= 1:
                n += 0 if last else hcount(nq, tap - 1)
            ev += [("wait_vm", n + miscount), ("bar",)]
    ev.append(("wait_vm", 0))
    return ev


def compute_program(ncs):
    ev = [("bar",), ("read", 0, 0)]
    for k in range(ncs * NT):
        ev += [("read", k, 1), ("mma", k, 0), ("read", k, 2), ("mma", k, 1), ("read", k, 3), ("mma", k, 2), ("wait_reads",), ("bar",)]
        if k + 1 < ncs * NT:
            ev.append(("read", k + 1, 0))
        ev.append(("mma", k, 3))
    return ev


def intervals(ev):
    out, cur = [], []
    for e in ev:
        if e[0] == "bar":
            out.append(cur)
            cur = []
        else:
            cur.append(e)
    out.append(cur)
    return out


def check(loaders, compute, ncs):
    liv, civ = [intervals(p) for p in loaders], intervals(compute)
    assert {len(iv) for iv in liv} == {len(civ)}, "loaders and compute waves execute different barrier counts"
    landed, issued = [], []
    for iv in liv:
        queue, land, log = [], {}, []
        for i, evs in enumerate(iv):
            for e in evs:
                if e[0] == "dma":
                    queue.append((e[1], e[2]))
                    log.append((i, e[1], e[2], e[3]))
                elif e[0] == "wait_vm":                      # vmcnt retires in issue order: all but the youngest n
                    while len(queue) > e[1]:
                        land[queue.pop(0)] = i
        assert not queue, "DMA still in flight at the end of the loop"
        landed.append(land)
        issued.append(log)
    have, last_read = set(), {}
    for i, evs in enumerate(civ):
        for e in evs:
            if e[0] == "read":
                k, j = e[1], e[2]
                for ld in landed:
                    assert ("w", k) in ld and ld[("w", k)] < i, f"W{k} read in interval {i} before a loader retired it"
                    if ("halo", k // NT) in ld:
                        assert ld[("halo", k // NT)] < i, f"halo {k // NT} read in interval {i} before a loader retired it"
                have.add((k, j))
                last_read[("stage", k)] = i
                last_read[("hbuf", k // NT)] = i
            elif e[0] == "mma":
                assert (e[1], e[2]) in have, f"slab {e[1]} k-step {e[2]} multiplied before it was read"
    assert have == {(k, j) for k in range(ncs * NT) for j in range(4)}
    for evs in civ[1:-1]:
        if any(e[0] == "read" for e in evs):
            assert ("wait_reads",) in evs, "reads in flight across a barrier"
    for log in issued:
        for i, kind, key, region in log:
            if kind == "w":
                assert region == ("stage", key % NSTG)
                if key >= NSTG:
                    assert last_read[("stage", key - NSTG)] < i, f"W{key} overwrites the stage of slab {key - NSTG} while it is read"
            elif kind == "halo" and key >= 2:
                assert last_read[("hbuf", key - 2)] < i, f"halo {key} overwrites channel slab {key - 2}'s while it is read"
    return len(civ)


@pytest.mark.parametrize("ncs", list(range(1, 21)))
def test_phase_mode_protocol_is_legal(ncs):
    # halo pieces of the UNets' launches: 340 rows (32 -> 64: 43 pieces), 324 (16 -> 32: 41), 396 (SDXL 64 -> 128: 50) on
    # 256-token tiles, 204 rows (26 pieces) on 128-token tiles: slots per loader (pieces lw, lw + 4, ...)
    for pieces in (43, 41, 50, 26):
        slots = [(pieces - lw + 3) // 4 for lw in range(4)]
        assert max(slots) <= HQ
        nb = check([loader_program(ncs, nq) for nq in slots], compute_program(ncs), ncs)
        assert nb == NT * ncs + 2


def test_the_checker_catches_a_wrong_count_and_an_early_refill():
    with pytest.raises(AssertionError, match="before a loader retired it"):
        check([loader_program(2, 13, miscount=1)] + [loader_program(2, 12)] * 3, compute_program(2), 2)
    with pytest.raises(AssertionError):
        check([loader_program(3, 13, ahead=3)] * 4, compute_program(3), 3)
