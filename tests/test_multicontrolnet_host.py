"""MultiControlNet without a GPU: cid_residual_accum_f16 is exported, bound and refuses bad arguments before any launch;
the guidance-window / keep-table / scale bookkeeping of the reference's MultiControlNet branches
(pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:139-149, :363-370, :397-398) as pure functions."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_symbol_is_declared_exported_and_bound(lib):
    from consistentid_amd import _lib
    src = (ROOT / "include" / "cid.h").read_text()
    names = set(re.findall(r"\b(cid_[a-z0-9_]+)\s*\(", src))
    assert "cid_residual_accum_f16" in names and "cid_residual_accum_f16" in _lib.SIGNATURES
    assert hasattr(lib, "cid_residual_accum_f16")
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)
    assert lib.cid_version() >= 106
    assert int(re.search(r"#define\s+CID_MAX_CONTROLNETS\s+(\d+)", src).group(1)) == _lib.MAX_CONTROLNETS == 4


def _segs(n_segs=1, n=64, nr=64, y=64, r=(128, 192, 256, 320)):
    from consistentid_amd._lib import AccumSeg
    segs = (AccumSeg * max(n_segs, 1))()
    for s in segs:
        s.y, s.n, s.nr = y, n, nr
        for k, a in enumerate(r):
            s.r[k] = a
    return segs


def test_residual_accum_refuses_bad_arguments_without_launching(lib):
    """every refusal is -22 with a message, decided on the host: the addresses are fake and no GPU is present"""
    call, err = lib.cid_residual_accum_f16, lib.cid_last_error
    SC = 4096                                                       # a fake non-null address for `scales`
    assert call(None, 1, 1, SC, None) == -22 and b"null pointer" in err()               # segs
    assert call(_segs(), 1, 1, None, None) == -22 and b"null pointer" in err()          # scales
    for n_segs in (0, 17, -1):
        assert call(_segs(max(n_segs, 1)), n_segs, 1, SC, None) == -22 and b"segments" in err()
    for n_nets in (0, 5, -1):
        assert call(_segs(), 1, n_nets, SC, None) == -22 and b"nets" in err()
    assert call(_segs(y=None), 1, 1, SC, None) == -22 and b"y is null" in err()
    for k in range(4):                                              # a null r[k] with k < n_nets, for every k and n_nets > k
        r = [128, 192, 256, 320]
        r[k] = None
        for n_nets in range(k + 1, 5):
            assert call(_segs(r=r), 1, n_nets, SC, None) == -22 and f"residual of net {k}".encode() in err()
    for n, nr in ((0, 8), (-8, 8), (12, 12), (64, 0), (64, -8), (64, 12), (64, 4), (64, 24), (8, 16)):
        assert call(_segs(n=n, nr=nr), 1, 1, SC, None) == -22 and b"multiples of 8" in err(), (n, nr)
    # the check reaches every segment, not only the first
    segs = _segs(16)
    segs[15].nr = 24
    assert call(segs, 16, 2, SC, None) == -22 and b"segment 15" in err()
    segs = _segs(3)
    segs[2].r[1] = None
    assert call(segs, 3, 2, SC, None) == -22 and b"segment 2" in err()
    # misaligned buffers (16-byte loads and stores)
    assert call(_segs(y=72), 1, 1, SC, None) == -22 and b"aligned" in err()
    assert call(_segs(r=(136, 192, 256, 320)), 1, 1, SC, None) == -22 and b"aligned" in err()


def test_front_end_refuses_cpu_tensors(lib):
    import torch
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    y = torch.zeros(16, dtype=torch.float16)
    with pytest.raises(CidError):
        ops.residual_accum([y], [[y.clone()]], torch.zeros(4))


def _ref_align(start, end, n_nets):
    """CN :139-149, verbatim but for the names"""
    if not isinstance(start, list) and isinstance(end, list):
        start = len(end) * [start]
    elif not isinstance(end, list) and isinstance(start, list):
        end = len(start) * [end]
    elif not isinstance(start, list) and not isinstance(end, list):
        start, end = n_nets * [start], n_nets * [end]
    return start, end


def _ref_keep(n, starts, ends):
    """CN :363-370 for a MultiControlNetModel"""
    return [[1.0 - float(i / n < s or (i + 1) / n > e) for s, e in zip(starts, ends)] for i in range(n)]


@pytest.mark.parametrize("n_nets", [1, 2, 3])
def test_guidance_alignment_and_keep_table_follow_the_reference(n_nets):
    from consistentid_amd.controlnet import align_control_guidance, controlnet_keep_table
    lists = {1: ([0.2], [0.9]), 2: ([0.0, 0.25], [0.75, 1.0]), 3: ([0.0, 0.3, 0.5], [0.4, 0.8, 1.0])}[n_nets]
    cases = [(0.0, 1.0), (0.1, 0.6), (lists[0], 0.9), (0.05, lists[1]), lists]       # float/float, list/float, float/list, list/list
    for start, end in cases:
        s, e = align_control_guidance(start, end, n_nets)
        rs, re_ = _ref_align(start, end, n_nets)
        assert (s, e) == ([float(v) for v in rs], [float(v) for v in re_]) and len(s) == len(e) == n_nets
        for steps in (1, 4, 7, 50):
            assert controlnet_keep_table(steps, s, e) == _ref_keep(steps, rs, re_)
    # tuples count as lists
    assert align_control_guidance(tuple(lists[0]), 1.0, n_nets) == align_control_guidance(lists[0], 1.0, n_nets)
    # a strength < 1 window: the skipped schedule entries come first, as zeros, and the windows count executed steps only
    s, e = align_control_guidance(lists[0], lists[1], n_nets)
    tab = controlnet_keep_table(4, s, e, first_step=3)
    assert tab[:3] == [[0.0] * n_nets] * 3 and tab[3:] == _ref_keep(4, s, e)


def _active_sets(windows, steps=4):
    from consistentid_amd.controlnet import active_nets, align_control_guidance, controlnet_keep_table
    s, e = align_control_guidance([w[0] for w in windows], [w[1] for w in windows], len(windows))
    return [set(active_nets(row)) for row in controlnet_keep_table(steps, s, e)]


def test_active_sets_of_two_windows():
    assert _active_sets([(0, .75), (.25, 1)]) == [{0}, {0, 1}, {0, 1}, {1}]
    assert _active_sets([(0, .5), (.75, 1)]) == [{0}, {0}, set(), {1}]


def test_scale_broadcast_and_length_mismatches():
    from consistentid_amd.controlnet import (HipMultiControlNet, align_control_guidance, broadcast_conditioning_scale,
                                             check_controlnet_count)
    assert broadcast_conditioning_scale(0.5, 3) == [0.5, 0.5, 0.5]
    assert broadcast_conditioning_scale(1, 1) == [1.0]
    assert broadcast_conditioning_scale([0.5, 0.8], 2) == [0.5, 0.8]
    assert broadcast_conditioning_scale((1, 0.2), 2) == [1.0, 0.2]
    with pytest.raises(ValueError, match="3 entries for 2 ControlNets"):
        broadcast_conditioning_scale([0.1, 0.2, 0.3], 2)
    with pytest.raises(ValueError, match="1 entries for 2 ControlNets"):
        broadcast_conditioning_scale([0.1], 2)
    with pytest.raises(ValueError, match="2 entries, control_guidance_end has 3"):
        align_control_guidance([0.0, 0.1], [1.0, 1.0, 1.0], 2)
    with pytest.raises(ValueError, match="3 entries for 2 ControlNets"):
        align_control_guidance([0.0, 0.1, 0.2], 1.0, 2)                 # a float beside a list of the wrong length
    with pytest.raises(ValueError, match="1 entries for 2 ControlNets"):
        align_control_guidance(0.0, [1.0], 2)
    with pytest.raises(ValueError, match="3 entries for 2 ControlNets"):
        align_control_guidance([0.0, 0.1, 0.2], [1.0, 1.0, 1.0], 2)
    # N = 5 (and N = 0): refused by the count alone, before any net is looked at or loaded
    with pytest.raises(ValueError, match="5 ControlNets: a MultiControlNet takes 1..4"):
        HipMultiControlNet([object()] * 5)
    with pytest.raises(ValueError, match="0 ControlNets"):
        HipMultiControlNet([])
    with pytest.raises(ValueError, match="5 ControlNets"):
        check_controlnet_count(5)
    from consistentid_amd import loader
    with pytest.raises(ValueError, match="5 ControlNets"):
        loader.load_controlnet(["a", "b", "c", "d", "e"])
    with pytest.raises(TypeError, match="expected HipControlNet"):
        HipMultiControlNet([object()])
