"""The long-context cross-attention entries (csrc/xattn_long.hip) without a GPU: declared, exported and bound; every argument
refusal comes back before any launch; cid_kv_pack_long_elems against the numpy model of the header's index formula
(tests/long_attention_ref.py); and the engine's launch-sequence strings for contexts up to 96 rows are the ones they were."""
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import long_attention_ref as lr

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("cid_id_xattn_long_f16", "cid_kv_pack_long_f16", "cid_kv_pack_long_elems", "cid_xattn_long_max_txt")
HEAD_CONFIGS = [(64, 2), (128, 2), (320, 8), (640, 8), (1280, 8), (640, 10), (1280, 20)]       # CID_XATTN_CONFIGS' (C, heads)


def test_entries_declared_exported_bound(lib):
    from consistentid_amd import _lib, ops, prompt_weighting
    header = (ROOT / "include" / "cid.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/cid.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.cid_version() >= 110
    cap = int(re.search(r"#define\s+CID_XATTN_LONG_MAX_TXT\s+(\d+)", header).group(1))
    cap_ip = int(re.search(r"#define\s+CID_XATTN_LONG_MAX_IP\s+(\d+)", header).group(1))
    assert cap >= 1024 and lib.cid_xattn_long_max_txt() == cap == ops.xattn_long_max_txt() == prompt_weighting.MAX_TEXT_ROWS
    assert cap_ip == ops.XATTN_LONG_MAX_IP == 32
    for name in ("kv_pack_long", "kv_pack_long_elems", "id_xattn_long"):
        assert callable(getattr(ops, name))
    assert "xattn_long.hip" in __import__("consistentid_amd.build", fromlist=["SOURCES"]).SOURCES


def test_core_refusals_before_any_launch(lib):
    """(no GPU here: anything that got as far as a launch would fail differently, with -5)"""
    err = lib.cid_last_error
    ok = dict(q=64, out=64, kp=64, vp=64, kvrow=64, B=2, N=64, C=320, heads=8, n_txt=154, n_ip=4)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cid_id_xattn_long_f16(a["q"], a["out"], a["kp"], a["vp"], a["kvrow"], a["B"], a["N"], a["C"], a["heads"],
                                         a["n_txt"], a["n_ip"], 1.0, None)

    for ptr in ("q", "out", "kp", "vp", "kvrow"):
        assert call(**{ptr: None}) == -22 and b"cid_id_xattn_long_f16: null pointer" in err(), ptr
    for bad in (dict(B=0), dict(N=0), dict(heads=0), dict(C=0), dict(C=324)):
        assert call(**bad) == -22 and b"cid_id_xattn_long_f16: bad shape" in err(), bad
    for N in (48, 33, 31):
        assert call(N=N) == -22 and b"multiple of 32" in err()
    for C, heads in ((384, 8), (128, 8), (1024, 8), (96, 1)):          # head widths 48, 16, 128, 96
        assert call(C=C, heads=heads) == -22 and b"no kernel for head_dim" in err(), (C, heads)
    for n_txt in (0, -1, 1025, 4096):
        assert call(n_txt=n_txt) == -22 and b"1 to 1024 text rows" in err(), n_txt
    for n_ip in (-1, 33, 77):
        assert call(n_ip=n_ip) == -22 and b"0 to 32 ID rows" in err(), n_ip


def test_pack_refusals_before_any_launch(lib):
    err = lib.cid_last_error
    ok = dict(kv_txt=64, kv_ip=64, kp=64, vp=64, R=2, C=320, heads=8, n_txt=154, n_ip=4)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cid_kv_pack_long_f16(a["kv_txt"], a["kv_ip"], a["kp"], a["vp"], a["R"], a["C"], a["heads"], a["n_txt"],
                                        a["n_ip"], None)

    for ptr in ("kv_txt", "kv_ip", "kp", "vp"):
        assert call(**{ptr: None}) == -22 and b"cid_kv_pack_long_f16: null pointer" in err(), ptr
    for bad in (dict(R=0), dict(heads=0), dict(C=324), dict(C=36, heads=3), dict(C=0)):
        assert call(**bad) == -22 and b"cid_kv_pack_long_f16: bad C/heads" in err(), bad
    for n_txt in (0, 1025):
        assert call(n_txt=n_txt) == -22 and b"1 to 1024 text rows" in err()
    for n_ip in (-1, 33):
        assert call(n_ip=n_ip) == -22 and b"0 to 32 ID rows" in err()
    for bad in ((320, 0, 154, 4), (320, 7, 154, 4), (320, 8, 0, 4), (320, 8, 1025, 4), (320, 8, 154, 33), (320, 8, 154, -1)):
        assert lib.cid_kv_pack_long_elems(*bad, 0) == -22 and lib.cid_kv_pack_long_elems(*bad, 1) == -22, bad


def test_a_context_without_id_rows_may_use_the_id_tile_for_text(lib):
    """a ControlNet is handed a pipeline's text AND ID rows as one text stream with n_ip = 0: 1024 text rows + 4 ID rows must
    not be refused there.  Without ID rows the text may fill the ID tile's 32 slots too -- 33 key tiles at the most either
    way, so no packed image grows beyond that of (1024, 32)."""
    err = lib.cid_last_error
    cap, ip = lib.cid_xattn_long_max_txt(), 32
    for C, heads in ((1280, 8), (64, 2)):
        biggest = [lib.cid_kv_pack_long_elems(C, heads, cap, ip, w) for w in (0, 1)]
        for n_txt in (cap + 4, cap + ip):
            got = [lib.cid_kv_pack_long_elems(C, heads, n_txt, 0, w) for w in (0, 1)]
            assert got == list(lr.long_elems(C, heads, n_txt, 0)) == biggest, (C, heads, n_txt, got)
        assert lib.cid_kv_pack_long_elems(C, heads, cap + ip + 1, 0, 0) == -22
        assert lib.cid_kv_pack_long_elems(C, heads, cap + 1, 1, 0) == -22
    # the entries: refused one row later, with the limit that holds in the message; (cap + 4, 0) gets as far as the launch
    assert lib.cid_id_xattn_long_f16(64, 64, 64, 64, 64, 2, 64, 320, 8, cap + ip + 1, 0, 1.0, None) == -22
    assert f"1 to {cap + ip} text rows".encode() in err()
    assert lib.cid_kv_pack_long_f16(64, 64, 64, 64, 2, 320, 8, cap + ip + 1, 0, None) == -22
    assert f"1 to {cap + ip} text rows".encode() in err()
    assert lib.cid_kv_pack_long_f16(64, 64, 64, 64, 2, 320, 8, cap + 1, 4, None) == -22 and f"1 to {cap} text rows".encode() in err()


@pytest.mark.parametrize("C,heads", HEAD_CONFIGS)
def test_pack_elems_match_the_model(lib, C, heads):
    for n_txt, n_ip in ((93, 4), (97, 0), (128, 4), (129, 3), (154, 4), (231, 4), (231, 32), (235, 0), (1, 0), (77, 4),
                        (32, 0), (33, 1), (1024, 32), (1024, 0)):
        want = lr.long_elems(C, heads, n_txt, n_ip)
        got = tuple(lib.cid_kv_pack_long_elems(C, heads, n_txt, n_ip, w) for w in (0, 1))
        assert got == want, (C, heads, n_txt, n_ip, got, want)


def test_pack_model_places_every_row_once():
    """the model itself: every real (row, head dim) value appears exactly once in either image, everything else is zero
    (values are distinct and non-zero by construction)"""
    R, C, heads, n_txt, n_ip = 2, 80, 2, 37, 3
    L = n_txt + n_ip
    base = (torch.arange(R * L * 2 * C, dtype=torch.float32).view(R * L, 2 * C) % 2000 + 1)
    kv_txt, kv_ip = base.half(), (-base).half()
    kp, vp = lr.kv_pack_long_ref(kv_txt, kv_ip, R, C, heads, n_txt, n_ip)
    assert (kp.shape[1], vp.shape[1]) == lr.long_elems(C, heads, n_txt, n_ip)
    t, i = kv_txt.view(R, L, 2 * C), kv_ip.view(R, L, 2 * C)
    for r in range(R):
        for img, col0 in ((kp, 0), (vp, C)):
            want = torch.cat([t[r, :n_txt, col0:col0 + C].reshape(-1), i[r, n_txt:, col0:col0 + C].reshape(-1)])
            got = img[r][img[r] != 0]
            assert torch.equal(got.float().sort().values, want.float().sort().values)
    # the ID keys start on the tile behind the last text tile: slot 64 of K, lane 0, head 0, k-step 0
    d, qks = C // heads, 3
    k0 = kp[0].view(heads, 3, qks, 64, 8)
    assert torch.equal(k0[0, 2, 0, 0], i[0, n_txt, :8]) and torch.equal(k0[0, 1, 0, 4], t[0, 36, :8])
    assert not k0[0, 1, 0, 5].any() and not k0[0, 2, 0, 3].any()            # text slot 37, ID slot 3: absent


class _Stub:
    """enough of HipUNet for cross_attention_path: the predicates it reads, none of the device state"""

    def __init__(self, v2, n_txt, n_ip, heads=8):
        from consistentid_amd import unet
        self._ctx = SimpleNamespace(v2=v2, n_txt=n_txt, n_ip=n_ip)
        self._xattn_fused_max_c, self._qattn, self._heads = 320, True, heads
        self._fused_gen1 = lambda c, tokens: unet.fused_gen1(c, tokens, 320)
        self._heads_of = lambda b: self._heads
        self.path = lambda *a: unet.HipUNet.cross_attention_path(self, *a)


def test_cross_attention_path_strings(lib):
    """contexts up to 96 rows keep their strings; a long context names its own sequence whatever the width"""
    from consistentid_amd import ops, unet
    b = "down_blocks.0.attentions.0.transformer_blocks.0"
    assert _Stub({b: 3}, 77, 4).path(b, 320, 4, 4096) == "id_xattn3_kernel<77,4> (one launch)"
    assert _Stub({b: 0}, 81, 0).path(b, 320, 4, 4096) == "id_xattn_kernel (one launch, first generation)"
    wide = _Stub({b: 0}, 77, 4).path(b, 1280, 8, 256)
    assert wide in ("q GEMM with attention epilogue + out GEMM (two launches)",
                    "layernorm + q GEMM with attention epilogue + out GEMM (three launches)")
    assert _Stub({b: 0}, 81, 0).path(b, 1280, 8, 256) == "layernorm + q GEMM + id_xattn core + out GEMM (four launches)"
    for c, B, N in ((320, 4, 4096), (640, 8, 1024), (1280, 8, 256)):
        got = _Stub({b: unet.LONG_CONTEXT}, 154, 4).path(b, c, B, N)
        want = ("q GEMM + id_xattn_long core<154,4> + out GEMM (three launches)" if ops.ln_fold(B * N) else
                "layernorm + q GEMM + id_xattn_long core<154,4> + out GEMM (four launches)")
        assert got == want, got
