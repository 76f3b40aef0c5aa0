"""The table of transformer-block launch paths (tests/golden/transformer_paths.json) against the host predicates of ops.py /
unet.py -- no GPU.  tests/test_gpu_transformer_paths.py runs one parity case per row; what is checked here is that the rows are
the combinations the models reach on the grid of tests/transformer_paths.py, each filed under what the engine would do."""
import os

import pytest

import transformer_paths as tp


@pytest.fixture(scope="module")
def table(lib):
    changed = {k: os.environ[k] for k, v in tp.SWITCHES.items() if os.environ.get(k, v) != v}
    if changed:
        pytest.skip(f"the launch-path table is for the default switches, this environment sets {changed}")
    return tp.load()


@pytest.fixture(scope="module")
def grid(table):
    return {f: tp.enumerate_grid(f) for f in tp.FAMILIES}


def test_switches_are_the_ones_the_predicates_read():
    """every CID_* switch ops.py / unet.py read for a launch-path decision is in SWITCHES with its default"""
    import re
    from pathlib import Path
    root = Path(tp.__file__).resolve().parents[1] / "consistentid_amd"
    read = dict(re.findall(r'os\.environ\.get\("(CID_[A-Z0-9_]+)", *"([^"]*)"\)', (root / "ops.py").read_text()
                           + (root / "unet.py").read_text()))
    read["CID_XATTN_GEN"] = "3"                 # (ops.xattn_generation: str(XATTN_GEN_DEFAULT))
    read.pop("CID_GN_EPILOGUE_STATS")           # whether statistics are attached, not whether the consumer is announced
    assert read == tp.SWITCHES


def test_regenerating_the_grid_reproduces_the_table(table, grid):
    for f in tp.FAMILIES:
        want = sorted((shp, key[1:]) for key, shp in grid[f].items() if shp is not None)
        assert sorted(table["cases"][f]) == want, f"{f}: {tp.REGENERATE}"


def test_every_combination_has_a_case_or_a_named_omission(table, grid):
    for f in tp.FAMILIES:
        filed = {(shp[0],) + comb for shp, comb in table["cases"][f]}
        named = {(c,) + comb for c, comb, reason in table["omitted"][f]}
        assert all(reason.strip() for _, _, reason in table["omitted"][f]), f"{f}: an omission without a reason"
        assert not filed & named, f"{f}: {filed & named} has a case and is omitted"
        assert filed | named == set(grid[f]), f"{f}: on the grid without a case or a named omission: {set(grid[f]) - filed - named}"
        assert len(named) <= 0.05 * len(grid[f]), f"{f}: {len(named)} of {len(grid[f])} combinations omitted"


def test_every_case_is_filed_under_what_the_predicates_say(table):
    for f in tp.FAMILIES:
        cfg, n_txt, n_ip = tp.family_config(f)
        assert len({comb for _, comb in table["cases"][f]}) > 1
        for shp, comb in table["cases"][f]:
            c, heads, n_layers, nt, ni, B, Bp, H, W = shp
            assert (nt, ni) == (n_txt, n_ip) and B * H * W <= tp.MAX_TOKENS, (f, shp)
            assert tp.predict(*shp) == comb, f"{f} {shp}: filed under {comb}, the predicates say {tp.predict(*shp)}"
            assert comb[2] in tp.QKV and comb[3] in tp.XATTN and comb[4] in tp.TAIL and comb[5] in tp.GEGLU
            assert comb[1] == (Bp != B) and (not comb[1] or (f, c) == ("sd15", 320)), "only SD1.5's first transformer deduplicates"


def test_what_was_covered_before_is_a_strict_subset(table):
    """documents the gap: the real-width shapes that ran against the oracle before reach fewer combinations than the table"""
    for f in tp.FAMILIES:
        filed = {(shp[0],) + comb for shp, comb in table["cases"][f]}
        before = tp.combinations_of(f, tp.COVERED_BEFORE[f])
        assert before < filed, (f, before - filed)
        print(f"[paths] {f}: {len(filed)} combinations, {len(before)} reached before, {len(filed - before)} new")


def test_the_levels_of_a_model_are_the_engine_walk():
    """levels(): resolution halves per down block, SD1.5's first transformer alone sees the Bp distinct samples"""
    sd = tp.levels("sd15", 4, 2, 24, 40)
    assert [(s[0], s[5], s[6], s[7], s[8]) for s in sd[:3]] == [(320, 4, 2, 24, 40), (320, 4, 4, 24, 40), (640, 4, 4, 12, 20)]
    assert len(sd) == 16 and sd[6][:3] == (1280, 8, 1) and sd[6][7:] == (3, 5)          # the mid block
    xl = tp.levels("sdxl", 2, 1, 128, 128)
    assert len(xl) == 11 and xl[0] == (640, 10, 2, 77, 4, 2, 2, 64, 64) and xl[4] == (1280, 20, 2, 77, 4, 2, 2, 32, 32)
    cn = tp.levels("controlnet", 3, 3, 24, 40)
    assert len(cn) == 7 and cn[-1] == (1280, 8, 1, 81, 0, 3, 3, 3, 5)


def _records(qkv_ln, xattn, folded, geglu, *, B=2, Bp=2, ntok=256, n_keys=240, c=640, layers=1, gn_hw=0):
    """the launches of one block as Trace would record them (a hand-written sequence, not the engine's)"""
    g = lambda **kw: dict(dict(op="gemm", mode=0, M=B * ntok, N=c, c1=c, ntok=0, ln=False, att=False, out2=False, res=False,
                               family="linear"), **kw)
    ln = dict(op="layernorm")
    rs = [g()]                                                                          # proj_in
    for k in range(layers):
        rs += ([] if qkv_ln else [ln]) + [g(mode=2, M=Bp * ntok, N=3 * c, ntok=ntok, ln=qkv_ln),
                                          dict(op="self_attn", N=ntok, n_keys=n_keys, B=Bp), g(res=True, out2=Bp != B)]
        rs += {"gen3": [dict(op="id_xattn3")], "gen1": [dict(op="id_xattn")],
               "qattn+fold": [g(mode=3, ntok=ntok, ln=True, att=True), g(res=True)],
               "qattn": [ln, g(mode=3, ntok=ntok, att=True), g(res=True)],
               "core+fold": [g(ln=True), dict(op="id_xattn_core"), g(res=True)],
               "core": [ln, g(), dict(op="id_xattn_core"), g(res=True)]}[xattn]
        rs += {"fold": [g(mode=1, N=8 * c, ln=True)], "ln+h32": [ln, g(mode=1, N=8 * c, family="geglu_h32")],
               "ln+gemm": [ln, g(mode=1, N=8 * c, family="geglu")]}[geglu]
        if not (folded and k == layers - 1):
            rs.append(g(c1=4 * c, res=True))
    rs.append(g(c1=5 * c, res=True, gn_hw=gn_hw) if folded else g(res=True, gn_hw=gn_hw))
    return rs


@pytest.mark.parametrize("xattn", tp.XATTN)
@pytest.mark.parametrize("geglu", tp.GEGLU)
def test_observed_reads_the_fields_off_a_record(xattn, geglu):
    for qkv_ln, folded, layers in ((True, True, 1), (False, False, 2), (True, False, 1), (False, True, 2)):
        tr = tp.Trace(2, 2, 12, 20)
        tr.records = _records(qkv_ln, xattn, folded, geglu, layers=layers)
        assert tp.observed(tr) == (True, False, "fold" if qkv_ln else "ln+gemm", xattn, "folded" if folded else "ff2+proj_out",
                                   geglu, False)
    tr = tp.Trace(4, 2, 16, 16)
    tr.records = _records(True, xattn, True, geglu, B=4, Bp=2, n_keys=256, gn_hw=256)
    assert tp.observed(tr) == (False, True, "fold", xattn, "folded", geglu, True)


def test_observed_names_a_launch_without_its_norm():
    tr = tp.Trace(2, 2, 12, 20)
    tr.records = [r for r in _records(False, "core", False, "ln+gemm") if r["op"] != "layernorm"]
    got = tp.observed(tr)
    assert got[2] == "gemm without norm1" and got[3] == "core without norm2" and got[5] == "gemm without norm3"
    tr.records = _records(True, "gen3", True, "fold", n_keys=256)            # padded projections, unmasked keys
    assert isinstance(tp.observed(tr)[0], str)
