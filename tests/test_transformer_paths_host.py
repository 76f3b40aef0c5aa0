"""The table of transformer-block launch paths (tests/golden/transformer_paths.json) against the host predicates of ops.py /
unet.py, at the default context and at contexts past 96 rows -- no GPU.  tests/test_gpu_transformer_paths.py runs one parity case per row; what is checked here is that the rows are
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


# ----------------------------------------------------------------------------- contexts past 96 rows
def _long_rows(table, f):
    """(the rows at LONG_CONTEXT, the one row at CAP_CONTEXT) of a family"""
    rows = table["long"][f]
    return [r for r in rows if r[0][3:5] == tp.LONG_CONTEXT[f]], [r for r in rows if r[0][3:5] == tp.CAP_CONTEXT[f]]


def test_the_short_rows_are_the_ones_from_before_the_long_contexts(table):
    """the 102 rows at 77 + 4 / 81 + 0 context rows, counted per family and spot-checked at both ends: teaching ``predict`` the
    long rule moved none of them (test_regenerating_the_grid_reproduces_the_table holds every one to the predicates)"""
    assert {f: len(rows) for f, rows in table["cases"].items()} == {"sd15": 35, "sdxl": 40, "controlnet": 27}
    assert table["cases"]["sd15"][0] == ((320, 8, 1, 77, 4, 1, 1, 24, 40), (False, False, "fold", "gen3", "folded", "fold", True))
    assert table["cases"]["controlnet"][-1] == ((1280, 8, 1, 81, 0, 6, 6, 24, 24),
                                                (False, False, "ln+gemm", "core", "folded", "fold", True))
    assert not any(comb[3].startswith("long") for rows in table["cases"].values() for _, comb in rows)
    assert all(tp.case_id(f, shp).count("ctx") == 0 for f, rows in table["cases"].items() for shp, _ in rows)


def test_every_long_row_is_filed_under_what_the_predicates_say(table):
    from consistentid_amd import ops
    for f in tp.FAMILIES:
        rows, cap = _long_rows(table, f)
        assert len(rows) + len(cap) == len(table["long"][f]) and len(cap) == 1, f
        for shp, comb in rows + cap:
            c, heads, n_layers, nt, ni, B, Bp, H, W = shp
            assert nt + ni > ops.XATTN_SHORT_MAX and tp.long_context(nt, ni) and B * H * W <= tp.MAX_TOKENS, (f, shp)
            assert tp.predict(*shp) == comb, f"{f} {shp}: filed under {comb}, the predicates say {tp.predict(*shp)}"
            Np = tp.padded_tokens(c, heads, nt, ni, H, W)
            assert Np == -(-H * W // 64) * 64 and comb[0] == (Np != H * W), "a long context pads to the self-attention's 64 tokens"
            assert comb[3] == ("long+fold" if ops.ln_fold(B * Np) else "long")
            assert (comb[4] == "folded") == ops.ff2_fold(B * Np, c, 0 if comb[0] else Np), "LONG_CONTEXT folds wherever ff2_fold holds"
            assert comb[1] == (Bp != B) and (not comb[1] or (f, c) == ("sd15", 320))
        # the padding rule differs from the short one exactly where a short context would run a 128-token kernel
        assert f == "sdxl" or any(c == 320 and (H * W) % 128 and not comb[0] for (c, _, _, _, _, _, _, H, W), comb in rows), f


def test_long_rows_cover_every_reduced_key_once(table):
    """SD1.5 and SDXL: one row per (c, heads, pad, dedup, xattn, tail) the family reaches on GRID under its long context, the
    smallest shape of each; no key is missing and none is listed that the grid does not reach.  The ControlNet: one row per
    width, the smallest of a key the grid reaches."""
    for f in tp.FAMILIES:
        rows, _ = _long_rows(table, f)
        reach = {}
        for s in tp.GRID:
            for shp in tp.levels(f, *s, tp.LONG_CONTEXT[f]):
                if shp[5] * shp[7] * shp[8] <= tp.MAX_TOKENS:
                    reach.setdefault(tp.long_key(shp), []).append(shp)
        filed = [tp.long_key(shp) for shp, _ in rows]
        assert len(set(filed)) == len(filed), f"{f}: a key has two rows"
        assert set(filed) <= set(reach), f"{f}: listed but not reachable on the grid: {set(filed) - set(reach)}"
        if f == "controlnet":
            assert sorted(k[0] for k in filed) == [320, 640, 1280], f"{f}: one row per width"
        else:
            assert set(filed) == set(reach), f"{f}: reachable without a row: {set(reach) - set(filed)}: {tp.REGENERATE}"
            assert {"long+fold", "long"} == {k[4] for k in filed} and {"folded", "ff2+proj_out"} == {k[5] for k in filed}
        assert sorted(shp for shp, _ in rows) == sorted(tp.enumerate_long(f).values()), f"{f}: {tp.REGENERATE}"
    assert any(k[3] for k in (tp.long_key(shp) for shp, _ in table["long"]["sd15"])), "no CFG-deduplicated long row"


def test_one_row_per_family_at_the_most_rows_a_pipeline_takes(table):
    from consistentid_amd import ops
    cap = ops.xattn_long_max_txt()
    assert tp.CAP_CONTEXT == {"sd15": (cap, 4), "sdxl": (cap, 4), "controlnet": (cap + 4, 0)}
    for f in tp.FAMILIES:
        (shp, comb), = _long_rows(table, f)[1]
        assert shp == tp.cap_shape(f) and shp[0] == tp.CAP_CHANNELS == 1280 and table["long"][f][-1] == (shp, comb)
        sizes = [s[5] * tp.padded_tokens(s[0], s[1], s[3], s[4], s[7], s[8]) for g in tp.GRID
                 for s in tp.levels(f, *g, tp.CAP_CONTEXT[f]) if s[0] == 1280]
        assert shp[5] * tp.padded_tokens(shp[0], shp[1], shp[3], shp[4], shp[7], shp[8]) == min(sizes)
        # the K/V pack of this row's B + 1 context rows walks its grid-stride loop (more than 2048 blocks of 256 chunks)
        ke, ve = ops.kv_pack_long_elems(shp[0], shp[1], shp[3], shp[4])
        assert (shp[5] + 1) * (ke + ve) // 8 > 2048 * 256, (f, ke, ve)


def test_long_rows_follow_the_short_rows_of_their_width(table):
    cases = tp.ordered_cases(table)
    assert len(cases) == sum(len(table[k][f]) for k in ("cases", "long") for f in tp.FAMILIES)
    assert len({tp.case_id(f, shp) for f, shp, _ in cases}) == len(cases), "two cases share an id"
    engines = [(f, shp[0]) for f, shp, _ in cases]
    assert [e for i, e in enumerate(engines) if i == 0 or engines[i - 1] != e] == sorted(set(engines), key=engines.index), \
        "an engine would be built twice"
    for i, (f, shp, _) in enumerate(cases[1:], 1):
        pf, pshp, _ = cases[i - 1]
        if (pf, pshp[0]) == (f, shp[0]):
            assert tp.long_context(*pshp[3:5]) <= tp.long_context(*shp[3:5]) and pshp[3] + pshp[4] <= shp[3] + shp[4], (f, shp)
    # one engine crosses 81, 158 and 1028 rows
    assert [s[3] + s[4] for f, s, _ in cases if (f, s[0]) == ("controlnet", 1280)][-3:] == [81, 158, 1028]


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
    assert tp.levels("controlnet", 3, 3, 24, 40, (158, 0))[-1] == (1280, 8, 1, 158, 0, 3, 3, 3, 5)
    assert [s[3:5] for s in tp.levels("sdxl", 2, 1, 128, 128, (231, 4))] == [(231, 4)] * 11


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
               "core": [ln, g(), dict(op="id_xattn_core"), g(res=True)],
               "long+fold": [g(ln=True), dict(op="id_xattn_long"), g(res=True)],
               "long": [ln, g(), dict(op="id_xattn_long"), g(res=True)]}[xattn]
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
    tr.records = [r for r in _records(False, "long", False, "ln+gemm") if r["op"] != "layernorm"]
    assert tp.observed(tr)[3] == "long without norm2"
    rs = _records(True, "long+fold", True, "fold")
    tr.records = [dict(r, mode=1) if rs[i + 1:i + 2] and rs[i + 1]["op"] == "id_xattn_long" else r for i, r in enumerate(rs)]
    # (the launch before the core is no plain projection)
    assert tp.observed(tr)[3] == "long without q"
    tr.records = _records(True, "gen3", True, "fold", n_keys=256)            # padded projections, unmasked keys
    assert isinstance(tp.observed(tr)[0], str)
