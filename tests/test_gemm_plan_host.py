"""Host checks of the GEMM dispatcher (no GPU): cid_gemm_plan / ops.gemm_plan report what cid_gemm_f16 would launch -- the
launch reads the same decision (csrc/gemm_plan.hip cidg::plan) -- so the planner can be held to the census of the launches the
models make (tests/golden/gemm_calls.json, tests/gemm_census.py) anywhere, and to the characterisation grid around it
(tests/golden/gemm_plan_grid.json, tests/gemm_plan_grid.py) under every planner switch."""
import ctypes as C
import json

import pytest

import gemm_census
import gemm_plan_grid

FIXTURE = gemm_census.load()
RECORDS = gemm_census.all_records(FIXTURE)
KEYS = gemm_census.keys_of(RECORDS)


def test_fixture_plans_match_planner(lib):
    """Planner drift: every recorded descriptor must still plan to the recorded launch (family, tile, split-K, N-loop, ring
    depth, instance flags, statistics).  A rule change that moves a model's shape shows here, with the shape."""
    moved = []
    for wl, rows in FIXTURE.items():
        for rec, plan in rows:
            now = dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(rec)))
            if now != plan:
                diff = {k: (plan[k], now[k]) for k in plan if plan[k] != now[k]}
                moved.append(f"{wl}: {gemm_census.variant_key(rec, plan)} M={rec['M']} N={rec['N']} K={rec['taps'] * (rec['c1'] + rec['c2'])}"
                             f" (recorded, now): {diff}")
    assert not moved, f"{len(moved)} of {len(RECORDS)} recorded launches plan differently now:\n  " + "\n  ".join(moved[:40]) + \
                      f"\nif the change is meant, regenerate the fixture: {gemm_census.REGENERATE}"


def test_fixture_is_the_census_it_claims_to_be(lib):
    """integers only, every workload present, and the launches the census was built to pin are in it by name"""
    assert set(FIXTURE) == {"sd15_512x512_cfg8", "sd15_512x512_cfg2", "sd15_512x768_cfg2", "sd15_controlnet_inpaint_cfg16",
                            "sdxl_1024x1024_cfg4", "sdxl_864x1152_cfg2", "vae_decode_512x512", "vae_encode_512x512", "clip_text_l",
                            "clip_text_bigg", "clip_vision_vit_h", "id_stack", "bisenet_512x512"}
    assert all(rows for rows in FIXTURE.values())
    assert all(type(v) is int for rec, plan in RECORDS for v in list(rec.values()) + list(plan.values()))
    families = {gemm_census.families()[p["family"]] for _, p in RECORDS}
    assert families == set(gemm_census.families()), f"families no workload reaches: {set(gemm_census.families()) - families}"
    # the UNets' Downsample2D convolutions (stride 2, pad 1, 320 / 640 / 1280 channels) at the benchmark's CFG batch:
    # 256x160 gather tiles, nine taps, split-K with its epilogue kernel, three-stage ring
    down = [(r, p) for r, p in FIXTURE["sd15_512x512_cfg8"] if r["taps"] == 9 and r["stride"] == 2]
    assert sorted(r["N"] for r, _ in down) == [320, 640, 1280]
    for r, p in down:
        assert (gemm_census.families()[p["family"]], p["bm"], p["bn"], p["nbuf"], p["splitk_epilogue"]) == ("igemm", 256, 160, 3, 1) \
            and p["splitk"] > 1, (r, p)
        assert gemm_census.variant_key(r, p) == "igemm-256x160-nb3-m0-t9-s2-u0-p0-sk-bias"


def test_every_reached_variant_has_a_parity_case(lib):
    """Every variant key of the census is either a case of test_gpu_gemm_census.test_variant_parity or, for mode 3 (the
    attention epilogue, which a descriptor alone cannot drive), the key of a launch test_id_cross_attention makes."""
    import test_gpu_gemm_census as table
    from test_gpu_kernels import XATTN_CASES, xattn_mode3_launches
    mode3 = set()
    for case in XATTN_CASES:
        for kw in xattn_mode3_launches(*case):
            rec = gemm_census.record_of(**dict(kw, att=True, ln=True if kw["ln"] else None))
            plan = dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(rec)))
            mode3.add(gemm_census.variant_key(rec, plan))
    assert mode3, "test_id_cross_attention makes no mode-3 launch"
    covered = set(table.TABLE) | mode3
    assert all(KEYS[k][0]["mode"] != 3 for k in table.TABLE) and all(k.startswith("igemm_att-") for k in mode3)
    uncovered = sorted(set(KEYS) - covered)
    print(f"[census] {len(KEYS)} variant keys: {len(table.TABLE)} table cases, {len(set(KEYS) & mode3)} matched by test_id_cross_attention")
    assert not uncovered, "launch variants the models reach without a parity case (add a test_id_cross_attention " \
                          f"parametrization for a mode-3 key):\n  " + "\n  ".join(uncovered)
    assert "igemm-256x160-nb3-m0-t9-s2-u0-p0-sk-bias" in table.TABLE


def test_gemm_plan_argument_validation(lib):
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError, GemmDesc, GemmPlanInfo
    info = GemmPlanInfo()
    d = GemmDesc()
    assert lib.cid_gemm_plan(C.byref(d), None) == -22 and b"null output" in lib.cid_last_error()
    assert lib.cid_gemm_plan(None, C.byref(info)) == -22 and b"null pointer" in lib.cid_last_error()
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == -22 and b"null pointer" in lib.cid_last_error()
    d.x1, d.w, d.out = 64, 64, 64
    d.c1, d.ld1, d.ldo, d.M, d.N, d.taps = 320, 320, 320, 256, 320, 1
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == 0
    assert (info.family, info.bm, info.bn, info.splitk, info.nloop, info.nbuf) == (0, 64, 160, 1, 1, 2)
    assert info.stats_rows == lib.cid_gemm_stats_rows(C.byref(d)) == 64
    # the query refuses what the launch refuses, with the launch's message
    d.taps = 3
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == -22 and b"taps must be 1 or 9" in lib.cid_last_error()
    d.taps, d.out = 1, 72
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == -22 and b"16-byte aligned" in lib.cid_last_error()
    d.out, d.pad_mode = 64, 1
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == -22 and b"pad_mode 1 needs" in lib.cid_last_error()
    d.pad_mode, d.act, d.ws, d.ws_bytes = 0, 1, 64, 1 << 20
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == -22 and b"act 1 needs" in lib.cid_last_error()
    d.act, d.gn_stats, d.N, d.ldo = 0, 64, 96, 96          # statistics from a launch off the 160-channel grid
    assert lib.cid_gemm_plan(C.byref(d), C.byref(info)) == -22 and b"cannot emit" in lib.cid_last_error()
    # the wrapper: dummy operands, the launch's errors as CidError, statistics only for a consumer that takes them
    p = ops.gemm_plan(M=8 * 4096, N=320, c1=320, taps=9, Hi=64, Wi=64, Ho=64, Wo=64, bias=True, gn_hw=4096)
    assert (p["family"], p["bm"], p["bn"], p["stats_rows"], p["stats"]) == ("conv_h32", 256, 160, 256, 1)
    assert ops.gemm_plan(M=8 * 4096, N=320, c1=320, taps=9, Hi=64, Wi=64, Ho=64, Wo=64, bias=True, gn_hw=0)["stats"] == 0
    with pytest.raises(CidError, match="c2 > 0 needs x2"):
        ops.gemm_plan(M=256, N=320, c1=320, c2=320)
    with pytest.raises(CidError, match="mode 3 needs att_kp"):
        ops.gemm_plan(M=1024, N=640, c1=640, mode=3, heads=8, dhead=80, ntok=1024)
    with pytest.raises(CidError, match="a tensor is required"):
        ops.gemm(True, True, True, M=256, N=320, c1=320)


def test_plan_grid_replays_under_every_switch(lib):
    """The characterisation grid: every case (census descriptors, their neighbours, the refusals) must plan to the recorded
    return code, plan fields and refusal text under the default switches and under each non-default value of each planner
    switch -- one child process per setting (the switches are read once per process), one after another."""
    z = gemm_plan_grid.load()
    cases = gemm_plan_grid.expand(z["descs"], z["neighbours"])
    assert len(z["default"]) == len(cases) and set(z["settings"]) == set(gemm_plan_grid.SETTINGS)
    moved = []
    for setting in ("",) + gemm_plan_grid.SETTINGS:
        got, want = gemm_plan_grid.run_child("plan", gemm_plan_grid.GOLDEN, setting), gemm_plan_grid.expected(z, setting)
        assert len(got) == len(want)
        moved += [f"{setting or 'defaults'}: case {i} {cases[i]}\n      recorded {w}\n      now      {g}"
                  for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not moved, f"{len(moved)} grid answers changed:\n  " + "\n  ".join(moved[:20]) + \
                      f"\nif the change is meant, regenerate the fixture: {gemm_plan_grid.REGENERATE}"


def _ln_fold_geglu_spec(M: int, C_: int, geglu_h32: bool) -> bool:
    """ops.ln_fold_geglu as it stood while it restated the planner's linear_h32 rule in Python (CID_LN_FOLD and
    CID_GEGLU_FOLD_MAX at their defaults; ``geglu_h32``: CID_GEGLU_H32 != 0): the specification of what it answers now"""
    h32 = geglu_h32 and C_ >= 1024 and M % 256 == 0 and (M // 256) * (8 * C_ // 160) >= 256 and (8 * C_) % 160 == 0
    return M <= 8192 and not h32


def test_ln_fold_geglu_matches_its_old_predicate(lib, tmp_path):
    """ops.ln_fold_geglu asks the planner whether the unfolded projection runs on linear_h32.hip; over every GEGLU shape of
    the census and of the grid it must answer what its own copy of the rule answered, with CID_GEGLU_H32 unset and = 0"""
    z = gemm_plan_grid.load()
    shapes = {(r["M"], r["c1"]) for r, _ in RECORDS if r["mode"] == 1}
    reached = len(shapes)
    shapes |= {(c["M"], c["c1"]) for c in gemm_plan_grid.expand(z["descs"], z["neighbours"])
               if c["mode"] == 1 and c["taps"] == 1 and c["c2"] == 0 and c["N"] == 8 * c["c1"] and c["c1"] % 64 == 0 and c["M"] > 0}
    shapes = sorted(shapes)
    assert reached >= 10 and len(shapes) > reached and any(_ln_fold_geglu_spec(M, c, False) != _ln_fold_geglu_spec(M, c, True) for M, c in shapes)
    (tmp_path / "shapes.json").write_text(json.dumps(shapes))
    for setting, on in (("", True), ("CID_GEGLU_H32=0", False)):
        got = gemm_plan_grid.run_child("fold", tmp_path / "shapes.json", setting)
        wrong = [(M, c, bool(g)) for (M, c), g in zip(shapes, got) if bool(g) != _ln_fold_geglu_spec(M, c, on)]
        assert not wrong, f"ops.ln_fold_geglu under {setting or 'the defaults'} differs from its old predicate at (M, C_, now): {wrong}"


# ----------------------------------------------------------------------------- the fast 3x3 convolutions on non-square images
FAST_CONV = ("igemm_halo", "conv_h32", "conv_h32_phase")


def test_rect_table_covers_every_fast_conv_key(lib):
    """tests/test_gpu_conv_rect.py: every 3x3 variant key of the census outside the gather kernel has at least one tall and one
    wide case, and every case still plans to its key.  A fast key added later fails here until it gets rectangular cases."""
    import test_gpu_conv_rect as rect
    fast = {k for k, (r, p) in KEYS.items() if r["taps"] == 9 and gemm_census.families()[p["family"]] != "igemm"}
    assert fast and {gemm_census.families()[KEYS[k][1]["family"]] for k in fast} == set(FAST_CONV)
    assert set(rect.RECT) == fast, f"without rectangular cases: {sorted(fast - set(rect.RECT))}; not in the census: {sorted(set(rect.RECT) - fast)}"
    moved = []
    for key, (tall, wide) in rect.RECT.items():
        assert tall and all(h > w for _, h, w in tall), f"{key}: no tall case / a tall case that is not tall: {tall}"
        assert wide and all(w > h for _, h, w in wide), f"{key}: no wide case / a wide case that is not wide: {wide}"
        base = KEYS[key][0]
        for shape in tall + wide:
            rec, plan, now = rect.rect_plan(key, shape)
            if now != key:
                moved.append(f"{key} {shape}: {now}")
            # only the geometry differs from the census record
            same = set(rec) - {"Hi", "Wi", "Ho", "Wo", "M", "gn_hw", "rows_per_sample"}
            assert all(rec[f] == base[f] for f in same) and rec["M"] == shape[0] * rec["Ho"] * rec["Wo"]
            assert max(shape[1], shape[2]) <= 4 * min(shape[1], shape[2])
    assert not moved, "rectangular cases that left their variant:\n  " + "\n  ".join(moved)
    assert len(rect.CASES) == sum(len(t) + len(w) for t, w in rect.RECT.values())


def _tile_geometry_faults(fam, bm, B, Hi, Wi, up):
    """What the kernels need of a planned tile, restated from their index arithmetic (csrc/gemm.hip igemm_halo_kernel,
    csrc/conv3x3.hip conv_h32_kernel): a list of violated conditions.  A tile is ``bm`` consecutive pixels of the tile image:
    the output image for the halo kernel and conv_h32, the input image (one output parity) for the phase mode."""
    Ho, Wo = Hi << up, Wi << up
    H, W = (Hi, Wi) if fam == "conv_h32_phase" else (Ho, Wo)
    P, M = H * W, B * Ho * Wo
    bad = []
    if M % bm:
        bad.append("M % bm != 0")
    if fam == "igemm_halo" and (bm != 256 or up):
        bad.append("the halo kernel has 256-token tiles and no upsampling")
    if P % bm and bm % P:
        bad.append("a tile is neither inside one image nor a whole number of whole images")
    if fam == "conv_h32_phase" and P % bm:
        bad.append("a phase tile is not inside one image (tiles per image and parity = P / bm)")
    seg = min(bm, P)                                  # pixels a tile takes from one image
    if seg % W:
        bad.append("a tile is not made of whole rows")
    rows = seg // W
    if up and fam == "conv_h32":
        if bm > P or rows % 2:
            bad.append("up = 1 on nine taps: a tile is not an even number of output rows of one image")
    # halo rows as the kernels count them: per image of the tile, its rows (input rows under up = 1) and columns plus a frame
    ups = up if fam == "conv_h32" else 0
    nh = (bm // seg) * ((rows >> ups) + 2) * ((W >> ups) + 2)
    cap = 448 if fam == "igemm_halo" else 400         # HPW * NW * 8 halo rows (gemm.hip); three weight stages next to two halo
    if nh > cap:                                      # buffers in 160 KB (conv3x3.hip)
        bad.append(f"{nh} halo rows exceed the buffer's {cap}")
    return bad


def test_fast_conv_tiles_on_a_rectangle_grid(lib):
    """Whatever route_halo / route_conv3x3 send to a fast kernel on a non-square image is a tiling that kernel can index."""
    from consistentid_amd import ops
    sides = (4, 8, 12, 16, 24, 32, 48, 64, 96, 128)
    seen, faults = {}, []
    for Hi in sides:
        for Wi in sides:
            if Hi == Wi:
                continue
            for B in (1, 2, 4, 8):
                for C_ in (320, 640, 1280):
                    for up, w4 in ((0, None), (1, True), (1, None)):
                        Ho, Wo = Hi << up, Wi << up
                        p = ops.gemm_plan(M=B * Ho * Wo, N=C_, c1=C_, taps=9, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, stride=1, up=up, bias=True,
                                          ws=True, ws_bytes=64 << 20, gn_hw=Ho * Wo, w_up4=w4)
                        fam = p["family"]
                        if fam not in FAST_CONV:
                            continue
                        assert fam != "conv_h32_phase" or w4, "the phase mode without folded weights"
                        orient = "tall" if Hi > Wi else "wide"
                        seen[fam, up, orient] = seen.get((fam, up, orient), 0) + 1
                        faults += [f"B={B} {Hi}x{Wi} C={C_} up={up} w_up4={bool(w4)} -> {fam} bm={p['bm']}: {why}"
                                   for why in _tile_geometry_faults(fam, p["bm"], B, Hi, Wi, up)]
    print(f"[rect grid] fast plans: {seen}")
    # the grid reaches every family in both orientations (and conv_h32's nine-tap up = 1 path), or it checks nothing
    for want in [(f, u, o) for o in ("tall", "wide") for f, u in (("igemm_halo", 0), ("conv_h32", 0), ("conv_h32", 1), ("conv_h32_phase", 1))]:
        assert seen.get(want, 0) >= 4, f"the grid hardly reaches {want}: {seen}"
    assert not faults, f"{len(faults)} planned tilings a kernel cannot index:\n  " + "\n  ".join(faults[:30])
