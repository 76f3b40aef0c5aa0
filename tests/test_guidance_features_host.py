"""Host-side checks of tests/test_gpu_guidance_features.py's lists, which are plain data, and of the PAG / SAG branch of
tests/engine_cases.py: the pairwise list covers every pair of factor values, every generation runs enough steps to warm up,
capture and replay, every step launch a spec names is one the engine can report, what the lists leave out is refused by
``refuse_sag_with`` or the PAG checks, and every generation that the GPU file compares with the oracle can fail -- for SAG,
conditions (a) and (b) of tests/test_gpu_sag.py's docstring and the margin (c) at the seed search's factor, on the fp32 oracle
with a CPU fp16 copy as the arm; for PAG, the guidance moves the fp32 oracle by ten times the largest tolerance the
comparison can come to.  No GPU."""
import dataclasses
import itertools

import pytest
import torch

import engine_cases as E
import test_gpu_guidance_features as G
from conftest import TOL_L2, rel_l2
from engine_cases import Spec, active_sets, executed_steps, expected_step_path, features_on, pag_on, single_pass

# the stock fp16 arm's rel_l2 on the MI355X over tests/test_gpu_pag.py's nine trajectories is 3.2e-3 - 5.7e-3 (its docstring):
# ten times max(TOL_L2, 1.5 x 6e-3) is the most ``assert_features_matter`` can ask of a PAG generation there
PAG_NEEDS = 10 * max(TOL_L2, 1.5 * 6e-3)


def _compared():
    """{label: spec} of the generations the GPU file holds to the oracle"""
    return {what: s.but(callback=False) for what, (s, bits) in G.all_specs().items() if not bits}


def _values(row):
    return dict(zip(G.FACTORS, row))


def test_pairwise_list_covers_every_pair_of_factor_values():
    rows = [_values(r) for r in G.PAIRWISE_ROWS]
    assert len(rows) <= 24 and len(G.PAIRWISE) == len(rows) == len(set(G.PAIRWISE_ROWS))
    for r in rows:
        assert all(r[k] in G.FACTORS[k] for k in G.FACTORS), r
    missing = []
    for a, b in itertools.combinations(G.FACTORS, 2):
        have = {(r[a], r[b]) for r in rows}
        missing += [((a, va), (b, vb)) for va, vb in itertools.product(G.FACTORS[a], G.FACTORS[b]) if (va, vb) not in have]
    assert not missing, f"pairs of factor values that no spec of the list has: {missing}"
    for row, spec in zip(G.PAIRWISE_ROWS, G.PAIRWISE.values()):
        r = _values(row)
        assert spec.pipe == r["pipe"] and spec.prediction == r["prediction"] and (spec.freeu is not None) == r["freeu"]
        assert bool(spec.loras) == r["loras"] and spec.scheduler == G.SAMPLERS[r["sampler"]]["scheduler"]
        assert single_pass(spec) == (r["sampler"] == "lcm single")
        mid = G.PAG_MID_V if r["prediction"] == "v_prediction" else G.PAG_MID
        assert (spec.pag, spec.sag) == {"none": (None, 0.0), "pag mid": (mid, 0.0), "pag all": (G.PAG_ALL, 0.0), "sag": (None, G.SAG)}[r["guidance"]]
        assert features_on(spec) == [k for k in ("freeu", "loras") if r[k]] + {"none": [], "sag": ["sag"]}.get(r["guidance"], ["pag"])


def test_every_generation_warms_up_captures_and_replays():
    """at least 3 executed steps on one set of active nets (eager, capture, replay), at most 11 generations a scenario, small
    latents; the only one-step spec is the masses-only one, which runs eagerly"""
    specs = G.all_specs()
    assert len(specs) == (len(G.ONE_ENGINE) + len(G.SIZES) + len(G.SAG_SCHEDULERS) + len(G.PAG_SCHEDULERS) + len(G.STRENGTH)
                          + len(G.PAG_SWITCHES) + len(G.SAG_SWITCHES) + len(G.SDXL_PAG) + len(G.SDXL_SAG) + len(G.TIME_COND)
                          + len(G.LN_FOLD) + len(G.SHARED) + len(G.PAIRWISE))
    for rows in (G.ONE_ENGINE, G.SIZES, G.SAG_SCHEDULERS, G.PAG_SCHEDULERS, G.STRENGTH, G.PAG_SWITCHES, G.SAG_SWITCHES, G.SDXL_PAG,
                 G.SDXL_SAG, G.TIME_COND, G.LN_FOLD, G.SHARED):
        assert len(rows) <= 11
    for what, (spec, bits) in specs.items():
        assert 3 <= executed_steps(spec) <= 5 and spec.steps <= 8 and spec.B in (1, 2, 3), what
        assert active_sets(spec) == {(): executed_steps(spec)} and not spec.nets and spec.rescale == 0.0, what
        assert spec.hw is None or spec.hw[0] * spec.hw[1] <= 16 * 16, what
        assert not bits or spec.sag > 0.0, f"{what}: only a SAG generation may go without the oracle"
        if spec.sag > 0.0 and not bits:     # the threshold trap: one sample, at most 16 mid-block tokens
            hm, wm = E.mid_size(spec)
            assert spec.B == 1 and hm * wm <= 16, what
    two = G.SDXL_TWO_SAMPLES
    assert two.B == 2 and executed_steps(two) == 1 and two.merge == -1 and two.null_post and E.mid_size(two) == (4, 4)


def test_step_paths_are_bound_entries():
    """every launch a spec names is "<kernel>[+pag | +sag]" of the three step kernels, follows its spec, and has its ops entry"""
    from consistentid_amd import ops
    entry = {"cfg_ddim": "cfg_{}ddim_step", "cfg_multistep": "cfg_{}multistep_step", "multistep": "{}multistep_step"}
    for what, (spec, _) in G.all_specs().items():
        path = expected_step_path(spec)
        base, _, guided = path.partition("+")
        assert base in entry and guided in ("", "pag", "sag"), (what, path)
        assert guided == ("pag" if pag_on(spec) else "sag" if spec.sag > 0.0 else ""), (what, path)
        assert (base == "multistep") == single_pass(spec), (what, path)
        assert callable(getattr(ops, entry[base].format(guided + "_" if guided else ""))), (what, path)
        assert E.unet_rows(spec) == ((1 if single_pass(spec) else 2) + (guided == "pag")) * spec.B
    assert expected_step_path(Spec(pag=("mid", 0.0, 0.0))) == "cfg_ddim" and E.unet_rows(Spec(pag=("mid", 0.0, 0.0))) == 4


class _Stop(Exception):
    pass


class _NoUNet:
    """stands where DenoiseEngine.run would first touch its UNet: the refusals come before"""

    def __getattr__(self, name):
        raise _Stop(name)


@pytest.mark.parametrize("case", [r[0] for r in G.REFUSED])
def test_refused_pairs_are_refused_by_the_engines_checks(case):
    """each pair the lists leave out: NotImplementedError from ``refuse_sag_with`` or the PAG checks of DenoiseEngine.run, which
    has touched neither its UNet nor a tensor by then; the same keywords without the second of the pair get past the checks.
    A ``Spec`` cannot say such a pair either."""
    from consistentid_amd import scheduler
    from consistentid_amd.denoise import DenoiseEngine, refuse_sag_with
    _, kind, extra = {r[0]: r for r in G.REFUSED}[case]
    kw = dict(extra, **({"controlnet": object()} if kind == "controlnet" else {}))
    run = lambda **k: DenoiseEngine(_NoUNet(), scheduler.DDIMScheduler(), use_graph=False).run(
        None, None, None, None, num_inference_steps=3, guidance_scale=5.0, start_merge_step=0, **k)
    with pytest.raises(NotImplementedError):
        run(**kw)
    if kw.get("sag_scale", 0.0) > 0.0:
        with pytest.raises(NotImplementedError):
            refuse_sag_with(kw["sag_scale"], kw.get("pag_scale", 0.0), kw.get("guidance_rescale", 0.0), "controlnet" in kw)
    first = next(k for k in ("pag_scale", "sag_scale") if k in kw)
    with pytest.raises(_Stop):
        run(**{first: kw[first]})
    fields = dict(pag=G.PAG_MID if "pag_scale" in kw else None, sag=kw.get("sag_scale", 0.0), rescale=kw.get("guidance_rescale", 0.0),
                  **(dict(pipe="controlnet", nets=("A",), scales=(0.5,), windows=((0.0, 1.0),)) if kind == "controlnet" else {}))
    with pytest.raises(ValueError, match="refused by the engine"):
        Spec(**fields)


def test_refused_list_is_what_the_engine_refuses():
    assert {r[0].replace(" on SDXL", "") for r in G.REFUSED} == {
        "PAG with SAG", "PAG with guidance_rescale", "SAG with guidance_rescale", "PAG with a ControlNet", "SAG with a ControlNet"}
    assert E.refused(Spec(pag=("mid", 0.0, 0.0), rescale=0.7)) is None, "a selection without a scale is a plain call"


def test_sag_references_can_tell():
    """every SAG generation that is compared with the oracle: (a) SAG moves the fp32 oracle by 20 x TOL_L2, (b) 1/8 - 7/8 of the
    mask cells are set at every evaluation, (c) min |mass - 1| is at least ten times the CPU stand-in's largest mass deviation,
    the seed search's target"""
    specs = {s: what for what, s in _compared().items() if s.sag > 0.0}
    assert len(specs) >= 22 and sum(what.startswith("10: ") for what in specs.values()) == 5
    for spec, what in specs.items():
        E.assert_sag_reference(spec, "cpu", E.SAG_SEARCH_FACTOR)
    assert not any(s.sag > 0.0 for s in _compared().values() if s.B != 1)


def test_only_what_no_seed_can_save_goes_without_a_trajectory_comparison():
    """``bits_only``: the 64-token latent size (192 cells a trajectory), LCM on the CFG path and DDIM with eta (the issue asks
    for the oracle "where (c) holds").  Their first-evaluation masses are still held to the reference: on the CPU at least half
    of those cells are further than 4 x the stand-in's deviation from the threshold, so the mask comparison is not empty"""
    import numpy as np
    bits = {what: s for what, (s, b) in G.all_specs().items() if b}
    assert sorted(bits) == ["2: 0 32 x 32: the mid block fills the token axis", "2: 2 32 x 32 again",
                            "3s: 4 LCM at guidance 5: the CFG path", "3s: 6 DDIM eta 1"]
    for what, spec in bits.items():
        ref, arm = E.guidance_trace(spec, "cpu")[0][0], E.guidance_trace(spec, "cpu", True)[0][0]
        clear = np.abs(ref - 1.0) > 4.0 * np.abs(arm - ref).max()
        assert clear.sum() >= ref.size // 2, what


def test_mass_cases_meet_their_reference_conditions():
    """test_gpu_sag.MASS_CASES on the reference alone (``mass_inputs``): the masses span 0.9 .. 1.1, the rows sum to n_keys, and
    the two samples of a split-buffer case are 10 x the fp32 arm's deviation apart; N = 4096 stays within a second"""
    import test_gpu_sag as T
    assert {"d32", "d40", "d80", "d40-partial-tile", "81-of-128", "33-of-64", "257-of-288-nine-tiles", "4096-top-of-lds",
            "split-buffers", "one-head", "three-heads"} <= set(T.MASS_CASES)
    for case, (B, heads, N, n_keys, d, sd, *layout) in T.MASS_CASES.items():
        qk, c, ref, arm = T.mass_inputs(case)
        real = ref[:, :n_keys]
        assert c == heads * d and tuple(qk.shape) == (B * N, 2 * c) and N % 32 == 0 and n_keys <= N <= 4096, case
        assert real.min() < 0.9 and real.max() > 1.1 and abs(float(real.sum(1).mean()) - n_keys) < 1e-6 * n_keys, case
        assert torch.equal(ref[:, n_keys:], torch.zeros(B, N - n_keys, dtype=ref.dtype)), case
        if layout:
            assert float((ref[0] - ref[1]).abs().max()) >= 10 * float((arm.double() - ref).abs().max()), case


def test_pag_references_can_tell():
    """every PAG generation that is compared with the oracle moves the fp32 oracle by ``PAG_NEEDS``, except the two at strength
    0.6, whose point is another one (below)"""
    strength = {s for _, s in G.STRENGTH}
    specs = {s: what for what, s in _compared().items() if pag_on(s) and s not in strength}
    assert len(specs) >= 30
    for spec, what in specs.items():
        moved = rel_l2(E.oracle_run(spec, "cpu"), E.oracle_run(spec.but(pag=None), "cpu"))
        assert moved >= PAG_NEEDS, f"{what}: PAG moves the fp32 oracle by {moved:.3e} < {PAG_NEEDS:.1e}"


def test_strength_specs_tell_the_schedule_entry_from_the_executed_step():
    from consistentid_amd.denoise import pag_scale_column
    from consistentid_amd import scheduler
    sch = scheduler.DDIMScheduler()
    for what, spec in G.STRENGTH:
        assert E.first_step(spec) == spec.steps - 3 > 0 and executed_steps(spec) == 3, what
        E.assert_misindexed_differs(spec, "cpu")
    sch.set_timesteps(G.STRENGTH[1][1].steps)
    skipped, into = (pag_scale_column(p[1], p[2], sch.timesteps) for p in (G.PAG_SKIPPED_ONLY, G.PAG_INTO_EXECUTED))
    first = E.first_step(G.STRENGTH[1][1])
    assert (skipped[:first] > 0).all() and (skipped[first:] == 0).all()
    assert (into[:first + 1] > 0).all() and (into[first + 1:] == 0).all()
    assert [s for s, _ in E.guidance_trace(G.STRENGTH[1][1], "cpu")[2]] == [0.0, 0.0, 0.0]
    assert [s > 0 for s, _ in E.guidance_trace(G.STRENGTH[1][1], "cpu", False, True)[2]] == [True, True, False]


def test_scenarios_are_the_sequences_they_claim():
    one = [s for _, s, _, _ in G.ONE_ENGINE]
    assert [expected_step_path(s) for s in one] == ["cfg_ddim", "cfg_ddim+sag", "cfg_ddim+sag", "cfg_ddim", "cfg_ddim+pag", "cfg_ddim+pag",
                                                    "cfg_ddim+pag", "cfg_ddim", "cfg_ddim+sag"]
    assert one[0] == one[3] == one[7] == G.ONE and one[8] == one[1] and G.ONE_ENGINE[3][2] == dict(sag_scale=0.0)
    assert one[5].pag[0] == one[6].pag[0] != one[4].pag[0] and one[6].pag[2] > 0.0, "the adaptive scale keeps the selection"
    assert [E.mid_size(s) for _, s, _ in G.SIZES] == [(8, 8), (4, 2), (8, 8), (4, 2)]
    for sag, pag in zip(G.SAG_SCHEDULERS, G.PAG_SCHEDULERS):
        assert (sag[1].scheduler, sag[1].eta, single_pass(sag[1])) == (pag[1].scheduler, pag[1].eta, single_pass(pag[1])), (sag[0], pag[0])
    assert [s.scheduler for _, s in G.PAG_SCHEDULERS] == ["ddim", "euler", "dpm", "pndm", "lcm", "lcm", "ddim"]
    assert G.SDXL_PAG[-1][1] == G.SDXL_PAG[0][1]
    for rows in (G.PAG_SWITCHES, G.SDXL_PAG[:-1]):      # one field at a time, except the steps back
        for (_, a), (what, b) in zip(rows, rows[1:]):
            diff = [f.name for f in dataclasses.fields(Spec) if getattr(a, f.name) != getattr(b, f.name)]
            assert 1 <= len(diff) <= 2, (what, diff)
    assert [features_on(s) for _, s in G.PAG_SWITCHES][:5] == [["pag"], ["freeu", "pag"], ["freeu", "loras", "pag"], ["loras", "pag"], ["pag"]]
    assert {w for w, _ in G.PAG_SWITCHES} == {w for w, _, _ in G.SAG_SWITCHES}, "the same switches under either guidance"
    assert G.PAG_SWITCHES[-1][1].adapter == G.SAG_SWITCHES[-1][1].adapter == 1 and not any(s.adapter for _, s in G.PAG_SWITCHES[:-1])
    assert [features_on(s) for _, s, _ in G.SAG_SWITCHES] == [["sag"], ["freeu", "sag"], ["sag"], ["loras", "sag"]] + [["sag"]] * 7
    assert E.inputs(G.PAG_SWITCHES[7][1], "cpu")["text"].shape[1] == 154 + 4
    assert all(s.null_post for _, s, _ in G.SDXL_SAG) and [s.time_ids for _, s, _ in G.SDXL_SAG] == [(0, 0), (8, 16), (8, 16), (0, 0)]
    assert all(single_pass(s) and s.time_cond for _, s in G.TIME_COND) and [E.unet_rows(s) for _, s in G.TIME_COND] == [2, 4, 1, 4, 2]
    assert [s.B for _, s in G.LN_FOLD] == [2, 3, 2] and all(s.pag == G.PAG_ALL for _, s in G.LN_FOLD)
    d = G.SHARED
    assert [p for _, p, _, _ in d] == ["P1", "P1", "P2", "P1", "P1"] and d[-1][2] == d[0][2]
    assert all(via is None or via != p for _, p, _, via in d), "every selection is made through the OTHER pipeline"
    assert [s.pag is not None for _, _, s, _ in d] == [False, True, True, True, False] and d[3][2].sag > 0.0 and not pag_on(d[3][2])
    from test_gpu_freeu import FREEU
    import test_gpu_pag as P
    assert G.FREEU == FREEU and P.SELECTIONS is E.PAG_SELECTIONS


def test_new_spec_fields_default_to_off_and_keep_the_memo_keys():
    s = Spec()
    assert (s.pag, s.sag) == (None, 0.0) and features_on(s) == [] and E.refused(s) is None
    assert Spec(pipe="inpaint", steps=5) == Spec(pipe="inpaint", steps=5, pag=None, sag=0.0)
    assert hash(Spec(pipe="inpaint", steps=5)) == hash(Spec(pipe="inpaint", steps=5, pag=None, sag=0.0))
    for base in (Spec(), Spec(pipe="sdxl", guidance=7.5)):
        assert E.inputs(base, "cpu") is E.inputs(base.but(pag=G.PAG_ALL), "cpu") is E.inputs(base.but(sag=1.0), "cpu")
    assert features_on(Spec(pag=("mid", 0.0, 0.0))) == [] and features_on(Spec(pag=G.PAG_MID, freeu=G.FREEU)) == ["freeu", "pag"]


def test_engine_cases_oracle_is_the_reference_of_the_two_test_files():
    """``oracle_run`` of a PAG / SAG spec is, bit for bit, what tests/test_gpu_pag.py and tests/test_gpu_sag.py compare with"""
    import test_gpu_pag as P
    import test_gpu_sag as T
    case = "dpm"
    assert torch.equal(E.oracle_run(T.CASES[case].but(sag=T.SAG), "cpu"), T.sag_oracle(case, "cpu", False, T.SAG)[0])
    spec = P._traj_spec("inpaint", "lcm")
    scale, adaptive = P.PAG["lcm"]
    assert torch.equal(E.oracle_run(spec.but(pag=("all", scale, adaptive)), "cpu"), P._pag_oracle(spec, "cpu", False, "all", scale, adaptive)[0])
