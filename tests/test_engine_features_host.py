"""Host-side checks of tests/test_gpu_engine_features.py's scenarios, which are plain data: the pairwise list covers every pair
of factor values the product accepts, every generation runs enough steps to warm up, capture and replay, the new ``Spec``
fields default to "off" and leave the memo keys of earlier specs alone, and the memoised fp32 oracle is what it was after a
FreeU spec went through it.  No GPU."""
import dataclasses
import itertools

import pytest
import torch

import test_gpu_engine_features as F
from engine_cases import (Spec, active_sets, executed_steps, features_on, hooked_modules, inputs, oracle_models, oracle_run,
                          product_scheduler, scheduler_kwargs)

# pairs of factor values the product refuses, and how: {((factor, value), (factor, value)): (exception type, message pattern,
# a callable that must raise it)}.  None today: all four samplers take either prediction type, guidance_rescale is a keyword
# of all five pipelines, FreeU and LoRAs are state of either UNet family.  (Zero-SNR is no factor of the list; its one
# restriction is asserted below.)
REFUSED = {}


def _values(row):
    return dict(zip(F.FACTORS, row))


def test_pairwise_list_covers_every_pair_of_factor_values():
    rows = [_values(r) for r in F.PAIRWISE_ROWS]
    assert len(rows) <= 30 and len(F.PAIRWISE) == len(rows) + 1 and len(set(F.PAIRWISE_ROWS)) == len(rows)
    for r in rows:
        assert all(r[k] in F.FACTORS[k] for k in F.FACTORS), r
    missing = []
    for a, b in itertools.combinations(F.FACTORS, 2):
        have = {(r[a], r[b]) for r in rows}
        for va, vb in itertools.product(F.FACTORS[a], F.FACTORS[b]):
            if (va, vb) not in have and ((a, va), (b, vb)) not in REFUSED:
                missing.append(((a, va), (b, vb)))
    assert not missing, f"pairs of factor values that no spec of the list has: {missing}"
    for pair, (exc, match, call) in REFUSED.items():
        with pytest.raises(exc, match=match):
            call()


def test_pairwise_specs_are_what_their_rows_say():
    for row, spec in zip(F.PAIRWISE_ROWS, F.PAIRWISE.values()):
        r = _values(row)
        assert spec.but(steps=4, windows=F.PIPES[r["pipe"]].windows) == F.PIPES[r["pipe"]].but(
            prediction=r["prediction"], freeu=F.FREEU if r["freeu"] else None, rescale=r["rescale"],
            loras=F.LORA_07 if r["loras"] else (), **F.SAMPLERS[r["sampler"]])
        assert features_on(spec) == [k for k in ("freeu", "rescale", "loras") if r[k]]
        assert F.step_path(spec) in ("cfg_ddim", "cfg_multistep", "cfg_ddim+rescale", "cfg_multistep+rescale")
        assert F.step_path(spec).startswith("cfg_ddim") == (r["sampler"] in ("ddim", "euler"))
        assert F.step_path(spec).endswith("+rescale") == (r["rescale"] > 0)
    z = F.ZERO_SNR_SPEC
    assert z.zero_snr and z.scheduler == "ddim" and z.freeu == F.FREEU and z.loras and list(F.PAIRWISE.values())[-1] is z


def test_zero_snr_needs_v_prediction():
    """why the zero-SNR spec is a v-prediction one: the product refuses the epsilon table at alphas_cumprod = 0"""
    from test_gpu_guidance_rescale import ZERO_SNR
    assert scheduler_kwargs(F.ZERO_SNR_SPEC) == dict(prediction_type="v_prediction", **ZERO_SNR)
    sch = product_scheduler(F.ZERO_SNR_SPEC.but(prediction="epsilon"))
    sch.set_timesteps(4)
    with pytest.raises(ValueError, match="needs prediction_type='v_prediction'"):
        sch.coefficient_table(False)
    ok = product_scheduler(F.ZERO_SNR_SPEC)
    ok.set_timesteps(4)
    assert int(ok.timesteps[0]) == 999 and ok.alphas_cumprod[999] == 0.0 and ok.coefficient_table(False).shape == (4, 5)


def test_every_generation_warms_up_captures_and_replays():
    """at least 3 executed steps per generation (eager, capture, replay).  A set of active nets is warmed up the first time
    it occurs and captured AND replayed the second time (DenoiseEngine._launch), so every set needs two steps; all have
    three, except (0,) in the 5-step generations of scenario b, whose windows the scenario fixes: (0, 1) three times, (0,)
    twice, and once more twice in each generation after the first."""
    specs = F.all_specs()
    assert len(specs) == (len(F.SCENARIO_A) + len(F.SCENARIO_B) + len(F.SCENARIO_C) + len(F.SCENARIO_D) + len(F.SCENARIO_G)
                          + len(F.LARGE) + len(F.PAIRWISE))
    two_sets = 0
    for what, spec in specs.items():
        assert executed_steps(spec) >= 3, what
        sets = active_sets(spec)
        assert sum(sets.values()) == executed_steps(spec), what
        if what.startswith("b: "):
            assert sets == {(0, 1): 3, (0,): 2}, (what, sets)
        else:
            assert all(n >= 3 for n in sets.values()), (what, sets)
        two_sets += len(sets) > 1
        assert spec.hw is None or spec.hw[0] * spec.hw[1] <= 72 * 64, what
    assert two_sets == len(F.SCENARIO_B) + 2


def test_tiny_models_emit_no_groupnorm_statistics_and_the_composed_case_does():
    """GEMM-epilogue GroupNorm statistics come out of the 160-wide tiles only (gemm_plan.hip check_stats), so no launch of a
    tiny model (64 / 128 channels) attaches ``_gn_stats`` at any size: scenario (e) runs the in-place updates above 256
    tokens, but no stale statistics can ride through them.  The launch the composed GPU case starts from does emit them, and
    the GroupNorm over its two outputs may use them."""
    from consistentid_amd import _lib, ops, unet_spec
    plan = lambda M, c, hw, **kw: ops.gemm_plan(M=M, N=c, c1=c, bias=True, ws=True, ws_bytes=ops.GEMM_WS_BYTES, gn_hw=hw, **kw)
    for name, spec in (("sd15", F.LARGE["ControlNet-inpaint, FreeU, plain net"]), ("sdxl", F.LARGE["SDXL, FreeU and a LoRA"])):
        cfg = unet_spec.tiny_config(name)
        assert all(c % 160 for c in cfg.block_out_channels)
        for lvl, c in enumerate(cfg.block_out_channels):
            h, w = spec.hw[0] >> lvl, spec.hw[1] >> lvl
            for kw in (dict(res=True, ldr=c, taps=9, Hi=h, Wi=w, Ho=h, Wo=w), dict(res=True, ldr=c),
                       dict(taps=9, Hi=2 * h, Wi=2 * w, Ho=h, Wo=w, stride=2), dict(taps=9, Hi=h // 2, Wi=w // 2, Ho=h, Wo=w, up=1)):
                assert plan(2 * spec.B * h * w, c, h * w, **kw)["stats_rows"] == 0, (name, lvl, kw)
    B, H, W, C = (F.STATS_SHAPE[k] for k in "BHWC")
    rows = plan(B * H * W, C, H * W, res=True, ldr=C)["stats_rows"]
    assert H * W > ops.GN_SMALL_MAX_HW and ops._stats_rows(rows, H * W, 0) > 0 and _lib.load().cid_groupnorm_stats_ok(C, C, 32)


def test_scenarios_are_the_sequences_they_claim():
    first = lambda rows: rows[0][1]
    assert F.SCENARIO_A[-1][1] == first(F.SCENARIO_A) and F.SCENARIO_C[-1][1] == first(F.SCENARIO_C)
    for rows in (F.SCENARIO_A, F.SCENARIO_C):       # one field (with the sampler: two) at a time, except the last step back
        for (_, a), (what, b) in zip(rows, rows[1:-1]):
            diff = [f.name for f in dataclasses.fields(Spec) if getattr(a, f.name) != getattr(b, f.name)]
            assert 1 <= len(diff) <= 2, (what, diff)
    g = [s for _, s in F.SCENARIO_G]        # a long context under the switches, down to 77 rows and back
    assert len(g) == 7 and g[0] == g[4] == g[6] == F.CN_A.but(text_len=154) and g[5] == F.CN_A and g[0].steps == 4
    assert [features_on(s) for s in g] == [[], ["loras"], ["freeu", "loras"], ["freeu", "rescale", "loras"], [], [], []]
    assert inputs(g[0], "cpu")["text"].shape[1] == 154 + 4 and inputs(g[0], "cpu") is inputs(g[3], "cpu") is not inputs(g[5], "cpu")
    d = F.SCENARIO_D
    assert d[-1][2] == d[0][2] and d[-2][2] == d[1][2] and d[-1][1] == "P1" and d[-2][1] == "P2"
    assert all(via is None or via != p for _, p, _, via, _ in d), "every switch of (d) is made through the OTHER pipeline"
    from test_gpu_freeu import FREEU
    assert F.FREEU == FREEU


def test_new_spec_fields_default_to_off_and_keep_the_memo_keys():
    s = Spec()
    assert (s.freeu, s.rescale, s.prediction, s.zero_snr, s.loras) == (None, 0.0, "epsilon", False, ())
    assert features_on(s) == [] and scheduler_kwargs(s) == {}
    # a spec written before the fields existed is equal to, and hashes like, the same spec today: the lru_cache entries of
    # fresh_eager / oracle_run are the ones they were
    assert Spec(pipe="inpaint", steps=5) == Spec(pipe="inpaint", steps=5, freeu=None, rescale=0.0, prediction="epsilon", zero_snr=False, loras=())
    for base in (Spec(), Spec(pipe="sdxl", guidance=7.5), F.CN_AB):
        other = base.but(freeu=F.FREEU, rescale=0.7, prediction="v_prediction", loras=F.LORA, scheduler="dpm")
        a, b = inputs(base, "cpu"), inputs(other, "cpu")
        assert a is b, "the inputs depend on the shapes and the seed only"


def test_memoised_fp32_oracle_is_unchanged_after_a_freeu_spec():
    import lora_cases as L
    o = oracle_models("cpu", "tiny")[0]
    before = L.oracle_forward(o, "tiny", lambda t: t.float())
    spec = Spec(steps=3, freeu=F.FREEU)
    assert not torch.equal(oracle_run(spec, "cpu"), oracle_run(spec.but(freeu=None), "cpu"))
    assert not hooked_modules(o)
    assert torch.equal(L.oracle_forward(o, "tiny", lambda t: t.float()), before)
