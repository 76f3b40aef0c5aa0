"""Host-side checks of the LCM scenarios of tests/test_gpu_engine_reuse.py, tests/test_gpu_engine_features.py and
tests/test_gpu_taesd.py, which are plain data, and of the LCM branch of tests/engine_cases.py: every generation runs enough
steps, the sequences are the ones they claim, every FreeU / LoRA switch moves the single-pass fp32 oracle by the threshold of
its own tests, guidance 1 and 2 (3 and 8 on the time-cond UNet) are far apart, ``oracle_run`` is test_gpu_lcm's reference,
and the single-pass row selectors stay inside the conditional K/V rows.  No GPU."""
import pytest
import torch

import engine_cases as E
import test_gpu_engine_features as F
import test_gpu_engine_reuse as R
from engine_cases import Spec, active_sets, executed_steps, expected_step_path, features_on, single_pass


def _reuse_scenarios():
    return {"one change": [s for _, s in R.LCM_ONE_CHANGE], "schedulers": [s for _, s in R.LCM_AMONG_SCHEDULERS],
            "sdxl": [s for _, s in R.SDXL_LCM], "shared": [s for _, _, s in R.SHARED_LCM],
            "time_cond": [s for _, _, s in R.TIME_COND]}


def _all_new_specs():
    from test_gpu_taesd import few_step_spec
    out = dict(F.lcm_specs())
    for name, specs in _reuse_scenarios().items():
        out.update({f"{name}: {n}": s for n, s in enumerate(specs)})
    out["taesd: few-step"] = few_step_spec()
    return out


def test_every_lcm_generation_warms_up_captures_and_replays():
    """4 steps (3 where the scenario says so), at least 3 executed, at most 8 generations a scenario; every set of active nets
    runs twice (warm-up, then capture and replay) except (0, 1) at strength 0.75, which the generations before captured"""
    for name, specs in {**_reuse_scenarios(), "h": [s for _, s in F.SCENARIO_H], "i": [s for _, s in F.SCENARIO_I]}.items():
        assert len(specs) <= 8, name
    for what, spec in _all_new_specs().items():
        assert spec.steps in (3, 4) and executed_steps(spec) >= 3 and spec.hw is None and spec.B in (1, 2), what
        sets = active_sets(spec)
        assert sum(sets.values()) == executed_steps(spec), what
        if what.startswith("i: ") and len(sets) > 1:
            assert sets == ({(0, 1): 2, (0,): 2} if spec.strength == 1.0 else {(0, 1): 1, (0,): 2}), (what, sets)
        else:
            assert len(sets) == 1, (what, sets)


def test_lcm_scenarios_are_the_sequences_they_claim():
    lcm1, path = R.LCM, [expected_step_path(s) for _, s in R.LCM_ONE_CHANGE]
    assert single_pass(lcm1) and not single_pass(lcm1.but(guidance=2.0)) and not single_pass(Spec(scheduler="dpm", guidance=1.0))
    assert path == ["multistep", "cfg_multistep"] + ["multistep"] * 6
    assert [s.scheduler for _, s in R.LCM_AMONG_SCHEDULERS] == ["ddim", "lcm", "dpm", "lcm", "pndm", "lcm", "ddim", "lcm"]
    assert [expected_step_path(s) for _, s in R.LCM_AMONG_SCHEDULERS] == [
        "cfg_ddim", "multistep", "cfg_multistep", "multistep", "cfg_multistep", "cfg_multistep", "cfg_multistep", "multistep"]
    # the noise rows: LCM's z has one row less than DDIM eta's
    eta, = [s for _, s in R.LCM_AMONG_SCHEDULERS if s.eta > 0.0]
    assert E.inputs(eta, "cpu")["variance_noise"].shape[0] == executed_steps(eta) == executed_steps(lcm1) == 4
    assert [single_pass(s) for _, s in R.SDXL_LCM] == [True, True, False, False, True]
    assert [s.null_post for _, s in R.SDXL_LCM] == [False, True, True, True, True]
    assert [(p, single_pass(s)) for _, p, s in R.SHARED_LCM] == [("P1", True), ("P2", False), ("P1", True), ("P2", False), ("P1", True)]
    assert all(single_pass(s) and s.time_cond for _, _, s in R.TIME_COND) and R.TIME_COND[-1][2] == R.TIME_COND[0][2]
    assert [s.guidance for _, _, s in R.TIME_COND] == [3.0, 8.0, 3.0, 3.0, 3.0]
    h = [s for _, s in F.SCENARIO_H]
    assert all(single_pass(s) for s in h) and h[4] == h[0] and h[3] == h[2].but(rescale=F.PHI)
    assert [features_on(s) for s in h] == [[], ["loras"], ["freeu", "loras"], ["freeu", "loras"], [], [], ["freeu", "loras"], ["freeu", "loras"]]
    assert [s.text_len for s in h] == [77] * 5 + [154, 154, 77]
    i = [s for _, s in F.SCENARIO_I]
    assert [single_pass(s) for s in i] == [True] * 5 + [False, True] and all(s.multi and s.nets == ("A", "B") for s in i)
    for first, second in F.PAIRWISE_LCM.values():
        assert single_pass(first) and first.scheduler == second.scheduler == "lcm" and first != second


def test_lcm_specs_get_their_noise_and_their_scheduler(monkeypatch):
    from consistentid_amd import scheduler
    from lcm_ref import LCMLoopRef
    spec = R.LCM
    assert type(E.product_scheduler(spec)) is scheduler.LCMScheduler
    calls = []

    class Pipe:
        def __call__(self, **kw):
            calls.append(kw)
            return type("Out", (), {"images": torch.zeros(1)})()
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    for s in (spec, spec.but(steps=1), spec.but(pipe="inpaint", strength=0.75), spec.but(rescale=0.7)):
        E.call_pipeline(Pipe(), s, torch.device("cpu"))
    noise = E.inputs(spec, "cpu")["variance_noise"]
    assert torch.equal(calls[0]["variance_noise"], noise[:3]) and "eta" not in calls[0]
    assert "variance_noise" not in calls[1], "a single step takes no noise"
    assert tuple(calls[2]["variance_noise"].shape[:1]) == (2,)
    assert calls[3]["guidance_rescale"] == 0.7, "an inert argument still goes to the pipeline call"
    ref = E.reference_scheduler(spec, list(noise.float()))
    assert isinstance(ref, LCMLoopRef) and len(ref.noises) == 3 and [int(t) for t in ref.timesteps] == [
        int(t) for t in _timesteps(E.product_scheduler(spec), 4)]


def _timesteps(sch, n):
    sch.set_timesteps(n)
    return sch.timesteps


@pytest.mark.parametrize("label", [k for k, s in _all_new_specs().items() if features_on(s)])
def test_switches_move_the_single_pass_oracle(label):
    """every new spec that switches FreeU or a LoRA on, on the fp32 oracle alone: the thresholds are those of the features' own
    tests (20 * TOL_L2, lora_cases.MATTERS), at guidance 1 on the conditional rows only"""
    spec = _all_new_specs()[label]
    assert set(features_on(spec)) <= {"freeu", "loras"}
    E.assert_features_matter(spec, "cpu")


@pytest.mark.parametrize("spec", [R.LCM, F._I1, R.XL_LCM.but(null_post=True), R.TC], ids=["txt2img", "multi", "sdxl", "time_cond"])
def test_guidance_values_are_far_apart(spec):
    other = 8.0 if spec.time_cond else 2.0
    E.assert_features_matter(spec, "cpu", guidance_vs=other)


def test_inert_rescale_and_ignored_null_post_leave_the_oracle_alone():
    """guidance_rescale and the second unconditional set do not reach a single pass: the reference run is the same one"""
    assert torch.equal(E.oracle_run(R.LCM.but(rescale=0.7), "cpu"), E.oracle_run(R.LCM, "cpu"))
    xl = R.XL_LCM
    assert torch.equal(E.oracle_run(xl.but(null_post=True), "cpu"), E.oracle_run(xl, "cpu"))
    assert not torch.equal(E.oracle_run(xl.but(null_post=True, guidance=2.0), "cpu"), E.oracle_run(xl.but(guidance=2.0), "cpu"))


@pytest.mark.parametrize("kind", ["txt2img", "inpaint", "sdxl", "controlnet"])
def test_oracle_run_is_the_reference_of_test_gpu_lcm(kind):
    """``oracle_run`` of an "lcm" spec at guidance 1 and test_gpu_lcm._oracle_pair's fp32 result take the same path through
    ``oracle.loop.denoise``: the same tensor, exactly"""
    import test_gpu_lcm as L
    spec = L._spec(kind, 1.0, strength=0.75 if kind == "inpaint" else 1.0).but(scheduler="lcm")
    # (_oracle_pair computes the arm too: on the CPU that is the fp16 copy of the oracle; only the fp32 result is compared)
    want = L._oracle_pair(spec, torch.device("cpu"))[0]
    assert torch.equal(E.oracle_run(spec, "cpu"), want)
    assert not torch.equal(E.oracle_run(spec.but(guidance=2.0), "cpu"), want)


@pytest.mark.parametrize("B", [1, 2, 3])
def test_single_pass_selectors_stay_in_the_conditional_rows(B):
    """``step_rows(..., single_pass=True)``: [B, 2B) up to the merge, [2B, 3B) after it.  tests/test_lcm_host.py covers
    ``first_step`` 0 and 1 without a second unconditional set and holds the ControlNets' selector to the CFG one.  New here:
    (a) ``null_embeds_post`` present -- the K/V cache has 4B rows and the CFG selector moves its unconditional half to
    [3B, 4B); the single pass must not; (b) that with ``controlnet=False`` and with a ControlNet, whose selector stays in its
    own 2B-row cache; (c) that with ``first_step`` up to 2 of 4 and a merge step inside, at and beyond the executed window;
    (d) B = 3."""
    from consistentid_amd.denoise import step_rows
    n_ts = 4
    for first in (0, 1, 2):
        for merge in (0, 1, 10):
            for cn in (False, True):
                rows = step_rows(n_ts, first, merge, B, True, controlnet=cn, single_pass=True)
                plain = step_rows(n_ts, first, merge, B, False, controlnet=cn, single_pass=True)
                cfg = step_rows(n_ts, first, merge, B, True, controlnet=cn)
                assert tuple(rows.unet.shape) == (n_ts, B) and rows.unet.dtype == torch.int32
                assert torch.equal(rows.unet, plain.unet), "null_embeds_post shifted the single-pass rows"
                assert torch.equal(rows.unet, cfg.unet[:, B:]), "the single pass is not the conditional half of the CFG selector"
                for i in range(n_ts):
                    merged = (i - first) > merge
                    lo = 2 * B if merged else B
                    assert rows.unet[i].tolist() == list(range(lo, lo + B)) and bool(rows.merged[i]) == merged
                    if merged:
                        assert cfg.unet[i, :B].tolist() == list(range(3 * B, 4 * B))
                assert int(rows.unet.min()) >= B and int(rows.unet.max()) < 3 * B
                if cn:
                    assert torch.equal(rows.controlnet, cfg.controlnet) and int(rows.controlnet.max()) < 2 * B
                else:
                    assert rows.controlnet is None
