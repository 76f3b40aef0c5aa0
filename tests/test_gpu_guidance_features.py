"""Perturbed-attention guidance and self-attention guidance (4.29) on one live denoise engine with graphs on:
across engine reuse, among the schedulers, at ``strength`` < 1, under FreeU, community LoRAs, a second adapter, v-prediction, a
154-row context, SDXL's second unconditional set, the time-conditioned LCM UNet and a UNet shared by two pipelines.  Each of the
two was tested against the base paths only.  The scenarios are lists of engine_cases.Spec run by engine_cases.run_scenario:
EVERY generation must equal, bit for bit, the same spec run eagerly on fresh objects, report the step launch and the UNet
batch rows its spec names, and -- the first, the last and every one marked -- lie within the fp16 arm of the fp32 oracle
(pag_ref.PagUNet / sag_ref.SagUNet in front of the oracle UNet), with every feature it switches on moving that oracle by the
threshold of the feature's own tests.

The threshold trap of tests/test_gpu_sag.py holds for every SAG generation here: one that is compared with the oracle first
asserts conditions (a) - (c) of that module's docstring on the reference alone (engine_cases.assert_sag_reference) and then
also holds ``eng.sag_mass`` to the reference's last evaluation (engine_cases.check_masses).  Those specs run one sample on small
latents with an input seed chosen by tools/sag_seed_search.py at a factor of at least 17 against the CPU stand-in
(tests/test_guidance_features_host.py asserts the tool's target, 10); the seeds of the plain samplers are those of test_gpu_sag.CASES.  EVERY SAG
generation has the masses of its first evaluation -- which no earlier mask can have moved -- held to the reference's at 1.5 x the
arm's deviation (engine_cases.check_first_masses).  The few whose reference has no margin for a trajectory (``bits_only``: 64
mid-block tokens, LCM on the CFG path, DDIM with eta) are held to that, to the fresh eager bits and to the features' thresholds.

The lists are data: tests/test_guidance_features_host.py checks them without a GPU."""
import pytest
import torch

import engine_cases as E
from conftest import TOL_L2, rel_l2
from engine_cases import Gen, Spec, apply_features, call_pipeline, expected_step_path, new_unet, pipeline_class, run_scenario
from test_gpu_sag import CASES as SAG_CASES

pytestmark = pytest.mark.gpu

FREEU = (0.9, 0.2, 1.2, 1.4)        # test_gpu_freeu.FREEU
LORA = ((11, 1.0),)
LORA_07 = ((11, 0.7),)
# "mid" alone moves the tiny models' oracle least: 7e-2 at scale 3, against the 5e-2 - 9e-2 that ten times the tolerance comes
# to.  On the CPU (fp32 oracle, fp16 copy as the arm) what PAG moves over the arm's error -- which has to reach 15 -- is 31 - 49 at
# scale 6 and 40 - 69 at scale 10 under epsilon prediction.  Under v-prediction the arm's own error grows faster than what PAG
# moves (36 at scale 6, 21 at 10, and below 23 on SDXL or with one selected level only), so there "mid" runs at scale 6
PAG_MID, PAG_MID_V, PAG_DOWN, PAG_ALL = ("mid", 10.0, 0.0), ("mid", 6.0, 0.0), ("first-down", 3.0, 0.0), ("all", 3.0, 0.0)
SAG = 1.0


def _chain(base, changes):
    """[(what, spec)]: ``base``, then one change after another, each on top of the one before"""
    out, s = [("base", base)], base
    for what, change in changes:
        s = s.but(**change)
        out.append((what, s))
    return out


def _pipe(dev, spec, unet=None):
    if unet is None:
        unet = new_unet(str(dev), spec.name, keep_base=True, time_cond=spec.time_cond)
    return pipeline_class(spec)(unet, use_graph=True)


# --------------------------------------------------------------------------- 1. one txt2img engine, one change at a time
# test_gpu_sag.CASES["ddim"]: one sample on 12 x 12 latents (a 3 x 3 mid block), three steps, the embed switch after the first.
# (what, spec, further keywords of the call, captures the generation adds): the SAG scale is in the graph key, the PAG
# selection reaches it through the UNet's epoch, and an adaptive PAG scale is a step-table column (no capture)
ONE = SAG_CASES["ddim"]
PAG_ADAPTIVE = ("first-down", 6.0, 0.01)        # s_i = 2.67, 0, 0 at DDIM's timesteps 667, 334, 1: zero from the second step on
ONE_ENGINE = [
    ("plain", ONE, None, 1), ("SAG 1.0", ONE.but(sag=SAG), None, 1), ("SAG 0.5", ONE.but(sag=0.5), None, 1),
    ("sag_scale = 0 spelled out", ONE, dict(sag_scale=0.0), 1), ("PAG on mid", ONE.but(pag=PAG_MID), None, 1),
    ("PAG on the first down block", ONE.but(pag=PAG_DOWN), None, 1), ("PAG adaptive", ONE.but(pag=PAG_ADAPTIVE), None, 0),
    ("plain again", ONE, None, 1), ("SAG 1.0 again", ONE.but(sag=SAG), None, 1)]


GUIDANCE_STATICS = {"sag_coef", "sag_mass", "sag_xdeg", "sag_eps", "pag"}      # the buffers DenoiseEngine.run makes for the two


def test_one_engine_one_guidance_at_a_time(dev):
    """plain -> SAG 1.0 -> SAG 0.5 -> sag_scale = 0 -> PAG mid -> PAG first-down -> PAG adaptive (zero from the second step
    on) -> plain -> SAG 1.0.  The plain generations are the bits of a pipeline that never saw either keyword, and every static
    buffer such a pipeline holds has the same shape and bits in this engine afterwards."""
    fresh = _pipe(dev, ONE)
    plain, _ = call_pipeline(fresh, ONE, dev)
    plain = plain.clone()
    untouched = {k: v.clone() for k, v in fresh._engine._static.items()}
    assert not any(k.startswith(("sag", "pag")) for k in untouched) and len(fresh._engine.captures) == 1
    pipe = _pipe(dev, ONE)
    counts = []

    def look(is_plain):
        def after(eng):
            counts.append(len(eng.captures))
            # the engine never frees a static buffer: what a guided generation made stays, and no launch of a plain step reads it
            assert set(eng._static) - set(untouched) <= GUIDANCE_STATICS and set(untouched) <= set(eng._static)
            if len(counts) == 1:
                assert set(eng._static) == set(untouched), "before any guidance ran"
            if is_plain:
                for k, want in untouched.items():
                    got = eng._static[k]
                    assert got.shape == want.shape and got.dtype == want.dtype, f"static buffer {k}: {tuple(got.shape)}"
                    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), f"static buffer {k} of a plain call"
        return after
    gens = [Gen(what, s, oracle=True, extra=extra, same_graphs=added == 0, after=look(s == ONE)) for what, s, extra, added in ONE_ENGINE]
    outs = run_scenario(dev, "one engine, one guidance at a time", gens, pipe)
    added = [b - a for a, b in zip([0] + counts, counts)]
    assert added == [row[3] for row in ONE_ENGINE], f"captures per generation {added}"
    for n, (what, s, _, _) in enumerate(ONE_ENGINE):
        if s == ONE:
            assert torch.equal(outs[n], plain), f"generation {n} ({what}) is not the plain generation of a fresh pipeline"
    assert torch.equal(outs[8], outs[1]) and not torch.equal(outs[2], outs[1]) and not torch.equal(outs[5], outs[4])
    seen = E.guidance_trace(ONE.but(pag=PAG_ADAPTIVE), str(dev))[2]
    assert [s > 0.0 for s, _ in seen] == [True, False, False], seen
    assert float(pipe._engine._static["pag"]) == 0.0 and pipe.unet.pag_layers == ()


# --------------------------------------------------------------------------- 2. the latent size under SAG
# 32 x 32 latents: an 8 x 8 mid block, exactly the 64 tokens the axis is padded to (no copy of the real columns); 16 x 8: 4 x 2 of
# 64 (test_gpu_sag.CASES["non-square"], compared with the oracle); 192 cells per trajectory at the full size leave no margin
_FULL = Spec(scheduler="ddim", steps=3, merge=0, B=1, sag=SAG)
SIZES = [("32 x 32: the mid block fills the token axis", _FULL, True), ("16 x 8: 8 of 64 tokens", SAG_CASES["non-square"].but(sag=SAG), False),
         ("32 x 32 again", _FULL, True), ("16 x 8 again", SAG_CASES["non-square"].but(sag=SAG), False)]


def test_latent_size_under_sag(dev):
    pipe = _pipe(dev, _FULL)
    shapes = []
    gens = [Gen(what, s, oracle=True, bits_only=bits, after=lambda eng: shapes.append(tuple(eng.sag_mass.shape))) for what, s, bits in SIZES]
    outs = run_scenario(dev, "latent size under SAG", gens, pipe)
    assert shapes == [(1, 64), (1, 8), (1, 64), (1, 8)], shapes
    assert torch.equal(outs[2], outs[0]) and torch.equal(outs[3], outs[1])


# --------------------------------------------------------------------------- 3. the schedulers under each guidance
_LCM5 = SAG_CASES["lcm-single-pass"].but(guidance=5.0)
SAG_SCHEDULERS = [("DDIM", SAG_CASES["ddim"], False), ("Euler", SAG_CASES["euler"], False), ("DPM-Solver++ 2M", SAG_CASES["dpm"], False),
                  ("PNDM", SAG_CASES["pndm"], False), ("LCM at guidance 5: the CFG path", _LCM5, True),
                  ("LCM single pass", SAG_CASES["lcm-single-pass"], False), ("DDIM eta 1", SAG_CASES["ddim"].but(eta=1.0), True)]
SAG_SCHEDULERS = [(what, s.but(sag=SAG), bits) for what, s, bits in SAG_SCHEDULERS]
_P = Spec(steps=4, merge=1, pag=PAG_ALL)
PAG_SCHEDULERS = [("DDIM", _P), ("Euler", _P.but(scheduler="euler")), ("DPM-Solver++ 2M", _P.but(scheduler="dpm")),
                  ("PNDM", _P.but(scheduler="pndm")), ("LCM at guidance 5: the CFG path", _P.but(scheduler="lcm")),
                  ("LCM single pass", _P.but(scheduler="lcm", guidance=1.0)), ("DDIM eta 1", _P.but(eta=1.0))]


def test_schedulers_under_sag(dev):
    """the coefficient table is rebuilt from whatever scheduler the pipeline holds: every generation its own noise model"""
    gens = [Gen(what, s, oracle=True, bits_only=bits) for what, s, bits in SAG_SCHEDULERS]
    pipe = _pipe(dev, gens[0].spec)
    run_scenario(dev, "schedulers under SAG", gens, pipe)
    assert pipe._engine.step_path == "cfg_multistep+sag"


def test_schedulers_under_pag(dev):
    gens = [Gen(what, s, oracle=True, same_graphs=what == "Euler") for what, s in PAG_SCHEDULERS]      # DDIM -> Euler: one kernel, new rows
    pipe = _pipe(dev, _P)
    run_scenario(dev, "schedulers under PAG", gens, pipe)
    assert pipe._engine.step_path == "cfg_multistep+pag"


# --------------------------------------------------------------------------- 4. inpaint at strength < 1
# PAG, 5 steps at strength 0.6: the loop runs schedule entries 2, 3, 4 (DDIM's timesteps 401, 201, 1 of 801, 601, 401, 201, 1).  A
# per-step column read at the executed step, not at the schedule entry, gives the values of 801, 601, 401.  max(s - a (1000 - t), 0)
# only falls along a schedule, so "non-zero in the executed part alone" does not exist; the second spec's scale is positive in
# the first executed step and reaches zero inside the executed part.  SAG, 8 steps at strength 0.4: entries 5, 6, 7 (timesteps
# 251, 126, 1), where the noise model is far from that of entries 0, 1, 2 (876, 751, 626); at 5 steps and strength 0.6 the two
# indexings moved the reference by 1.4e-2 only.
INPAINT = Spec(pipe="inpaint", scheduler="ddim", steps=5, strength=0.6, merge=0, B=2)
INPAINT_SAG = Spec(pipe="inpaint", scheduler="ddim", steps=8, strength=0.4, merge=0, B=1, hw=(16, 8), seed=114, sag=SAG)
PAG_SKIPPED_ONLY = ("all", 3.0, 0.006)        # 1.806, 0.606 | 0, 0, 0
PAG_INTO_EXECUTED = ("all", 3.0, 0.0045)      # 2.1005, 1.2005 | 0.3045, 0, 0
STRENGTH = [("SAG", INPAINT_SAG), ("PAG, the scale positive in the skipped entries only", INPAINT.but(pag=PAG_SKIPPED_ONLY)),
            ("PAG, the scale reaches zero in the executed part", INPAINT.but(pag=PAG_INTO_EXECUTED)), ("SAG again", INPAINT_SAG)]


def test_inpaint_strength_reads_the_schedule_entry(dev):
    """first_step = 2 (SAG: 5): the ``sag_coef`` and ``pag`` columns are read at the schedule entry.  On the reference, the same
    generation with the column read at the executed step is at least 20 x TOL_L2 away (``misindexed``), so an engine that
    did that could not pass the oracle comparison; the first PAG generation is then the plain one's oracle."""
    gens = [Gen(what, s, oracle=True, misindexed=True) for what, s in STRENGTH]
    pipe = _pipe(dev, INPAINT)
    outs = run_scenario(dev, "inpaint at strength < 1 under a guidance", gens, pipe)
    skipped = STRENGTH[1][1]
    assert E.first_step(skipped) == 2 and all(s == 0.0 for s, _ in E.guidance_trace(skipped, str(dev))[2])
    # (3B rows against 2B through the same fp32 kernels: not the same bits)
    assert rel_l2(E.oracle_run(skipped, str(dev)), E.oracle_run(skipped.but(pag=None), str(dev))) < 1e-5
    assert [s > 0.0 for s, _ in E.guidance_trace(STRENGTH[2][1], str(dev))[2]] == [True, False, False]
    assert torch.equal(outs[3], outs[0])


# --------------------------------------------------------------------------- 5. one switch at a time under each guidance
_PB = Spec(steps=4, merge=1, pag=PAG_ALL)
PAG_SWITCHES = _chain(_PB, [
    ("FreeU on", dict(freeu=FREEU)), ("LoRA loaded", dict(loras=LORA)), ("FreeU off", dict(freeu=None)), ("LoRA unloaded", dict(loras=())),
    ("v-prediction", dict(prediction="v_prediction")), ("epsilon", dict(prediction="epsilon")), ("154 text rows", dict(text_len=154)),
    ("77 text rows", dict(text_len=77)), ("callback", dict(callback=True)), ("the second adapter", dict(callback=False, adapter=1))])
# every generation that is compared with the oracle has the seed the search found for ITS switches (new input values keep the graphs)
# (v-prediction: seed 23 at 8 x 8, not test_gpu_sag's 974 -- its last-evaluation masses were at 0.45 of the bound in the worst of three
# arm runs on the MI355X, 974's at 0.82 in one)
_SB = SAG_CASES["non-square"].but(sag=SAG)                       # 16 x 8 latents, seed 331
SAG_SWITCHES = [("base", _SB, False), ("FreeU on", _SB.but(freeu=FREEU, seed=51), False), ("FreeU off", _SB, False),
                ("LoRA loaded", _SB.but(loras=LORA, seed=249), False), ("LoRA unloaded", _SB, False),
                ("v-prediction", SAG_CASES["v-prediction"].but(sag=SAG, seed=23), False), ("epsilon", _SB, False),
                ("154 text rows", _SB.but(text_len=154, seed=0), False), ("77 text rows", _SB, False), ("callback", _SB.but(callback=True), False),
                ("the second adapter", _SB.but(adapter=1, seed=159), False)]


def _second_adapter(dev, pipe):
    ad2 = E.unet_models(str(dev), "tiny", 1)[2]
    return lambda: pipe.load_ConsistentID_model({"adapter_modules": ad2}, lora_rank=8)


def test_one_switch_at_a_time_under_pag(dev):
    """the folded Wo Wv of every selected layer follows the LoRA and the second adapter in place; the perturbed rows read the
    long K/V images the conditional rows read"""
    pipe = _pipe(dev, _PB)
    gens = [Gen(what, s, oracle=True) for what, s in PAG_SWITCHES]
    gens[-1].before = _second_adapter(dev, pipe)
    outs = run_scenario(dev, "switches under PAG", gens, pipe)
    assert torch.equal(outs[4], outs[0]) and torch.equal(outs[6], outs[0]) and torch.equal(outs[8], outs[0]) and torch.equal(outs[9], outs[0])
    assert not torch.equal(outs[10], outs[0]) and not torch.equal(outs[2], outs[1])


def test_one_switch_at_a_time_under_sag(dev):
    """a LoRA moves the mid block's to_q, hence the masses: ``sag_mass`` of every compared generation is the reference's"""
    pipe = _pipe(dev, _SB)
    gens = [Gen(what, s, oracle=True, bits_only=bits) for what, s, bits in SAG_SWITCHES]
    gens[-1].before = _second_adapter(dev, pipe)
    outs = run_scenario(dev, "switches under SAG", gens, pipe)
    for n in (2, 4, 6, 8, 9):
        assert torch.equal(outs[n], outs[0]), f"generation {n} ({SAG_SWITCHES[n][0]}) is not the base generation"
    assert not torch.equal(outs[10], outs[0])


# --------------------------------------------------------------------------- 6. SDXL
_XP = Spec(pipe="sdxl", steps=4, merge=1, guidance=7.5, pag=PAG_ALL)
SDXL_PAG = _chain(_XP, [("second unconditional set", dict(null_post=True)), ("new time_ids", dict(time_ids=(8, 16))),
                        ("LoRA loaded", dict(loras=LORA)), ("everything back", dict(loras=(), null_post=False, time_ids=(0, 0)))])
_XS = SAG_CASES["sdxl-null-post"].but(sag=SAG)              # 6 x 6 latents, seed 324
SDXL_SAG = [("second unconditional set", _XS, False), ("new time_ids, guidance 7.5", _XS.but(time_ids=(8, 16), guidance=7.5, seed=362), False),
            ("LoRA loaded", _XS.but(time_ids=(8, 16), guidance=7.5, loras=LORA, seed=970), False), ("LoRA unloaded, first time_ids, guidance 5", _XS, False)]
# B = 2, ONE evaluation after the merge (start_merge_step -1), masses only, as test_gpu_sag.TWO_SAMPLES: the guide rows of the
# second forward are the post-merge null set's and the first B rows of ``pooled`` / ``time_ids``
SDXL_TWO_SAMPLES = Spec(pipe="sdxl", scheduler="ddim", steps=1, merge=-1, guidance=7.5, B=2, hw=(8, 8), time_ids=(8, 16), null_post=True,
                        loras=LORA, sag=SAG)


def test_sdxl_under_pag(dev):
    def rows(spec):
        def after(eng):
            assert eng._static["pooled"].shape[0] == 3 * spec.B == eng._static["time_ids"].shape[0]
        return after
    gens = [Gen(what, s, oracle=True, same_graphs=what == "new time_ids", after=rows(s)) for what, s in SDXL_PAG]
    outs = run_scenario(dev, "SDXL under PAG", gens, _pipe(dev, _XP))
    assert torch.equal(outs[4], outs[0]) and not torch.equal(outs[2], outs[1])


def test_sdxl_under_sag(dev):
    gens = [Gen(what, s, oracle=True, bits_only=bits) for what, s, bits in SDXL_SAG]
    outs = run_scenario(dev, "SDXL under SAG", gens, _pipe(dev, _XS))
    assert torch.equal(outs[3], outs[0]) and not torch.equal(outs[1], outs[0]) and not torch.equal(outs[2], outs[1])


def test_sdxl_two_samples_masses(dev):
    """test_gpu_sag.test_two_samples_masses' checks on the merged step of SDXL with a LoRA: every mass within 1.5 x the fp16
    arm's largest deviation, every mask cell further than 4 x that deviation from the threshold equal, and on the reference
    the two samples' masses at least 10 x that deviation apart"""
    import numpy as np
    spec = SDXL_TWO_SAMPLES
    masses, arm_masses = E.guidance_trace(spec, str(dev))[0], E.guidance_trace(spec, str(dev), True)[0]
    assert len(masses) == 1 and masses[0].shape == (2, 16)
    want = torch.from_numpy(masses[0])
    dev_arm = float(np.abs(arm_masses[0] - masses[0]).max())
    apart = float((want[0] - want[1]).abs().max())
    pipe = pipeline_class(spec)(new_unet(str(dev), "tinyxl", keep_base=True), use_graph=False)
    apply_features(pipe, spec)
    call_pipeline(pipe, spec, dev)
    got = pipe.sag_mass.cpu().double()
    off = float((got - want).abs().max())
    print(f"[parity] SDXL two samples: largest mass deviation {off:.3e} | fp16 arm {dev_arm:.3e} -> tol {1.5 * dev_arm:.3e}; the samples' "
          f"masses are {apart:.3e} apart (needs >= {10 * dev_arm:.3e})")
    assert apart >= 10 * dev_arm
    assert tuple(got.shape) == tuple(want.shape) and torch.isfinite(got).all() and off <= 1.5 * dev_arm
    clear = (want - 1.0).abs() > 4.0 * dev_arm
    assert torch.equal((got > 1.0)[clear], (want > 1.0)[clear]) and int(clear.sum()) >= want.numel() // 2
    assert pipe._engine.step_path == "cfg_ddim+sag"


# --------------------------------------------------------------------------- 7. the time-conditioned LCM UNet
TC = Spec(scheduler="lcm", time_cond=True, steps=4, merge=1, guidance=3.0)
TC_SAG = Spec(scheduler="lcm", time_cond=True, steps=3, merge=0, guidance=3.0, B=1, hw=(16, 8), seed=131, sag=SAG)
TIME_COND = [("plain", TC), ("PAG", TC.but(pag=PAG_ALL)), ("SAG", TC_SAG), ("PAG at guidance 8", TC.but(pag=PAG_ALL, guidance=8.0)), ("plain again", TC)]


def test_time_cond_unet_under_each_guidance(dev):
    """the single pass at every guidance_scale: [cond | perturbed] rows under PAG, the conditional rows guide SAG"""
    gens = [Gen(what, s, oracle=True) for what, s in TIME_COND]
    outs = run_scenario(dev, "time_cond_proj_dim UNet under a guidance", gens, _pipe(dev, TC))
    assert torch.equal(outs[4], outs[0]) and not torch.equal(outs[3], outs[1])


# --------------------------------------------------------------------------- 8. both sides of ops.ln_fold's row limit
_F2 = Spec(steps=3, merge=1, pag=PAG_ALL)
LN_FOLD = [("B = 2: 2048 perturbed rows at level 0, folded", _F2), ("B = 3: 3072 rows, LayerNorm + GEMM", _F2.but(B=3)), ("B = 2 again", _F2)]


def test_pag_on_both_sides_of_the_fold_limit(dev):
    """no monkeypatch: at B = 3 the level-0 layers of ``all`` take the unfolded branch by themselves, inside a captured step"""
    from consistentid_amd import ops
    assert ops.ln_fold(2 * 1024) and not ops.ln_fold(3 * 1024)
    gens = [Gen(what, s, oracle=True) for what, s in LN_FOLD]
    outs = run_scenario(dev, "PAG across the LayerNorm-fold limit", gens, _pipe(dev, _F2))
    assert torch.equal(outs[2], outs[0])


# --------------------------------------------------------------------------- 9. one UNet under two pipelines
# (what, the pipeline that generates, its spec, the pipeline whose enable_pag / disable_pag brings the UNet there or None).
# pag = ("mid", 0, 0): the layers are selected (by the OTHER pipeline) and this call is a plain one
T2I, INP = Spec(steps=4, merge=1), Spec(pipe="inpaint", steps=4, merge=1)
_SEL = ("mid", 0.0, 0.0)
SHARED = [("P1", "P1", T2I, None), ("P1 after P2.enable_pag", "P1", T2I.but(pag=_SEL), "P2"), ("P2 with PAG", "P2", INP.but(pag=PAG_MID), None),
          ("P1 with SAG, P2's selection still set", "P1", ONE.but(sag=SAG, pag=_SEL), None),
          ("P1 after P2.disable_pag", "P1", T2I, "P2")]


def test_shared_unet_under_pag_and_sag(dev):
    unet = new_unet(str(dev), keep_base=True)
    pipes = {"P1": _pipe(dev, T2I, unet), "P2": _pipe(dev, INP, unet)}
    p1_captures = []

    def switch(via, spec):
        def before():
            p1_captures.append(len(pipes["P1"]._engine.captures))
            assert via is None or apply_features(pipes[via], spec), "the switch was a no-op"
        return before
    gens = [Gen(what, s, oracle=True, pipe=pipes[p], before=switch(via, s)) for what, p, s, via in SHARED]
    outs = run_scenario(dev, "a shared UNet under PAG and SAG", gens)
    assert torch.equal(outs[1], outs[0]), "P2.enable_pag moved P1's plain generation"
    assert torch.equal(outs[4], outs[0]), "P1 does not return to its first result"
    # P2's enable_pag reached P1's engine through the shared UNet's epoch: P1 captured again, once per generation since
    assert p1_captures == [0, 1, 2, 2, 3], f"P1's captures before each generation: {p1_captures}"
    assert len(pipes["P1"]._engine.captures) == 4 and len(pipes["P2"]._engine.captures) == 1


# --------------------------------------------------------------------------- 10. every pair of factor values
GUIDANCES = {"none": {}, "pag mid": dict(pag=PAG_MID), "pag all": dict(pag=PAG_ALL), "sag": dict(sag=SAG)}
PIPES = {"txt2img": Spec(steps=4, merge=1), "inpaint": Spec(pipe="inpaint", steps=4, merge=1), "sdxl": Spec(pipe="sdxl", steps=4, merge=1, guidance=7.5)}
SAMPLERS = {"ddim": dict(scheduler="ddim"), "euler": dict(scheduler="euler"), "dpm": dict(scheduler="dpm"), "pndm": dict(scheduler="pndm"),
            "lcm single": dict(scheduler="lcm", guidance=1.0)}
FACTORS = {"guidance": tuple(GUIDANCES), "pipe": tuple(PIPES), "sampler": tuple(SAMPLERS), "prediction": ("epsilon", "v_prediction"),
           "freeu": (False, True), "loras": (False, True)}
# Under v-prediction the stock fp16 arm is 1e-2 - 7e-2 from the fp32 oracle on these weights, and ten times the tolerance is more
# than PAG on one level, or on SDXL, moves: the rows with PAG and v-prediction are the combinations measured (on the CPU) to
# leave room -- "mid" on inpaint under the LCM single pass, "all" on the SD1.5 pipelines; SDXL meets v-prediction in the other rows
PAIRWISE_ROWS = [
    # guidance, pipe,      sampler,      prediction,     freeu, loras
    ("none",    "txt2img", "ddim",       "v_prediction", True,  True),
    ("none",    "txt2img", "dpm",        "epsilon",      True,  True),
    ("none",    "inpaint", "pndm",       "v_prediction", False, True),
    ("none",    "sdxl",    "euler",      "epsilon",      True,  False),
    ("none",    "sdxl",    "lcm single", "v_prediction", True,  False),
    ("pag mid", "txt2img", "ddim",       "epsilon",      True,  False),
    ("pag mid", "inpaint", "dpm",        "epsilon",      True,  False),
    ("pag mid", "inpaint", "pndm",       "epsilon",      True,  False),
    ("pag mid", "inpaint", "lcm single", "v_prediction", False, True),
    ("pag mid", "sdxl",    "euler",      "epsilon",      False, True),
    ("pag all", "txt2img", "euler",      "v_prediction", False, True),
    ("pag all", "txt2img", "pndm",       "v_prediction", False, False),
    ("pag all", "txt2img", "lcm single", "epsilon",      True,  True),
    ("pag all", "inpaint", "ddim",       "v_prediction", True,  False),
    ("pag all", "sdxl",    "dpm",        "epsilon",      True,  False),
    ("sag",     "txt2img", "dpm",        "v_prediction", False, False),
    ("sag",     "inpaint", "euler",      "epsilon",      True,  False),
    ("sag",     "inpaint", "lcm single", "epsilon",      False, False),
    ("sag",     "sdxl",    "ddim",       "epsilon",      False, True),
    ("sag",     "sdxl",    "pndm",       "epsilon",      True,  False),
]
# what the engine refuses is in no row: (what, the pipe, further keywords of the call)
REFUSED = [("PAG with SAG", "txt2img", dict(pag_scale=3.0, sag_scale=1.0)),
           ("PAG with guidance_rescale", "txt2img", dict(pag_scale=3.0, guidance_rescale=0.7)),
           ("SAG with guidance_rescale", "inpaint", dict(sag_scale=1.0, guidance_rescale=0.7)),
           ("PAG with a ControlNet", "controlnet", dict(pag_scale=3.0)), ("SAG with a ControlNet", "controlnet", dict(sag_scale=1.0)),
           ("PAG with SAG on SDXL", "sdxl", dict(pag_scale=3.0, sag_scale=1.0))]


# the SAG rows, as every SAG generation that is compared with the oracle: one sample, three UNet evaluations with the embed switch
# after the first (PNDM: two steps), and per row the latent size and input seed tools/sag_seed_search.py found for its switches
# (factor 17 at the least on the CPU stand-in).  The GPU's stock fp16 arm does not repeat itself: its largest mass deviation on
# one spec moved by a factor of two between three runs in one process.  So among the seeds the search gave, each row has the one
# whose figures on the MI355X leave most room in the worst of three arm runs: condition (c) at 16.0 (DPM-Solver++ v-prediction,
# seed 14), 16.2 (inpaint Euler FreeU, seed 58) and 6.9 (SDXL PNDM FreeU, seed 2001: the arm's deviation is 1.9e-2 - 2.5e-2 there
# and 4800 seeds at 6 x 6, the smallest latent cid_sag_degrade_f16 takes on that model, gave no better), and the engine's
# last-evaluation masses at 0.15, 0.29 and 0.29 of 1.5 x the SMALLEST of the three arm deviations.
SAG_ROWS = {("txt2img", "dpm"): dict(hw=(8, 8), seed=14), ("inpaint", "euler"): dict(hw=(16, 8), seed=58),
            ("inpaint", "lcm single"): dict(hw=(16, 8), seed=2), ("sdxl", "ddim"): dict(hw=(6, 6), seed=189),
            ("sdxl", "pndm"): dict(hw=(6, 6), seed=2001, steps=2)}


def pairwise_spec(guidance, pipe, sampler, prediction, freeu, loras):
    s = PIPES[pipe].but(prediction=prediction, freeu=FREEU if freeu else None, loras=LORA_07 if loras else (),
                        **{**SAMPLERS[sampler], **GUIDANCES[guidance]})
    if guidance == "pag mid" and prediction == "v_prediction":
        s = s.but(pag=PAG_MID_V)
    return s.but(B=1, **{**dict(steps=3, merge=0), **SAG_ROWS[pipe, sampler]}) if guidance == "sag" else s


PAIRWISE = {f"{r[0]}, {r[1]}, {r[2]}, {r[3]}{', FreeU' if r[4] else ''}{', LoRA' if r[5] else ''}": pairwise_spec(*r) for r in PAIRWISE_ROWS}


@pytest.mark.parametrize("case", list(PAIRWISE))
def test_pairwise(dev, case):
    """two generations on one new pipeline: warm-up and capture in the first, the second replays only"""
    spec = PAIRWISE[case]
    pipe = _pipe(dev, spec)
    gens = [Gen("warm-up and capture", spec, oracle=True), Gen("replay", spec, oracle=True, same_graphs=True)]
    a, b = run_scenario(dev, case, gens, pipe)
    assert len(pipe._engine.captures) == 1 and torch.equal(a, b)
    assert pipe._engine.step_path == expected_step_path(spec)


@pytest.mark.parametrize("case", [r[0] for r in REFUSED])
def test_refused_pairs_raise_before_any_launch(dev, case):
    """NotImplementedError, and the engine has neither a step launch nor a static buffer afterwards"""
    _, kind, extra = {r[0]: r for r in REFUSED}[case]
    spec = Spec(pipe=kind, steps=3, **(dict(nets=("A",), scales=(0.5,), windows=((0.0, 1.0),)) if kind == "controlnet" else {}))
    kw = {"controlnet": E.new_net(str(dev), "A")} if kind == "controlnet" else {}
    pipe = pipeline_class(spec)(new_unet(str(dev), spec.name, keep_base=True), use_graph=True, **kw)
    with pytest.raises(NotImplementedError):
        call_pipeline(pipe, spec, dev, extra)
    eng = pipe._engine
    assert eng.step_path is None and not eng._static and not eng.captures and not eng._warm_keys


def all_specs():
    """{label: (spec, bits_only)} of every generation of the lists above"""
    out = {}
    for name, rows in (("1", [(w, s, False) for w, s, _, _ in ONE_ENGINE]), ("2", SIZES), ("3s", SAG_SCHEDULERS),
                       ("3p", [(w, s, False) for w, s in PAG_SCHEDULERS]), ("4", [(w, s, False) for w, s in STRENGTH]),
                       ("5p", [(w, s, False) for w, s in PAG_SWITCHES]), ("5s", SAG_SWITCHES), ("6p", [(w, s, False) for w, s in SDXL_PAG]),
                       ("6s", SDXL_SAG), ("7", [(w, s, False) for w, s in TIME_COND]), ("8", [(w, s, False) for w, s in LN_FOLD]),
                       ("9", [(w, s, False) for w, _, s, _ in SHARED])):
        out.update({f"{name}: {n} {what}": (s, bits) for n, (what, s, bits) in enumerate(rows)})
    out.update({f"10: {k}": (s, False) for k, s in PAIRWISE.items()})
    return out
