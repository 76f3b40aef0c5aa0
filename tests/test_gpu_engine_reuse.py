"""One denoise engine across differing generations.  A scenario is a list of generations (engine_cases.Spec) run on one live
pipeline with use_graph=True; after every generation the latents (and with a callback every per-step clone) must equal, bit
for bit, the same spec run eagerly on objects nothing else has touched (engine_cases.fresh_eager): a replay issues the same
launches on the same values, so a difference means the graph read something that was not this generation's.  The first and
the last generation and every one that follows a change of net or UNet are also held to the fp32 oracle within the fp16 arm
(conftest.check_vs_fp16_arm, defaults), so two engines that are wrong in the same way cannot agree their way through.  Where
the engine promises to keep its graphs ``len(eng.captures)`` must not grow; elsewhere the count is printed
as an ``[engine]`` line.  Every generation has at least 3 steps on one set of active nets: eager, capture, replay."""
import pytest
import torch

from engine_cases import Gen, Spec, new_net, new_unet, pipeline_class, unet_models
from engine_cases import run_scenario as _run       # (Gen and the runner live in engine_cases: test_gpu_engine_features shares them)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- 1. txt2img
def test_txt2img_one_change_at_a_time(dev):
    base = Spec(steps=4, merge=1, guidance=5.0)
    cfg = unet_models(str(dev))[0]
    assert (24, 40) != (cfg.sample_size, cfg.sample_size)
    s = base
    gens = [Gen("base", s)]
    for what, change, promised in (
            ("merge 2", dict(merge=2), True), ("6 steps", dict(steps=6), False), ("4 steps", dict(steps=4), False),
            ("guidance 7.5", dict(guidance=7.5), False), ("B = 1", dict(B=1), False), ("B = 2", dict(B=2), False),
            ("24 x 40 latents", dict(hw=(24, 40)), False), ("square latents", dict(hw=None), False),     # (test_tiny_unet_odd_resolution)
            ("32 text tokens", dict(text_len=32), False), ("77 text tokens", dict(text_len=77), False),  # (32, 4): attention edges
            ("new values", dict(seed=5), True), ("callback", dict(callback=True), False)):
        s = s.but(**change)
        gens.append(Gen(what, s, same_graphs=promised, oracle=what in ("24 x 40 latents", "32 text tokens")))
    pipe = pipeline_class(base)(new_unet(str(dev)), use_graph=True)
    _run(dev, "txt2img", gens, pipe)


# --------------------------------------------------------------------------- 2. schedulers
def test_schedulers_on_one_pipeline(dev):
    base = Spec(steps=4, merge=1)
    gens = [Gen("DDIM", base), Gen("Euler", base.but(scheduler="euler"), same_graphs=True),
            Gen("DPM-Solver++ 2M", base.but(scheduler="dpm")), Gen("PNDM", base.but(scheduler="pndm")),
            Gen("DDIM eta 1", base.but(eta=1.0)), Gen("DDIM eta 0", base)]
    pipe = pipeline_class(base)(new_unet(str(dev)), use_graph=True)
    outs = _run(dev, "schedulers", gens, pipe)
    assert torch.equal(outs[-1], outs[0]), "DDIM at eta 0 after five other step kernels is not the DDIM it started with"
    assert pipe._engine.step_path == "cfg_ddim"


# --------------------------------------------------------------------------- 3. inpaint
def test_inpaint_strength_windows(dev):
    """strength 1.0 -> 0.6 -> 1.0 at 5 steps (first_step 0 -> 2 -> 0), DDIM then DPM-Solver++: the solver's history starts
    empty at ``first_step`` every time, or the bits (and the oracle, which every generation here is held to) differ"""
    base = Spec(pipe="inpaint", steps=5, merge=1, guidance=7.5)
    gens = []
    for sch in ("ddim", "dpm"):
        s = base.but(scheduler=sch)
        gens += [Gen(f"{sch}, strength 1.0", s, oracle=True, same_graphs=False),
                 Gen(f"{sch}, strength 0.6", s.but(strength=0.6), oracle=True, same_graphs=True),
                 Gen(f"{sch}, strength 1.0 again", s, oracle=True, same_graphs=True)]
    pipe = pipeline_class(base)(new_unet(str(dev)), use_graph=True)
    _run(dev, "inpaint", gens, pipe)


# --------------------------------------------------------------------------- 4. ControlNet identity
CN = Spec(pipe="controlnet", steps=4, merge=1, guidance=5.0)


def _one(label, scale=0.5):
    return CN.but(nets=(label,), scales=(scale,), windows=((0.0, 1.0),))


def test_controlnet_identity_plain(dev):
    """net A -> a fresh net B -> A again -> no control image -> A.  The graphs are keyed by the INDEX of the nets that run,
    (0,) for either net; A's buffers do not move when it comes back."""
    nets = {k: new_net(str(dev), k) for k in "AB"}                          # held for the whole test
    gens = [Gen("net A", _one("A")), Gen("fresh net B", _one("B"), oracle=True), Gen("net A again", _one("A"), oracle=True),
            Gen("no control image", CN, oracle=True), Gen("net A", _one("A"), oracle=True)]
    pipe = pipeline_class(CN)(new_unet(str(dev)), controlnet=nets["A"], use_graph=True)
    _run(dev, "plain ControlNet", gens, pipe, nets)


def test_controlnet_identity_multi(dev):
    """[A, B] -> a new HipMultiControlNet([B, A]) with images and scales swapped to match -> [A] -> [A, B]; the engine's key
    says ("multi", 2) for both orders.  Then the two transitions of a MultiControlNet that keep the graphs: new scales, and
    guidance windows that leave the sets of active nets as they were.  Precomputed residuals beside control images are
    refused as before."""
    nets = {k: new_net(str(dev), k) for k in "AB"}
    two = lambda a, b, sa, sb: CN.but(nets=(a, b), multi=True, scales=(sa, sb), windows=((0.0, 1.0), (0.0, 1.0)))
    ab = two("A", "B", 0.5, 0.8)
    gens = [Gen("[A, B]", ab), Gen("[B, A]", two("B", "A", 0.8, 0.5), oracle=True),
            Gen("[A]", CN.but(nets=("A",), multi=True, scales=(0.5,), windows=((0.0, 1.0),)), oracle=True),
            Gen("[A, B]", ab, oracle=True), Gen("[A, B], new scales", ab.but(scales=(0.3, 0.9)), same_graphs=True),
            # 5 steps: (0, 1) three times, then (0,) twice, so both are captured within the generation
            Gen("5 steps, B's window ends at 0.6", ab.but(steps=5, windows=((0.0, 1.0), (0.0, 0.6)))),
            Gen("B's window ends at 0.7: the same active sets", ab.but(steps=5, windows=((0.0, 1.0), (0.0, 0.7))), same_graphs=True)]
    pipe = pipeline_class(CN)(new_unet(str(dev)), controlnet=[nets["A"], nets["B"]], use_graph=True)
    _run(dev, "MultiControlNet", gens, pipe, nets)
    with pytest.raises(ValueError, match="pass either control_image"):
        pipe(prompt_embeds=torch.zeros(6, 81, 8), latents=torch.zeros(2, 4, 8, 8), control_image=[torch.zeros(2, 3, 64, 64)] * 2,
             image_latents=torch.zeros(2, 4, 8, 8), noise=torch.zeros(2, 4, 8, 8), mask_latents=torch.zeros(2, 1, 8, 8),
             num_inference_steps=4, output_type="latent", down_block_res_samples=[torch.zeros(2, 64, 8)],
             mid_block_res_sample=torch.zeros(2, 64, 8))


# --------------------------------------------------------------------------- 5. one UNet under two pipelines
def test_shared_unet_under_two_pipelines(dev):
    """P1 (txt2img) at B = 2, P2 (inpaint) at B = 1 and B = 2 -- the UNet's K/V buffers move twice -- then P1 at B = 2 again:
    ``set_context`` keeps the buffers it finds, which are not the ones P1's graph was captured with.  Then P2 loads a second
    adapter into the shared UNet and P1 runs: it must see the new weights (a fresh UNet built with that adapter, and its
    oracle)."""
    unet = new_unet(str(dev), keep_base=True)
    t2i, inp = Spec(steps=4, merge=1), Spec(pipe="inpaint", steps=4, merge=1)
    p1 = pipeline_class(t2i)(unet, use_graph=True)
    p2 = pipeline_class(inp)(unet, use_graph=True)
    ad2 = unet_models(str(dev), "tiny", 1)[2]
    gens = [Gen("P1, B = 2", t2i, pipe=p1), Gen("P2, B = 1", inp.but(B=1), pipe=p2, oracle=True),
            Gen("P2, B = 2", inp, pipe=p2, oracle=True), Gen("P1, B = 2 again", t2i, pipe=p1, oracle=True),
            Gen("P1 after P2 loaded a second adapter", t2i.but(adapter=1), pipe=p1, oracle=True,
                before=lambda: p2.load_ConsistentID_model({"adapter_modules": ad2}, lora_rank=8)),
            Gen("P2 with the second adapter", inp.but(adapter=1), pipe=p2, oracle=True)]
    _run(dev, "shared UNet", gens)


# --------------------------------------------------------------------------- 6. SDXL
def test_sdxl_one_change_at_a_time(dev):
    base = Spec(pipe="sdxl", steps=4, merge=1, guidance=7.5)
    s = base
    gens = [Gen("base", s)]
    for what, change, promised in (
            ("second unconditional set", dict(null_post=True), False), ("one unconditional set", dict(null_post=False), False),
            ("new time_ids", dict(time_ids=(8, 16)), True), ("new values", dict(seed=3), True), ("3 steps", dict(steps=3), False)):
        s = s.but(**change)
        gens.append(Gen(what, s, same_graphs=promised, oracle="unconditional" in what))
    pipe = pipeline_class(base)(new_unet(str(dev), "tinyxl"), use_graph=True)
    _run(dev, "SDXL", gens, pipe)


# --------------------------------------------------------------------------- 7. the LCM single pass on a live engine
# LCMScheduler at guidance_scale <= 1 runs the B conditional rows and cid_multistep_step_f16; every other generation 2B rows
# and a CFG step.  ``kvrow``, ``pooled``, ``time_ids`` and the UNet workspace change size between the two while ``lat``,
# ``ms_hist``, ``ms_saved`` and ``ms_row`` keep theirs; engine_cases.run_scenario holds every generation to the step launch and
# the UNet batch rows its spec names, beside the fresh eager bits.  The scenarios are data: tests/test_lcm_engine_host.py
# checks their shape without a GPU.
LCM = Spec(scheduler="lcm", steps=4, merge=1, guidance=1.0)
FULL = (0.0, 1.0)


def _chain(base, changes):
    """[(what, spec)]: ``base``, then one change after another, each on top of the one before"""
    out, s = [("base", base)], base
    for what, change in changes:
        s = s.but(**change)
        out.append((what, s))
    return out


LCM_ONE_CHANGE = _chain(LCM, [
    ("guidance 2: the CFG path, 2B rows", dict(guidance=2.0)), ("guidance 1 again", dict(guidance=1.0)),
    ("3 steps: z loses a row", dict(steps=3)), ("B = 1", dict(B=1)), ("B = 2", dict(B=2)), ("merge 2", dict(merge=2)),
    ("callback", dict(callback=True))])

_T2I = Spec(steps=4, merge=1)
_LCM2 = LCM.but(guidance=2.0)
LCM_AMONG_SCHEDULERS = [
    ("DDIM at guidance 5", _T2I), ("LCM at guidance 1", LCM), ("DPM-Solver++ at guidance 1: 2B rows on LCM's ring", _T2I.but(scheduler="dpm", guidance=1.0)),
    ("LCM at guidance 1 again", LCM), ("PNDM at guidance 5", _T2I.but(scheduler="pndm")), ("LCM at guidance 2", _LCM2),
    ("DDIM eta 0.5: its own z, one row more than LCM's", _T2I.but(eta=0.5)), ("LCM at guidance 1", LCM)]

XL_LCM = Spec(pipe="sdxl", scheduler="lcm", steps=4, merge=1, guidance=1.0)
SDXL_LCM = _chain(XL_LCM, [
    ("second unconditional set, which the single pass ignores", dict(null_post=True)), ("guidance 2: it matters now", dict(guidance=2.0)),
    ("new time_ids", dict(time_ids=(8, 16))), ("guidance 1", dict(guidance=1.0))])

_INP = Spec(pipe="inpaint", steps=4, merge=1)
SHARED_LCM = [("P1: LCM single pass", "P1", LCM), ("P2: DDIM inpaint at guidance 5", "P2", _INP), ("P1 again", "P1", LCM),
              ("P2 at B = 1", "P2", _INP.but(B=1)), ("P1 once more", "P1", LCM)]

TC = Spec(scheduler="lcm", time_cond=True, steps=4, merge=1, guidance=3.0)
TIME_COND = [("txt2img at guidance 3", "txt2img", TC), ("guidance 8", "txt2img", TC.but(guidance=8.0)),
             ("inpaint at strength 0.75", "inpaint", TC.but(pipe="inpaint", strength=0.75)),
             ("ControlNet-inpaint with net A", "controlnet", TC.but(pipe="controlnet", nets=("A",), scales=(0.5,), windows=(FULL,))),
             ("txt2img at guidance 3 again", "txt2img", TC)]


def _other_guidance(spec):
    """the guidance_scale a single-pass / CFG generation of these scenarios is told apart from"""
    return {1.0: 2.0, 2.0: 1.0, 3.0: 8.0, 8.0: 3.0}.get(spec.guidance) if spec.scheduler == "lcm" else None


def test_lcm_one_change_at_a_time(dev):
    """single pass -> CFG path -> single pass (``kvrow`` B -> 2B -> B), then the changes that move ``z``, ``lat`` and the ring"""
    gens = [Gen(what, s, oracle=n <= 2, guidance_vs=_other_guidance(s) if n <= 2 else None, same_graphs=what == "merge 2")
            for n, (what, s) in enumerate(LCM_ONE_CHANGE)]
    pipe = pipeline_class(LCM)(new_unet(str(dev)), use_graph=True)
    outs = _run(dev, "LCM txt2img", gens, pipe)
    assert torch.equal(outs[2], outs[0]), "guidance 1 after guidance 2 is not the single pass it started with"
    assert not torch.equal(outs[1], outs[0])


def test_lcm_among_the_other_schedulers(dev):
    """DPM-Solver++ and PNDM share ``ms_row`` / ``ms_hist`` / ``ms_saved`` with LCM and run 2B rows on them; ``z`` comes (LCM: 3
    rows, DDIM eta: 4) and goes.  The three single passes are the same generation: the same bits."""
    gens = [Gen(what, s, oracle=True, guidance_vs=_other_guidance(s)) for what, s in LCM_AMONG_SCHEDULERS]
    pipe = pipeline_class(LCM)(new_unet(str(dev)), use_graph=True)
    outs = _run(dev, "LCM among the schedulers", gens, pipe)
    assert torch.equal(outs[3], outs[1]) and torch.equal(outs[7], outs[1]), "the single pass came back with other bits"
    assert pipe._engine.step_path == "multistep"


def test_sdxl_lcm_single_and_cfg(dev):
    """The pooled column and the time ids have B rows in the single pass (the conditional half's) and 2B on the CFG path; the
    fourth embed set (``null_post``) lengthens the K/V cache under a single pass that must not read it."""
    from conftest import rel_l2
    from engine_cases import fresh_eager, oracle_run, single_pass

    def rows_match(spec):
        def after(eng):
            want = spec.B if single_pass(spec) else 2 * spec.B
            assert eng._static["pooled"].shape[0] == want and eng._static["time_ids"].shape[0] == want, \
                (spec, eng._static["pooled"].shape, eng._static["time_ids"].shape)
        return after
    gens = [Gen(what, s, oracle=True, guidance_vs=_other_guidance(s), after=rows_match(s)) for what, s in SDXL_LCM]
    pipe = pipeline_class(XL_LCM)(new_unet(str(dev), "tinyxl"), use_graph=True)
    outs = _run(dev, "SDXL LCM", gens, pipe)
    assert torch.equal(outs[1], outs[0]), "the second unconditional set moved the single pass"
    # ... and matters on the CFG path.  Its values (engine_cases._inputs: the null set + 0.5 randn) move the fp32 oracle at
    # guidance 2 by rel_l2 1.0e-3 only, which no tolerance tells from rounding: that generation 2 read them is held bit for bit,
    # against a fresh eager run of the same generation without them
    g2 = SDXL_LCM[2][1]
    moved = rel_l2(oracle_run(g2, str(dev)), oracle_run(g2.but(null_post=False), str(dev)))
    print(f"[engine] SDXL LCM: the second unconditional set moves the fp32 oracle at guidance 2 by rel_l2={moved:.3e}")
    assert moved > 0.0 and not torch.equal(outs[2], fresh_eager(g2.but(null_post=False), str(dev))[0]), \
        "the second unconditional set did not reach the CFG path"


def test_shared_unet_single_pass_and_cfg(dev):
    """one HipUNet under P1 (txt2img, LCM at guidance 1: B rows) and P2 (inpaint, DDIM at guidance 5: 2B rows, then B = 1):
    the UNet's workspace and K/V buffers are sized by whoever ran last"""
    unet = new_unet(str(dev))
    pipes = {"P1": pipeline_class(LCM)(unet, use_graph=True), "P2": pipeline_class(_INP)(unet, use_graph=True)}
    gens = [Gen(what, s, oracle=True, pipe=pipes[p], guidance_vs=_other_guidance(s)) for what, p, s in SHARED_LCM]
    outs = _run(dev, "shared UNet, single pass and CFG", gens)
    assert torch.equal(outs[2], outs[0]) and torch.equal(outs[4], outs[0]), "P1 does not return to its first result"


def test_time_cond_unet_across_pipelines(dev):
    """the UNet with time_cond_proj_dim (the single pass at every guidance_scale, the scale in its time rows) under three
    pipelines: it had run txt2img only"""
    unet = new_unet(str(dev), time_cond=True)
    nets = {"A": new_net(str(dev), "A")}
    pipes = {k: pipeline_class(Spec(pipe=k))(unet, use_graph=True, **({"controlnet": nets["A"]} if k == "controlnet" else {}))
             for k in ("txt2img", "inpaint", "controlnet")}
    gens = [Gen(what, s, oracle=True, pipe=pipes[p], guidance_vs=_other_guidance(s) if n < 2 else None)
            for n, (what, p, s) in enumerate(TIME_COND)]
    outs = _run(dev, "time_cond_proj_dim UNet", gens, net_objects=nets)
    assert torch.equal(outs[4], outs[0]), "guidance 3 after three other generations is not the guidance 3 it started with"
    assert not torch.equal(outs[1], outs[0])
