"""FreeU, community LoRAs, guidance_rescale and v-prediction in combination, on one denoise engine with graphs on.  Each of the
four was tested against the base txt2img, inpaint or SDXL path only; here they meet each other, the ControlNet-inpaint
pipeline, a HipMultiControlNet with a net outside its guidance window, SDXL's second unconditional set and a UNet shared by
two pipelines.  The scenarios are lists of engine_cases.Spec run by engine_cases.run_scenario: EVERY generation must equal,
bit for bit, the same spec run eagerly on fresh objects, lie within the fp16 arm of the fp32 oracle
(conftest.check_vs_fp16_arm, defaults) -- the oracle composed of freeu_ref's hooks, vpred_ref's wrapper and schedulers and
lora_cases' merged state dicts -- and every feature a spec switches on must move the fp32 oracle by the threshold of that
feature's own tests (engine_cases.assert_features_matter), so an engine that ignored it could not pass.

The scenarios are data (``SCENARIO_A`` .. ``SCENARIO_D``, ``SCENARIO_G``, ``LARGE``, ``PAIRWISE``): tests/test_engine_features_host.py checks
without a GPU that the pairwise list covers every pair of factor values and that every spec runs enough steps.

``SCENARIO_H``, ``SCENARIO_I`` and ``PAIRWISE_LCM`` put the same switches, a 154-row context and a HipMultiControlNet under the
LCM single pass, whose UNet batch is B rows, not 2B; tests/test_lcm_engine_host.py checks those lists."""
import pytest
import torch

from conftest import check_vs_fp16_arm, dev_half
from engine_cases import (Gen, Spec, apply_features, expected_step_path, hooked_modules, new_net, new_unet, oracle_models,
                          oracle_pair, pipeline_class, run_scenario)

pytestmark = pytest.mark.gpu

FREEU = (0.9, 0.2, 1.2, 1.4)        # test_gpu_freeu.FREEU (tests/test_engine_features_host.py holds the two equal)
PHI = 0.7
LORA = ((11, 1.0),)                 # lora_cases.unet_lora's default seed, as tests/test_gpu_lora.py loads it
LORA_07 = ((11, 0.7),)
FULL = (0.0, 1.0)

CN = Spec(pipe="controlnet", steps=4, merge=1, guidance=5.0)
CN_A = CN.but(nets=("A",), scales=(0.5,), windows=(FULL,))
CN_AB = CN.but(nets=("A", "B"), multi=True, scales=(0.5, 0.8), windows=(FULL, FULL))


def _chain(base, changes):
    """[(what, spec)]: ``base``, then one change after another, each on top of the one before"""
    out, s = [("base", base)], base
    for what, change in changes:
        s = s.but(**change)
        out.append((what, s))
    return out


# a. ControlNet-inpaint with net A at scale 0.5: one switch at a time, and back
SCENARIO_A = _chain(CN_A, [
    ("FreeU on", dict(freeu=FREEU)), ("guidance_rescale 0.7", dict(rescale=PHI)), ("LoRA loaded", dict(loras=LORA)),
    ("v-prediction", dict(prediction="v_prediction")), ("DPM-Solver++ 2M", dict(scheduler="dpm")), ("PNDM", dict(scheduler="pndm")),
    ("FreeU off", dict(freeu=None)), ("LoRA unloaded", dict(loras=())), ("guidance_rescale 0", dict(rescale=0.0)),
    ("epsilon DDIM", dict(prediction="epsilon", scheduler="ddim"))])

# b. [A, B] with FreeU on; 5 steps and B's window ending at 0.6: (0, 1) three times, then (0,) twice -- warm-up, then capture
# and replay -- so both active sets are captured under FreeU within the first generation and replayed in the second
_B0 = CN_AB.but(steps=5, windows=(FULL, (0.0, 0.6)), freeu=FREEU)
SCENARIO_B = [("[A, B], FreeU, B's window ends at 0.6", _B0), ("new scales", _B0.but(scales=(0.3, 0.9))),
              ("FreeU off", _B0.but(scales=(0.3, 0.9), freeu=None)),
              ("guidance_rescale 0.7, DDIM eta 1", _B0.but(scales=(0.3, 0.9), freeu=None, rescale=PHI, eta=1.0)),
              ("FreeU on again", _B0.but(scales=(0.3, 0.9), rescale=PHI, eta=1.0))]
SCENARIO_B_SAME_GRAPHS = ("new scales",)        # MultiControlNet scales are step-table values

# c. SDXL
XL = Spec(pipe="sdxl", steps=4, merge=1, guidance=7.5)
SCENARIO_C = _chain(XL, [
    ("FreeU on", dict(freeu=FREEU)), ("second unconditional set", dict(null_post=True)), ("LoRA loaded", dict(loras=LORA)),
    ("guidance_rescale 0.7, Euler", dict(rescale=PHI, scheduler="euler")),
    ("everything off", dict(freeu=None, null_post=False, loras=(), rescale=0.0, scheduler="ddim"))])

# g. the same switches under a long context (154 text rows: every cross-attention layer on csrc/xattn_long.hip, its K/V images
# packed by ops.context_kv(long=True) into buffers of another size), then down to 77 rows and up again
CN_LONG = CN_A.but(text_len=154)
SCENARIO_G = _chain(CN_LONG, [
    ("LoRA loaded", dict(loras=LORA)), ("FreeU on", dict(freeu=FREEU)), ("guidance_rescale 0.7", dict(rescale=PHI)),
    ("everything off", dict(loras=(), freeu=None, rescale=0.0)), ("77 text rows", dict(text_len=77)),
    ("154 text rows again", dict(text_len=154))])

# d. one UNet under a txt2img pipeline P1 and an inpaint pipeline P2: (what, the pipeline that generates, its spec, the
# pipeline whose enable_freeu / disable_freeu / load_lora_weights / unload_lora_weights brings the UNet there or None,
# whether the engine promises to keep its graphs)
T2I, INP = Spec(steps=4, merge=1), Spec(pipe="inpaint", steps=4, merge=1)
_FU, _FULO, _LO = dict(freeu=FREEU), dict(freeu=FREEU, loras=LORA), dict(loras=LORA)
SCENARIO_D = [
    ("P1", "P1", T2I, None, False), ("P2", "P2", INP, None, False),
    ("P1 after P2.enable_freeu", "P1", T2I.but(**_FU), "P2", False), ("P2 with FreeU", "P2", INP.but(**_FU), None, False),
    # set_lora: no address and no host-side launch argument changes, the epoch stays -- and P2's engine was not told
    ("P2 after P1.load_lora_weights", "P2", INP.but(**_FULO), "P1", True), ("P1 with FreeU and the LoRA", "P1", T2I.but(**_FULO), None, False),
    ("P1 after P2.disable_freeu", "P1", T2I.but(**_LO), "P2", False),
    ("P2 after P1.unload_lora_weights", "P2", INP, "P1", False), ("P1", "P1", T2I, None, False)]

# e. up blocks above ops.GN_SMALL_MAX_HW = 256 tokens, B = 1: the smallest sizes at which a skip tensor carries GEMM-epilogue
# GroupNorm statistics through BOTH in-place updates (the residual add, then FreeU).  Tiny SD1.5 at 72 x 64 latents: up block 0
# at 18 x 16 = 288 tokens, up block 1 at 36 x 32; tiny SDXL at 40 x 32: up block 0 at 20 x 16 = 320 tokens.
LARGE = {"ControlNet-inpaint, FreeU, plain net": CN_A.but(B=1, hw=(72, 64), freeu=FREEU),
         "ControlNet-inpaint, FreeU, [A, B]": CN_AB.but(B=1, hw=(72, 64), freeu=FREEU),
         "SDXL, FreeU and a LoRA": XL.but(B=1, hw=(40, 32), freeu=FREEU, loras=LORA)}

# f. every pair of factor values, written out: pipe x sampler in full, the four switches chosen so that each value of one
# meets each value of every other factor (tests/test_engine_features_host.py checks it).
# The multi rows with the two multistep samplers that take no doubled first step run 6 steps with B's window ending at 0.5:
# (0, 1) and (0,) three times each, a net that falls out of its window under the ring of the multistep kernel.
PIPES = {"txt2img": Spec(), "inpaint": Spec(pipe="inpaint"), "controlnet plain": CN_A, "controlnet multi": CN_AB,
         "sdxl": XL}
SAMPLERS = {"ddim": dict(scheduler="ddim"), "euler": dict(scheduler="euler"), "dpm": dict(scheduler="dpm"),
            "pndm": dict(scheduler="pndm"), "ddim eta = 1": dict(scheduler="ddim", eta=1.0)}
FACTORS = {"pipe": tuple(PIPES), "sampler": tuple(SAMPLERS), "prediction": ("epsilon", "v_prediction"), "freeu": (False, True),
           "rescale": (0.0, PHI), "loras": (False, True)}
PAIRWISE_ROWS = [
    # pipe,             sampler,        prediction,     freeu, rescale, loras
    ("txt2img",          "ddim",         "epsilon",      True,  PHI,     False),
    ("txt2img",          "euler",        "epsilon",      False, PHI,     True),
    ("txt2img",          "dpm",          "epsilon",      True,  PHI,     False),
    ("txt2img",          "pndm",         "v_prediction", False, 0.0,     False),
    ("txt2img",          "ddim eta = 1", "v_prediction", True,  0.0,     True),
    ("inpaint",          "ddim",         "v_prediction", False, PHI,     True),
    ("inpaint",          "euler",        "epsilon",      False, PHI,     True),
    ("inpaint",          "dpm",          "v_prediction", False, 0.0,     True),
    ("inpaint",          "pndm",         "v_prediction", True,  PHI,     False),
    ("inpaint",          "ddim eta = 1", "v_prediction", False, PHI,     True),
    ("controlnet plain", "ddim",         "epsilon",      True,  0.0,     False),
    ("controlnet plain", "euler",        "v_prediction", False, PHI,     True),
    ("controlnet plain", "dpm",          "epsilon",      True,  0.0,     False),
    ("controlnet plain", "pndm",         "v_prediction", False, PHI,     False),
    ("controlnet plain", "ddim eta = 1", "epsilon",      True,  PHI,     True),
    ("controlnet multi", "ddim",         "epsilon",      True,  PHI,     False),
    ("controlnet multi", "euler",        "epsilon",      False, 0.0,     False),
    ("controlnet multi", "dpm",          "v_prediction", True,  0.0,     True),
    ("controlnet multi", "pndm",         "epsilon",      False, 0.0,     True),
    ("controlnet multi", "ddim eta = 1", "epsilon",      False, 0.0,     True),
    ("sdxl",             "ddim",         "v_prediction", True,  0.0,     False),
    ("sdxl",             "euler",        "v_prediction", True,  0.0,     False),
    ("sdxl",             "dpm",          "v_prediction", True,  0.0,     True),
    ("sdxl",             "pndm",         "epsilon",      True,  PHI,     False),
    ("sdxl",             "ddim eta = 1", "v_prediction", False, PHI,     False),
]


def pairwise_spec(pipe, sampler, prediction, freeu, rescale, loras):
    s = PIPES[pipe].but(prediction=prediction, freeu=FREEU if freeu else None, rescale=rescale, loras=LORA_07 if loras else (),
                        **SAMPLERS[sampler])
    if pipe == "controlnet multi" and sampler in ("dpm", "ddim eta = 1"):
        s = s.but(steps=6, windows=(FULL, (0.0, 0.5)))
    return s


def step_path(spec):
    """the step launch the engine must report: the first-order kernel for DDIM at eta 0 and Euler, the multistep kernel for
    the others, ``+rescale`` where guidance_rescale is honoured; ``multistep`` for the LCM single pass
    (engine_cases.expected_step_path, which run_scenario holds every generation to)"""
    return expected_step_path(spec)


PAIRWISE = {f"{r[0]}, {r[1]}, {r[2]}{', FreeU' if r[3] else ''}{', rescale' if r[4] else ''}{', LoRA' if r[5] else ''}": pairwise_spec(*r)
            for r in PAIRWISE_ROWS}
# zero-SNR betas with trailing spacing start at alphas_cumprod = 0, which only a v-prediction can step from
ZERO_SNR_SPEC = Spec(zero_snr=True, prediction="v_prediction", rescale=PHI, freeu=FREEU, loras=LORA_07)
PAIRWISE["zero-SNR DDIM, v_prediction, FreeU, rescale, LoRA"] = ZERO_SNR_SPEC


# h. the LCM single pass (LCMScheduler at guidance_scale 1: the UNet runs the B conditional rows) under the
# switches that were written while the UNet batch was always 2B.  guidance_rescale is inert there: the same bits as the
# generation before, the step launch stays "multistep", cid_cfg_rescale_f16 is never launched.
LCM1 = Spec(scheduler="lcm", steps=4, merge=1, guidance=1.0)
SCENARIO_H = _chain(LCM1, [
    ("LoRA loaded", dict(loras=LORA)), ("FreeU on", dict(freeu=FREEU)), ("guidance_rescale 0.7 (inert)", dict(rescale=PHI)),
    ("everything off", dict(loras=(), freeu=None, rescale=0.0)), ("154 text rows", dict(text_len=154)),
    ("154 text rows, LoRA and FreeU", dict(loras=LORA, freeu=FREEU)), ("77 text rows", dict(text_len=77))])

# i. the single pass with a HipMultiControlNet [A, B]: 4 steps with B's window ending at 0.5 are (0, 1) twice, then (0,) twice
# -- warm-up and capture of both sets within the generation; at strength 0.75 (3 executed steps) (0, 1) once and (0,) twice
_I0 = CN_AB.but(scheduler="lcm", guidance=1.0)
_I1 = _I0.but(windows=(FULL, (0.0, 0.5)))
SCENARIO_I = _chain(_I0, [
    ("B's window ends at 0.5", dict(windows=_I1.windows)), ("new scales", dict(scales=(0.3, 0.9))), ("FreeU on", dict(freeu=FREEU)),
    ("strength 0.75", dict(strength=0.75)), ("guidance 2: the CFG path", dict(guidance=2.0)), ("guidance 1", dict(guidance=1.0))])
SCENARIO_I_SAME_GRAPHS = ("new scales",)        # the multi path reads its scales from the step table

# j. pairs of generations on one new pipeline
XL_LCM1 = XL.but(scheduler="lcm", guidance=1.0)
PAIRWISE_LCM = {"txt2img, LCM at guidance 1, then with a LoRA": (LCM1, LCM1.but(loras=LORA_07)),
                "sdxl, LCM with FreeU, guidance 1 then 2": (XL_LCM1.but(freeu=FREEU), XL_LCM1.but(freeu=FREEU, guidance=2.0))}


def lcm_specs():
    """{label: spec} of every generation of (h) - (j)"""
    out = {}
    for name, rows in (("h", SCENARIO_H), ("i", SCENARIO_I)):
        out.update({f"{name}: {n} {what}": s for n, (what, s) in enumerate(rows)})
    out.update({f"j: {k}, generation {n}": s for k, pair in PAIRWISE_LCM.items() for n, s in enumerate(pair)})
    return out


def all_specs():
    """{label: spec} of every generation of (a) - (g)"""
    out = {}
    for name, rows in (("a", SCENARIO_A), ("b", SCENARIO_B), ("c", SCENARIO_C), ("g", SCENARIO_G)):
        out.update({f"{name}: {n} {what}": s for n, (what, s) in enumerate(rows)})
    out.update({f"d: {n} {row[0]}": row[2] for n, row in enumerate(SCENARIO_D)})
    out.update({f"e: {k}": s for k, s in LARGE.items()})
    out.update({f"f: {k}": s for k, s in PAIRWISE.items()})
    return out


def _pipe(dev, spec, nets=None, unet=None):
    kw = {}
    if spec.pipe == "controlnet":
        kw["controlnet"] = [nets[k] for k in spec.nets] if spec.multi else nets[spec.nets[0]]
    return pipeline_class(spec)(unet or new_unet(str(dev), spec.name, keep_base=True), use_graph=True, **kw)


def _nets(dev, spec):
    return {k: new_net(str(dev), k) for k in spec.nets}


# --------------------------------------------------------------------------- a - c: one pipeline, one switch at a time
def test_controlnet_inpaint_one_switch_at_a_time(dev):
    nets = _nets(dev, CN_A)
    pipe = _pipe(dev, CN_A, nets)
    outs = run_scenario(dev, "features on ControlNet-inpaint", [Gen(what, s, oracle=True) for what, s in SCENARIO_A], pipe, nets)
    assert torch.equal(outs[-1], outs[0]), "ten switches on and off again, and the first generation does not come back"
    assert pipe._engine.step_path == "cfg_ddim" and "seed11" not in pipe.get_list_adapters() and pipe.unet._freeu is None


def test_multicontrolnet_with_freeu_and_a_net_outside_its_window(dev):
    nets = _nets(dev, CN_AB)
    pipe = _pipe(dev, CN_AB, nets)
    gens = [Gen(what, s, oracle=True, same_graphs=what in SCENARIO_B_SAME_GRAPHS) for what, s in SCENARIO_B]
    run_scenario(dev, "features on a MultiControlNet", gens, pipe, nets)
    assert {(0, 1), (0,)} <= set(pipe._engine.captures), pipe._engine.captures
    assert pipe._engine.step_path == "cfg_multistep+rescale"


def test_sdxl_one_switch_at_a_time(dev):
    pipe = _pipe(dev, XL)
    outs = run_scenario(dev, "features on SDXL", [Gen(what, s, oracle=True) for what, s in SCENARIO_C], pipe)
    assert torch.equal(outs[-1], outs[0]), "everything off again, and the first generation does not come back"


# --------------------------------------------------------------------------- g: a long context under the switches
def test_long_context_one_switch_at_a_time(dev):
    """base -> LoRA -> FreeU -> guidance_rescale -> all off -> 77 text rows -> 154 again, graphs on.  A LoRA changes the K/V
    projections: the long K/V images must be packed anew from the merged weights (every generation is held to a fresh eager
    run of its spec and to the oracle with the LoRA merged), in the long layout, into the same buffers."""
    from test_gpu_long_context import _long_layers
    nets = _nets(dev, CN_LONG)
    pipe = _pipe(dev, CN_LONG, nets)
    layer = next(iter(pipe.unet.packed.xattn_layers))
    seen = {}

    def look(what):
        def before():           # the state the generation BEFORE this one left behind
            ctx = pipe.unet._ctx
            seen[what] = (ctx.kp[layer].clone(), ctx.kp[layer].data_ptr(), ctx.n_txt, list(_long_layers(pipe.unet)),
                          [list(_long_layers(n)) for n in nets.values()])
        return before
    gens = [Gen(what, s, oracle=True) for what, s in SCENARIO_G]
    gens[1].before, gens[2].before, gens[5].before = look("base"), look("LoRA"), look("all off")
    outs = run_scenario(dev, "features under a long context", gens, pipe, nets)
    assert torch.equal(outs[-1], outs[0]), "154 text rows again, and the first generation does not come back"
    assert torch.equal(outs[4], outs[0]), "everything off again, and the first generation does not come back"
    assert not torch.equal(outs[1], outs[0]) and not torch.equal(outs[5], outs[0])
    for what in ("base", "LoRA", "all off"):
        kp, ptr, n_txt, layers, net_layers = seen[what]
        assert n_txt == 154 and layers and all(layers), f"after {what}: a layer is not packed for the long-context kernel"
        assert all(l and all(l) for l in net_layers), f"after {what}: a ControlNet layer is not packed for the long-context kernel"
    assert seen["LoRA"][0].shape == seen["base"][0].shape and seen["LoRA"][1] == seen["base"][1], "the K image moved under a LoRA"
    assert not torch.equal(seen["LoRA"][0], seen["base"][0]), "the long K image did not follow the LoRA's to_k"
    assert torch.equal(seen["all off"][0], seen["base"][0]), "the long K image of the base did not come back after the unload"
    assert all(_long_layers(pipe.unet)) and pipe.unet._ctx.n_txt == 154 and "seed11" not in pipe.get_list_adapters()


# --------------------------------------------------------------------------- h - j: the LCM single pass
def _guidance_vs(spec):
    return {1.0: 2.0, 2.0: 1.0}[spec.guidance]


def test_lcm_single_pass_one_switch_at_a_time(dev, monkeypatch):
    from consistentid_amd import ops
    launches = []
    rescale = ops.cfg_rescale
    monkeypatch.setattr(ops, "cfg_rescale", lambda *a, **k: (launches.append(1), rescale(*a, **k))[1])
    pipe = _pipe(dev, LCM1)
    gens = [Gen(what, s, oracle=True, guidance_vs=2.0 if n == 0 else None) for n, (what, s) in enumerate(SCENARIO_H)]
    outs = run_scenario(dev, "features on the LCM single pass", gens, pipe)
    assert torch.equal(outs[3], outs[2]), "guidance_rescale moved the single pass"
    assert not launches and "escale" not in pipe._engine._static, "cid_cfg_rescale_f16 was launched in a single pass"
    assert torch.equal(outs[4], outs[0]), "everything off again, and the first generation does not come back"
    assert not torch.equal(outs[1], outs[0]) and not torch.equal(outs[2], outs[1]) and not torch.equal(outs[5], outs[0])
    assert pipe.unet._ctx.n_txt == 77 and pipe.unet._freeu == FREEU and "seed11" in pipe.get_list_adapters()


def test_lcm_single_pass_multicontrolnet(dev):
    nets = _nets(dev, _I0)
    pipe = _pipe(dev, _I0, nets)
    gens = [Gen(what, s, oracle=True, same_graphs=what in SCENARIO_I_SAME_GRAPHS,
                guidance_vs=_guidance_vs(s) if n in (0, 5, 6) else None) for n, (what, s) in enumerate(SCENARIO_I)]
    seen = []
    gens[2].before = lambda: seen.append(list(pipe._engine.captures))
    outs = run_scenario(dev, "MultiControlNet on the LCM single pass", gens, pipe, nets)
    assert seen[0][-2:] == [(0, 1), (0,)], f"B fell out of its window and the graphs did not gain (0,): {seen[0]}"
    assert not torch.equal(outs[2], outs[1]), "the new scales did not reach the replayed step"
    assert pipe._engine.step_path == "multistep"


@pytest.mark.parametrize("case", list(PAIRWISE_LCM))
def test_pairwise_lcm(dev, case):
    """two differing generations on one new pipeline: warm-up and capture in the first; the second follows a switch"""
    first, second = PAIRWISE_LCM[case]
    pipe = _pipe(dev, first)
    vs = lambda s: _guidance_vs(s) if first.guidance != second.guidance or not s.loras else None
    gens = [Gen("the first of the pair", first, oracle=True, guidance_vs=vs(first)),
            Gen("the second of the pair", second, oracle=True, guidance_vs=vs(second))]
    a, b = run_scenario(dev, case, gens, pipe)
    assert pipe._engine.captures and not torch.equal(a, b)
    assert pipe._engine.step_path == step_path(second)


# --------------------------------------------------------------------------- d: a shared UNet
def test_shared_unet_sees_the_other_pipelines_switches(dev):
    """as in diffusers, where the UNet holds both: FreeU enabled or a LoRA loaded through one pipeline shows in the other"""
    unet = new_unet(str(dev), keep_base=True)
    pipes = {"P1": _pipe(dev, T2I, unet=unet), "P2": _pipe(dev, INP, unet=unet)}
    p1_captures = []            # of P1's engine, before every generation

    def switch(via, spec):
        def before():
            p1_captures.append(len(pipes["P1"]._engine.captures))
            assert via is None or apply_features(pipes[via], spec), "the switch was a no-op"
        return before
    gens = [Gen(what, spec, oracle=True, same_graphs=same, pipe=pipes[p], before=switch(via, spec))
            for what, p, spec, via, same in SCENARIO_D]
    outs = run_scenario(dev, "features on a shared UNet", gens)
    assert torch.equal(outs[-1], outs[0]), "P1 does not return to its first result"
    assert torch.equal(outs[-2], outs[1]), "P2 does not return to its first result"
    assert not torch.equal(outs[2], outs[0]), "P2.enable_freeu did not show in P1"
    assert not torch.equal(outs[4], outs[3]), "P1.load_lora_weights did not show in P2"
    # P2's enable_freeu reached P1's engine through the shared UNet's epoch: P1 captured again for its next generation
    assert p1_captures[3] > p1_captures[2] >= 1, f"P1 did not re-capture after P2.enable_freeu: {p1_captures}"


# --------------------------------------------------------------------------- e: statistics through both in-place updates
@pytest.mark.parametrize("case", list(LARGE))
def test_up_blocks_above_256_tokens(dev, case):
    from consistentid_amd import ops
    spec = LARGE[case]
    down = 2 if spec.pipe == "sdxl" else 4          # up block 0 sits below two (tiny SDXL: one) downsamplers
    assert spec.B == 1 and spec.hw[0] * spec.hw[1] <= 72 * 64 and (spec.hw[0] // down) * (spec.hw[1] // down) > ops.GN_SMALL_MAX_HW
    nets = _nets(dev, spec)
    run_scenario(dev, case, [Gen("the one generation", spec, oracle=True)], _pipe(dev, spec, nets), nets)


# --------------------------------------------------------------------------- f: every pair of factor values
@pytest.mark.parametrize("case", list(PAIRWISE))
def test_pairwise(dev, case):
    """two generations on one new pipeline: warm-up and capture in the first, the second replays only"""
    spec = PAIRWISE[case]
    nets = _nets(dev, spec)
    pipe = _pipe(dev, spec, nets)
    gens = [Gen("warm-up and capture", spec, oracle=True), Gen("replay", spec, oracle=True, same_graphs=True)]
    a, b = run_scenario(dev, case, gens, pipe, nets)
    assert pipe._engine.captures and torch.equal(a, b)
    assert pipe._engine.step_path == step_path(spec)


# --------------------------------------------------------------------------- GroupNorm after the in-place updates
# The tiny models never attach GEMM-epilogue GroupNorm statistics (``_gn_stats``): only the 160-wide tiles emit them, unsplit,
# i.e. at widths that are multiples of 160 (``cid_gemm_stats_rows``; tests/test_engine_features_host.py asserts it for every
# launch shape of (e)).  What (e) cannot reach is composed here from the launches themselves at the smallest shape that can:
# two 1 x 1 GEMMs at 320 channels and 20 x 16 = 320 tokens write ``x`` and ``skip`` WITH statistics, then the updates
# ``forward_tokens`` makes in place run in its order, then the resnet's GroupNorm over [x | skip] -- against float64 on the
# updated tensors.  Statistics that survive an update describe the tensor before it, and the GroupNorm would apply them.
STATS_SHAPE = dict(B=2, H=20, W=16, C=320)
UPDATES = {"FreeU": ("freeu",), "residual add (plain net)": ("add",), "residuals of [A, B], B outside its window": ("accum",),
           "residual add, then FreeU": ("add", "freeu"), "residuals of [A, B], then FreeU": ("accum", "freeu"),
           "mid residual on x, FreeU off": ("add_x",)}


@pytest.mark.parametrize("case", list(UPDATES))
def test_groupnorm_after_in_place_updates_of_tensors_with_statistics(dev, case):
    import torch.nn.functional as Fn
    from conftest import check_close
    from consistentid_amd import ops
    from freeu_ref import fourier_filter
    B, H, W, C = (STATS_SHAPE[k] for k in "BHWC")
    HW, M = H * W, B * H * W
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half()
    ws = torch.empty(ops.GEMM_WS_BYTES, dtype=torch.uint8, device=dev)
    made = []
    for _ in range(2):      # x, then skip: a 1 x 1 convolution with bias and residual, every group's mean well off zero
        a, w, bias, res = rnd(M, C), rnd(C, C, scale=C ** -0.5), (1.0 + rnd(C).float()).half(), rnd(M, C)
        out = torch.empty(M, C, dtype=torch.float16, device=dev)
        ops.gemm(a.to(dev), w.to(dev), out, M=M, N=C, c1=C, bias=bias.to(dev), res=res.to(dev), ldr=C, ws=ws, gn_hw=HW)
        assert hasattr(out, "_gn_stats"), "this launch was expected to emit statistics: the test would be vacuous"
        made.append(out)
    x, skip = made
    x0, s0 = x.double().cpu(), skip.double().cpu()
    r = [rnd(M // 2, C).to(dev) for _ in range(2)]          # B-row residuals under the 2B-row batch, as in the loop
    want_x, want_s = x0, s0
    for step in UPDATES[case]:
        if step == "add":
            ops.add_inplace(skip, r[0])
            want_s = want_s + torch.cat([r[0].double().cpu()] * 2)
        elif step == "add_x":
            ops.add_inplace(x, r[0])
            want_x = want_x + torch.cat([r[0].double().cpu()] * 2)
        elif step == "accum":       # net 1 did not run: None, and a scale of exactly 0
            ops.residual_accum([skip], [[r[0]], None], torch.tensor([0.5, 0.0, 0.0, 0.0], device=dev))
            want_s = want_s + 0.5 * torch.cat([r[0].double().cpu()] * 2)
        else:
            fws = torch.zeros(ops.freeu_ws_bytes(B, C, H, W), dtype=torch.uint8, device=dev)
            ops.freeu(x, skip, fws, B=B, H=H, W=W, c_x=C, c_skip=C, s=FREEU[1], b=FREEU[3])
            want_x = torch.cat([want_x[:, :C // 2] * FREEU[3], want_x[:, C // 2:]], dim=1)
            want_s = fourier_filter(want_s.view(B, H, W, C).permute(0, 3, 1, 2), 1, FREEU[1]).permute(0, 2, 3, 1).reshape(M, C)
    torch.cuda.synchronize()
    check_close(x, want_x, f"{case}: x after the updates")
    check_close(skip, want_s, f"{case}: skip after the updates (residuals first, FreeU on the sum)")
    gm, bt = (1 + 0.1 * rnd(2 * C).float()).half(), rnd(2 * C, scale=0.1)
    cat = torch.cat([x.double().cpu(), skip.double().cpu()], dim=1).view(B, HW, 2 * C)
    moved = torch.cat([x0, s0], dim=1).view(B, HW, 2 * C)
    gn = lambda t: Fn.silu(Fn.group_norm(t.transpose(1, 2), 32, gm.double(), bt.double(), 1e-5)).transpose(1, 2)
    ref = gn(cat)
    from conftest import TOL_L2, rel_l2
    assert rel_l2(gn(moved), ref) >= 20 * TOL_L2, "the GroupNorm of the tensors before the updates is too close to tell"
    y = torch.empty(M, 2 * C, dtype=torch.float16, device=dev)
    gws = torch.zeros(ops.groupnorm_ws_bytes(B, 2 * C), dtype=torch.uint8, device=dev)
    ops.groupnorm(x, y, gm.to(dev), bt.to(dev), gws, B=B, HW=HW, c1=C, x2=skip, c2=C, groups=32, eps=1e-5, silu=True)
    torch.cuda.synchronize()
    check_close(y.view(B, HW, 2 * C), ref, f"{case}: GroupNorm over [x | skip] after the updates")


# --------------------------------------------------------------------------- the K/V cache of the diffusers-style call
@pytest.mark.parametrize("name", ["tiny", "tinyxl"])
def test_cached_context_does_not_outlive_a_lora(dev, name):
    """``HipUNet.__call__`` keeps the packed cross-attention K/V while it is handed the very same embeddings tensor (the
    engine's loop does not: it projects them anew every generation).  A LoRA changes to_k / to_v, so the call after
    ``load_lora_weights`` -- same tensor object, FreeU on -- must project again: held to the oracle with the LoRA merged and
    FreeU hooked in, and after the unload to the bits of the first call."""
    import lora_cases as L
    from freeu_ref import install_freeu
    spec = (XL if name == "tinyxl" else T2I).but(freeu=FREEU, loras=LORA_07)
    pipe = _pipe(dev, spec)
    lat, t, ehs, kw = L.forward_inputs(name)
    lat, ehs, kw = lat.to(dev), ehs.to(dev), {k: {a: b.to(dev) for a, b in v.items()} for k, v in kw.items()}     # made once
    call = lambda: pipe.unet(lat, t, encoder_hidden_states=ehs, cross_attention_kwargs={}, **kw).sample.clone()
    apply_features(pipe, spec.but(loras=()))
    first = call()
    apply_features(pipe, spec)
    got = call()
    refs = []
    for model, f in zip(oracle_models(str(dev), name, 0, spec.loras), (lambda x: x.float(), lambda x: dev_half(x, dev))):
        handles = install_freeu(model, *FREEU)
        try:
            refs.append(L.oracle_forward(model, name, f))
        finally:
            for h in handles:
                h.remove()
    base = oracle_models(str(dev), name)[0]
    handles = install_freeu(base, *FREEU)
    try:
        L.assert_matters(refs[0], L.oracle_forward(base, name, lambda x: x.float()), f"{name} forward with FreeU, LoRA x 0.7")
    finally:
        for h in handles:
            h.remove()
    check_vs_fp16_arm(got, *refs, f"{name} UNet forward on cached embeddings after load_lora_weights, FreeU on")
    apply_features(pipe, spec.but(loras=()))
    assert torch.equal(call(), first), "the call after unload_lora_weights is not the call before the load"


# --------------------------------------------------------------------------- the memoised oracles stay as they were
@pytest.mark.parametrize("name", ["tiny", "tinyxl"])
def test_memoised_oracles_are_unchanged_after_freeu_specs(dev, name):
    """engine_cases.oracle_run hooks FreeU into the memoised fp32 oracle and fp16 arm for one call; afterwards no hook is
    left and a forward gives what it gave before: the fp32 oracle on the CPU bit for bit; the arm, whose stock fp16 kernels
    do not repeat their bits from call to call (measured: rel_l2 3.6e-3 between two calls, its distance to the oracle), as
    close to the fp32 oracle as it was -- FreeU left in would move it by more than 0.1"""
    import lora_cases as L
    o, arm = oracle_models(str(dev), name)
    run = lambda: (L.oracle_forward(o, name, lambda t: t.float()),
                   L.oracle_forward(arm, name, lambda t: t.to(dev).half() if t.is_floating_point() else t.to(dev)))
    before = run()
    spec = (XL if name == "tinyxl" else CN_A).but(freeu=FREEU)
    plain = oracle_pair(spec.but(freeu=None), str(dev))
    with_freeu = oracle_pair(spec, str(dev))
    assert not torch.equal(with_freeu[0], plain[0]) and not torch.equal(with_freeu[1], plain[1])
    assert not hooked_modules(o, arm), "oracle_run left FreeU hooks on a memoised oracle"
    after = run()
    assert torch.equal(after[0], before[0])
    check_vs_fp16_arm(after[1], before[0], before[1], f"{name} fp16 arm after a FreeU spec, judged like an engine against the arm before")
