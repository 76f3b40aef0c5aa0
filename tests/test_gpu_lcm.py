"""Few-step sampling on the GPU: cid_multistep_step_f16 (the single pass) against its CFG sibling and the float64 model of the
row contract, the launch replayed from a hipGraph behind cid_step_select, LCMScheduler trajectories of the four pipelines
on the tiny models against ``oracle.loop.denoise`` driven by tests/lcm_ref.py, and a tiny UNet with ``time_cond_proj_dim``."""
import numpy as np
import pytest
import torch

import engine_cases as E
from conftest import TOL_L2, check_close, check_vs_fp16_arm, dev_half, rel_l2
from engine_cases import set_guidance as _set_guidance, time_cond_models as _cond_models
from lcm_ref import CondOnly, LCMLoopRef
from multistep_ref import RowEmulator

pytestmark = pytest.mark.gpu

NAN = float("nan")
BIG = 8 * 262403      # 262403 threads' worth of 8 halfs (4.2 MB): past grid_for's cap of 1024 blocks x 256 threads x 8, and ragged


def _row(a=0.0, b=1.0, c_x=0.0, c_m=0.0, c_hist=(0.0, 0.0, 0.0, 0.0), c_z=0.0, c_init=1.0, c_noise=0.0, w=-1, flags=0, z_row=0):
    """one multistep row as include/cid.h lays it out (word 8: the model-input scale, unused by the kernel)"""
    return [a, b, c_x, c_m, *c_hist, 1.0, c_init, c_noise, c_z, float(w), float(flags), float(z_row), 0.0]


# in turn: a ring write with a save; two ring writes that weigh one and two earlier slots; a restore with all four slots (one
# unwritten, coefficient 0) and noise from the LAST row of z; everything together with the inpaint blend's coefficients
KERNEL_ROWS = [
    _row(a=0.3, b=0.9, c_x=0.8, c_m=-0.4, w=0, flags=1),
    _row(a=-0.2, b=1.1, c_x=1.05, c_m=0.5, c_hist=(-0.3, 0, 0, 0), w=1),
    _row(a=0.0, b=1.0, c_x=0.9, c_m=0.6, c_hist=(0.2, -0.5, 0, 0), w=2),
    _row(a=0.5, b=0.5, c_x=0.95, c_m=0.4, c_hist=(0.3, -0.35, 0.2, 0), c_z=0.6, flags=2, z_row=2),
    _row(a=1.2, b=-0.7, c_x=0.7, c_m=0.3, c_hist=(0.1, 0.25, -0.45, 0), c_z=-0.3, c_init=0.8, c_noise=0.6, w=3, flags=3, z_row=2),
    _row(a=0.1, b=1.0, c_x=1.0, c_m=-0.5, c_hist=(0.45, -0.2, 0.3, -0.25), c_init=0.8, c_noise=0.6, w=0),
]


def _device_row(row, dev):
    from consistentid_amd.scheduler import pack_step_rows
    return torch.from_numpy(pack_step_rows(np.asarray([row]))[0]).to(dev).view(torch.float32)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
@pytest.mark.parametrize("B,per", [(1, 8), (3, 320), (1, BIG)], ids=["one-item", "3x320", "past-the-grid-cap"])
def test_single_pass_kernel_is_the_cfg_kernel_on_equal_halves(dev, B, per, inpaint):
    """Six launches on two sets of buffers: ``multistep_step(eps)`` and ``cfg_multistep_step(cat([eps, eps]), 7.5)`` -- u + g (u -
    u) is exactly u, so latents, ring and ``saved`` agree bit for bit after every launch -- and both against the float64
    model of the row contract (check_close defaults per launch, the ring fp32 against float64 at 1e-6, ``saved`` a bit
    copy, as test_multistep_kernel_matches_the_row_contract).  ``eps`` is a tensor of exactly B * per_sample elements; the ring,
    ``saved`` and noise rows 0 and 1 start as NaN, so whatever a zero coefficient covers must not be read."""
    from consistentid_amd import ops
    n = B * per
    g = torch.Generator().manual_seed(n % 1000 + inpaint)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    lat0 = rnd(n)
    z = torch.full((3, n), NAN, dtype=torch.float16)
    z[2] = rnd(n)
    blend_h, blend_e = {}, ()
    if inpaint:
        mask, init, noise = (torch.rand(n, generator=g) > 0.5).half(), rnd(n), rnd(n)
        blend_h = dict(mask=mask.to(dev), init=init.to(dev), noise=noise.to(dev))
        blend_e = tuple(t.double().numpy() for t in (mask, init, noise))
    state = lambda: (lat0.to(dev), torch.full((4, n), NAN, device=dev), torch.full((n,), NAN, dtype=torch.float16, device=dev))
    (lat, hist, saved), (lat2, hist2, saved2) = state(), state()
    emu, zd = RowEmulator(n, z=z.double().numpy()), z.to(dev)
    for k, row in enumerate(KERNEL_ROWS):
        eps = rnd(n)
        x_in = lat.cpu().double().numpy()
        want = emu.step(row, x_in, eps.double().numpy(), eps.double().numpy(), 1.0, *blend_e)
        eps_d = eps.to(dev)
        assert eps_d.numel() == n
        ops.multistep_step(eps_d, lat, hist, saved, _device_row(row, dev), B=B, per_sample=per, z=zd, **blend_h)
        ops.cfg_multistep_step(torch.cat([eps, eps]).to(dev), lat2, hist2, saved2, _device_row(row, dev), 7.5, B=B,
                               per_sample=per, z=zd, **blend_h)
        torch.cuda.synchronize()
        for a, b, what in ((lat, lat2, "latents"), (hist, hist2, "ring"), (saved, saved2, "saved")):
            assert _same_bits(a, b), f"row {k}: {what} differ from the CFG entry on equal halves"
        check_close(lat, torch.from_numpy(want), f"single-pass kernel B={B} per_sample={per} inpaint={inpaint} row {k}")
        if k == 0:
            assert torch.equal(saved.cpu().double(), torch.from_numpy(x_in)), "saved is not a copy of the incoming sample"
    assert torch.isfinite(hist).all()
    check_close(hist, torch.from_numpy(emu.hist), f"single-pass ring n={n}", tol_l2=1e-6, tol_max=1e-6)   # fp32 vs float64
    assert torch.equal(saved.cpu().double(), torch.from_numpy(emu.saved))


def test_single_pass_launch_replays_from_a_graph(dev):
    """One captured launch behind cid_step_select over a 4-row table whose rows change slot, flags and noise row (the model
    output of each step is a table column too): bit-identical to four eager launches, and right against the emulator."""
    from consistentid_amd import ops
    from consistentid_amd.scheduler import pack_step_rows
    n, B = 3 * 1024, 3
    g = torch.Generator().manual_seed(22)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    rows = [KERNEL_ROWS[0], KERNEL_ROWS[1], _row(a=0.5, b=0.5, c_x=0.95, c_m=0.4, c_hist=(0.3, -0.35, 0, 0), c_z=0.6, flags=2, z_row=1),
            _row(a=0.1, b=1.0, c_x=1.0, c_m=-0.5, c_hist=(0.45, -0.2, 0, 0), c_z=-0.3, w=0, z_row=2)]
    eps_all, lat0, z = rnd(4, n), rnd(n), rnd(3, n)
    emu, x = RowEmulator(n, z=z.double().numpy()), lat0.double().numpy()
    for k, row in enumerate(rows):
        x = emu.step(row, x, eps_all[k].double().numpy(), eps_all[k].double().numpy(), 1.0)
        x = x.astype(np.float16).astype(np.float64)            # the kernel's one rounding, at the store of the latents
    row_buf = torch.zeros(16, dtype=torch.int32, device=dev)
    eps_buf = torch.zeros(n, dtype=torch.float16, device=dev)
    tab = ops.StepTable([(row_buf, torch.from_numpy(pack_step_rows(np.asarray(rows)))), (eps_buf, eps_all)], dev)
    lat, hist = lat0.to(dev), torch.full((4, n), NAN, device=dev)
    saved, zd = torch.full((n,), NAN, dtype=torch.float16, device=dev), z.to(dev)

    def launch():
        tab.select()
        ops.multistep_step(eps_buf, lat, hist, saved, row_buf.view(torch.float32), B=B, per_sample=n // B, z=zd)

    def start():
        lat.copy_(lat0)
        hist.fill_(NAN)
        saved.fill_(NAN)
        tab.reset(0)
    for _ in range(4):
        launch()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (lat, hist, saved)]
    check_close(lat, torch.from_numpy(x), "four eager single-pass launches")
    start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    start()
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    for got, want, what in zip((lat, hist, saved), eager, ("latents", "ring", "saved")):
        assert _same_bits(got, want), f"graph replay differs from eager launches: {what}"
    check_close(lat, torch.from_numpy(x), "four replayed single-pass launches")


# ----------------------------------------------------------------------------------------------------------- trajectories
STEPS, MERGE = 4, 1
_REFS = {}


def _spec(kind, guidance, strength=1.0):
    nets = dict(nets=("A",), scales=(0.8,), windows=((0.0, 1.0),)) if kind == "controlnet" else {}
    return E.Spec(pipe=kind, steps=STEPS, guidance=guidance, merge=MERGE, strength=strength, **nets)


def _noises(spec, dev):
    """the executed steps' noise but the last one's, [n_run - 1, B, 4, h, w] fp16"""
    return E.inputs(spec, str(dev))["variance_noise"][:E.executed_steps(spec) - 1]


def _oracle_pair(spec, dev, unets=None, single=None):
    """(fp32 oracle latents, fp16-arm latents): ``oracle.loop.denoise`` stepping with LCMLoopRef, on the conditional rows only
    where the engine takes the single pass; computed once per spec"""
    key = (spec, id(unets))
    if key in _REFS:
        return _REFS[key]
    from oracle import loop
    M = E.models(str(dev))
    inp, single = E.inputs(spec, str(dev)), spec.guidance <= 1.0 if single is None else single
    out = []
    for arm in (False, True):
        unet = (unets or E.oracle_models(str(dev), spec.name))[int(arm)]
        f = (lambda t: dev_half(t, dev)) if arm else (lambda t: t.float())
        kw = dict(num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge)
        if spec.pipe in ("inpaint", "controlnet"):
            kw.update(inpaint_mask=f(inp["mask"]), inpaint_init=f(inp["init"]), inpaint_noise=f(inp["noise"]), strength=spec.strength)
        if spec.pipe == "sdxl":
            kw.update(add_text_embeds_null=f(inp["pooled_null"]), add_text_embeds_text=f(inp["pooled_text"]),
                      add_text_embeds_aug=f(inp["pooled_augmented"]), add_time_ids=f(inp["time_ids"]))
        if spec.nets:
            net = M["a_cns" if arm else "o_cns"][list(E.NET_SEEDS).index(spec.nets[0])]
            kw.update(controlnet=net, control_image=f(inp["imgs"][spec.nets[0]]), conditioning_scale=spec.scales[0])
        sch = LCMLoopRef(list(_noises(spec, dev).float()))
        out.append(loop.denoise(CondOnly(unet) if single else unet, sch, f(inp["latents"]), f(inp["null"]), f(inp["augmented"]),
                                f(inp["text"]), **kw))
    _REFS[key] = tuple(out)
    return _REFS[key]


class _WithNoise:
    """``pipe(**kw)`` of engine_cases.call_pipeline with LCM's noise (or a generator) added to the call"""

    def __init__(self, pipe, **extra):
        self.pipe, self.extra = pipe, extra

    def __call__(self, **kw):
        return self.pipe(**kw, **self.extra)


def _pipeline(dev, spec, use_graph, unet=None):
    from consistentid_amd import scheduler
    kw = {"controlnet": E.new_net(str(dev), spec.nets[0])} if spec.pipe == "controlnet" else {}
    return E.pipeline_class(spec)(unet or E.new_unet(str(dev), spec.name), scheduler=scheduler.LCMScheduler(), use_graph=use_graph, **kw)


def _run_twice(dev, spec, use_graph, what, path, rows):
    """two generations on one pipeline -- with graphs the second replays what the first captured -- each held to the fp16 arm
    like every trajectory here; the step launch and the UNet's batch rows (the K/V row selector's length) as expected"""
    pipe = _pipeline(dev, spec, use_graph)
    ref, arm = _oracle_pair(spec, dev)
    outs = []
    for gen in range(2):
        out, _ = E.call_pipeline(_WithNoise(pipe, variance_noise=_noises(spec, dev).to(dev)), spec, dev)
        eng = pipe._engine
        assert eng.step_path == path and tuple(eng._static["kvrow"].shape) == (rows,)
        check_vs_fp16_arm(out, ref, arm, f"{what}, graph={use_graph}, generation {gen}")
        outs.append(out.clone())
    assert torch.equal(*outs) and bool(pipe._engine.captures) == use_graph
    return pipe, outs[0]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_tiny_lcm_single_pass_trajectory(dev, use_graph):
    """4-step LCM at guidance_scale 1.0 on the tiny SD1.5 pipeline: the UNet runs B = 2 rows, the step is cid_multistep_step_f16;
    against LCMRef driving the fp32 oracle UNet on the conditional rows only, within max(1e-3, 1.5 x the torch-fp16 arm) like
    test_tiny_multistep_trajectory.  Measured on the MI355X, eager and graph alike (both generations the same bits):
    rel_l2 7.2e-4 / max_rel 1.1e-3 against the arm's 1.5e-3 / 1.8e-3, so the bounds were 2.3e-3 / 4.0e-3.  The other
    trajectories of this file: guidance 2 (CFG path) 1.3e-3 / 1.3e-3 (arm 2.7e-3 / 3.4e-3), inpaint at strength 0.75
    6.5e-4 / 7.7e-4 (arm 1.4e-3 / 1.6e-3), tinyxl 7.0e-4 / 9.0e-4 (arm 1.4e-3 / 2.1e-3), one ControlNet 7.0e-4 / 1.1e-3
    (arm 1.4e-3 / 1.8e-3), time_cond_proj_dim at guidance 3 and 8 7.0e-4 / 8.8e-4 (arm 1.5e-3 / 1.8e-3)."""
    spec = _spec("txt2img", 1.0)
    _run_twice(dev, spec, use_graph, "tiny LCM 4-step single pass", "multistep", spec.B)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_tiny_lcm_with_guidance_takes_the_cfg_path(dev, use_graph):
    """guidance_scale 2.0: two passes and the CFG combine, as for every other sampler"""
    spec = _spec("txt2img", 2.0)
    _, cfg_out = _run_twice(dev, spec, use_graph, "tiny LCM 4-step at guidance 2", "cfg_multistep", 2 * spec.B)
    one = _oracle_pair(_spec("txt2img", 1.0), dev)[0]
    assert rel_l2(cfg_out, one) >= 20 * TOL_L2, "guidance 2 and guidance 1 coincide: the comparison says nothing about the path"


def test_tiny_lcm_inpaint_strength_window(dev):
    """strength 0.75 of 4 steps: first_step = 1, three executed steps and two noise tensors; the blend re-noises the kept region
    to the NEXT LCM timestep"""
    spec = _spec("inpaint", 1.0, strength=0.75)
    assert E.executed_steps(spec) == 3
    _run_twice(dev, spec, True, "tiny LCM inpaint, strength 0.75", "multistep", spec.B)


def test_tinyxl_lcm_single_pass(dev):
    """SDXL: the pooled column is p_text / p_aug with B rows and the time ids are the conditional half's"""
    spec = _spec("sdxl", 1.0)
    pipe, _ = _run_twice(dev, spec, True, "tinyxl LCM 4-step single pass", "multistep", spec.B)
    assert pipe._engine._static["pooled"].shape[0] == spec.B and pipe._engine._static["time_ids"].shape[0] == spec.B


def test_tiny_lcm_single_pass_with_a_controlnet(dev):
    spec = _spec("controlnet", 1.0)
    _run_twice(dev, spec, True, "tiny LCM ControlNet-inpaint single pass", "multistep", spec.B)


def test_lcm_draws_its_noise_from_the_generator(dev):
    """``latents`` are given, so the generator's first draws are the loop's: one randn [B, 4, h, w] fp16 per executed step but the
    last, in loop order -- the same seed gives the same bits, and so do those tensors passed as variance_noise"""
    spec = _spec("txt2img", 1.0)
    pipe = _pipeline(dev, spec, True)
    seeded = lambda s: E.call_pipeline(_WithNoise(pipe, generator=torch.Generator(dev).manual_seed(s)), spec, dev)[0].clone()
    a, b = seeded(1234), seeded(1234)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    g2 = torch.Generator(dev).manual_seed(1234)
    shape = E.inputs(spec, str(dev))["latents"].shape
    drawn = torch.stack([torch.randn(shape, generator=g2, device=dev, dtype=torch.float16) for _ in range(STEPS - 1)])
    c = E.call_pipeline(_WithNoise(pipe, variance_noise=drawn), spec, dev)[0]
    assert torch.equal(a, c)
    assert not torch.equal(a, seeded(99))
    with pytest.raises(ValueError, match="variance_noise of shape"):
        E.call_pipeline(_WithNoise(pipe, variance_noise=drawn[:1]), spec, dev)
    one = E.call_pipeline(pipe, spec.but(steps=1), dev)[0]          # a single step needs no noise and no generator
    assert torch.isfinite(one.float()).all()


@pytest.mark.parametrize("name,path", [("ddim", "cfg_ddim"), ("euler", "cfg_ddim"), ("pndm", "cfg_multistep"), ("dpm", "cfg_multistep")])
def test_other_schedulers_keep_their_step_at_guidance_one(dev, name, path):
    """the single pass is LCMScheduler's: the four other classes launch UNet(2B) + their CFG step at guidance_scale 1.0 too"""
    spec = E.Spec(scheduler=name, guidance=1.0)
    pipe = E.pipeline_class(spec)(E.new_unet(str(dev)), scheduler=E.product_scheduler(spec), use_graph=False)
    out, _ = E.call_pipeline(pipe, spec, dev)
    assert pipe._engine.step_path == path and tuple(pipe._engine._static["kvrow"].shape) == (2 * spec.B,)
    assert torch.isfinite(out.float()).all()


# ----------------------------------------------------------------------------------- a UNet with time_cond_proj_dim
def test_time_cond_table_rows(dev):
    """time_embed_table of the UNet with time_cond_proj_dim: every row is time_emb_proj(silu(MLP(sincos(t) + cond_proj(w_emb))))
    for all resnets side by side -- recomputed in torch fp32 and, as the arm, in torch fp16 on the GPU (check_vs_fp16_arm: the
    chain rounds to fp16 after the sum and after each of the three linears)"""
    import torch.nn.functional as F
    from oracle.unet import timestep_embedding
    C = _cond_models(dev)
    hip, sd, cfg = C["hip"], C["sd"], C["cfg"]
    tvals = torch.tensor([999.0, 759.0, 519.0, 279.0])
    names = sorted(hip.packed.temb_offsets, key=hip.packed.temb_offsets.get)
    tables = {}
    for guidance in (1.0, 3.0, 8.0):
        w_emb = _set_guidance(C, guidance)

        def ref(dtype, device):
            p = lambda k: sd[k].half().to(device=device, dtype=dtype)
            x = timestep_embedding(tvals.to(device), cfg.block_out_channels[0]).to(dtype)
            x = x + F.linear(w_emb.to(device=device, dtype=dtype)[None], p("time_embedding.cond_proj.weight"))
            x = F.linear(F.silu(F.linear(x, p("time_embedding.linear_1.weight"), p("time_embedding.linear_1.bias"))),
                         p("time_embedding.linear_2.weight"), p("time_embedding.linear_2.bias"))
            return torch.cat([F.linear(F.silu(x), p(f"{n}.time_emb_proj.weight"), p(f"{n}.time_emb_proj.bias")) for n in names], 1)
        got = hip.time_embed_table(tvals.to(dev), guidance_scale=guidance)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (4, hip.packed.temb_total)
        check_vs_fp16_arm(got, ref(torch.float32, "cpu"), ref(torch.float16, dev), f"time table at guidance_scale {guidance}")
        tables[guidance] = got.clone()
    assert rel_l2(tables[3.0], tables[8.0]) >= 20 * TOL_L2, "the guidance embedding does not move the time rows"
    with pytest.raises(ValueError, match="guidance_scale"):
        hip.time_embed_table(tvals.to(dev))


def test_time_cond_unet_generations(dev):
    """guidance_scale 3 then 8 on one graph pipeline, then 3 again: the single pass at every scale (guidance is in the time
    embedding), each against the hooked oracle on the conditional rows; 3 and 8 differ, and the second run at 3 repeats the
    first bit for bit (no stale time table).  Any other scheduler and guidance_rescale > 0 are refused."""
    from consistentid_amd import pipeline, scheduler
    C = _cond_models(dev)
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(C["hip"], scheduler=scheduler.LCMScheduler(), use_graph=True)
    outs = {}
    for gen, guidance in enumerate((3.0, 8.0, 3.0)):
        spec = _spec("txt2img", guidance)
        _set_guidance(C, guidance)
        ref, arm = _oracle_pair(spec, dev, unets=C["oracles"], single=True)
        out, _ = E.call_pipeline(_WithNoise(pipe, variance_noise=_noises(spec, dev).to(dev)), spec, dev)
        assert pipe._engine.step_path == "multistep" and tuple(pipe._engine._static["kvrow"].shape) == (spec.B,)
        check_vs_fp16_arm(out, ref, arm, f"tiny time_cond_proj_dim UNet, guidance_scale {guidance}, generation {gen}")
        if guidance in outs:
            assert torch.equal(out, outs[guidance]), "the same guidance_scale gives other bits the second time"
        outs[guidance] = out.clone()
    assert rel_l2(outs[3.0], outs[8.0]) >= 20 * TOL_L2
    spec = _spec("txt2img", 3.0)
    with pytest.raises(ValueError, match="guidance_rescale"):
        E.call_pipeline(_WithNoise(pipe, variance_noise=_noises(spec, dev).to(dev), guidance_rescale=0.7), spec, dev)
    for cls in (scheduler.DDIMScheduler, scheduler.EulerDiscreteScheduler, scheduler.PNDMScheduler, scheduler.DPMSolverMultistepScheduler):
        pipe.scheduler = cls()
        with pytest.raises(NotImplementedError, match=cls.__name__):
            E.call_pipeline(pipe, spec, dev)


def test_time_cond_unet_on_the_per_step_time_path(dev, monkeypatch):
    """CID_NO_TEMB_TABLE: the three time GEMVs run in every step, and the guidance row is added there (the path SDXL's
    text_time conditioning always takes); a fresh eager pipeline on the same UNet, against the same reference"""
    from consistentid_amd import pipeline, scheduler
    monkeypatch.setenv("CID_NO_TEMB_TABLE", "1")
    C = _cond_models(dev)
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(C["hip"], scheduler=scheduler.LCMScheduler(), use_graph=False)
    spec = _spec("txt2img", 8.0)
    _set_guidance(C, 8.0)
    ref, arm = _oracle_pair(spec, dev, unets=C["oracles"], single=True)
    out, _ = E.call_pipeline(_WithNoise(pipe, variance_noise=_noises(spec, dev).to(dev)), spec, dev)
    assert pipe._engine.step_path == "multistep" and "temb" not in pipe._engine._static
    check_vs_fp16_arm(out, ref, arm, "tiny time_cond_proj_dim UNet, guidance_scale 8, per-step time path")
