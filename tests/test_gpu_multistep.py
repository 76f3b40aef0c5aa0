"""cid_cfg_multistep_step_f16 on the GPU: the kernel against the float64 model of its row contract, the same launch replayed
from a hipGraph behind cid_step_select, and PNDM / DPM-Solver++ 2M / DDIM-with-eta trajectories of the pipelines on the tiny
UNet pair against ``oracle.loop.denoise`` driven by the stateful restatements of tests/multistep_ref.py."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import check_close, check_vs_fp16_arm, dev_half, half_arm
from multistep_ref import DDIMEtaRef, DPMSolverPP2MRef, PNDMRef, RowEmulator
from oracle_utils import build_oracle, make_weights

pytestmark = pytest.mark.gpu

NAN = float("nan")
BIG = 8 * 262403      # 262403 threads' worth of 8 halfs: past grid_for's cap of 1024 blocks x 256 threads, and not a multiple of it


def _row(a=0.0, b=1.0, c_x=0.0, c_m=0.0, c_hist=(0.0, 0.0, 0.0, 0.0), c_z=0.0, c_init=1.0, c_noise=0.0, w=-1, flags=0, z_row=0):
    """one multistep row as include/cid.h lays it out (word 8: the model-input scale, unused by the kernel)"""
    return [a, b, c_x, c_m, *c_hist, 1.0, c_init, c_noise, c_z, float(w), float(flags), float(z_row), 0.0]


# every write slot and none, one to four ring coefficients, save then restore of the source sample, noise row 2 of 3, and a
# last row that weighs ring slot 0 and overwrites it in the same launch
KERNEL_ROWS = [
    _row(a=0.3, b=0.9, c_x=0.8, c_m=-0.4, w=0, flags=1),
    _row(a=-0.2, b=1.1, c_x=1.05, c_m=0.5, c_hist=(-0.3, 0, 0, 0), w=1),
    _row(a=0.0, b=1.0, c_x=0.9, c_m=0.6, c_hist=(0.2, -0.5, 0, 0), w=2),
    _row(a=1.2, b=-0.7, c_x=0.7, c_m=0.3, c_hist=(0.1, 0.25, -0.45, 0), w=3),
    _row(a=0.5, b=0.5, c_x=0.95, c_m=0.4, c_hist=(0.3, -0.35, 0.2, 0.15), c_z=0.6, w=-1, flags=2, z_row=2),
    _row(a=0.1, b=1.0, c_x=1.0, c_m=-0.5, c_hist=(0.45, -0.2, 0.3, -0.25), c_init=0.8, c_noise=0.6, w=0),
]


def _device_row(row, dev):
    from consistentid_amd.scheduler import pack_step_rows
    return torch.from_numpy(pack_step_rows(np.asarray([row]))[0]).to(dev).view(torch.float32)


@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
@pytest.mark.parametrize("n", [8, 3 * 1024, BIG])
def test_multistep_kernel_matches_the_row_contract(dev, n, inpaint):
    """Six launches that share ring, ``saved`` and ``z`` with the emulator; every launch starts from the GPU's own latents,
    so each one is judged alone (check_close defaults).  The ring, ``saved`` and noise rows 0 and 1 start as NaN: whatever
    a zero coefficient covers must not be read, so every output is finite.  ``saved`` must be a bit copy, the ring fp32."""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(n % 1000 + inpaint)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    B, per = 2, n // 2
    lat = rnd(n).to(dev)
    hist = torch.full((4, n), NAN, device=dev)
    saved = torch.full((n,), NAN, dtype=torch.float16, device=dev)
    z = torch.full((3, n), NAN, dtype=torch.float16)
    z[2] = rnd(n)
    blend_h = blend_e = ()
    if inpaint:
        mask, init, noise = (torch.rand(n, generator=g) > 0.5).half(), rnd(n), rnd(n)
        blend_h = dict(mask=mask.to(dev), init=init.to(dev), noise=noise.to(dev))
        blend_e = tuple(t.double().numpy() for t in (mask, init, noise))
    emu = RowEmulator(n, z=z.double().numpy())
    zd = z.to(dev)
    for k, row in enumerate(KERNEL_ROWS):
        eps = rnd(2 * n)
        x_in = lat.cpu().double().numpy()
        want = emu.step(row, x_in, eps[:n].double().numpy(), eps[n:].double().numpy(), 2.5, *blend_e)
        ops.cfg_multistep_step(eps.to(dev), lat, hist, saved, _device_row(row, dev), 2.5, B=B, per_sample=per, z=zd,
                               **(blend_h or {}))
        torch.cuda.synchronize()
        check_close(lat, torch.from_numpy(want), f"multistep kernel n={n} inpaint={inpaint} row {k}")
        if k == 0:
            assert torch.equal(saved.cpu().double(), torch.from_numpy(x_in)), "saved is not a copy of the incoming sample"
    assert torch.isfinite(hist).all()
    check_close(hist, torch.from_numpy(emu.hist), f"multistep ring n={n}", tol_l2=1e-6, tol_max=1e-6)   # fp32 vs float64
    assert torch.equal(saved.cpu().double(), torch.from_numpy(emu.saved))


def test_multistep_kernel_without_noise_rows(dev):
    """z = NULL: a row's c_z is ignored (nothing to read), the rest of the update is unchanged"""
    from consistentid_amd import ops
    n = 64
    g = torch.Generator().manual_seed(5)
    lat, eps = torch.randn(n, generator=g).half(), torch.randn(2 * n, generator=g).half()
    row = _row(a=0.2, b=1.0, c_x=0.9, c_m=0.5, c_z=0.7, w=1)
    emu = RowEmulator(n)
    want = emu.step(row, lat.double().numpy(), eps[:n].double().numpy(), eps[n:].double().numpy(), 4.0)
    ld, hist = lat.to(dev), torch.full((4, n), NAN, device=dev)
    ops.cfg_multistep_step(eps.to(dev), ld, hist, torch.full((n,), NAN, dtype=torch.float16, device=dev), _device_row(row, dev),
                           4.0, B=1, per_sample=n)
    torch.cuda.synchronize()
    check_close(ld, torch.from_numpy(want), "multistep kernel, no noise rows")
    assert torch.isfinite(hist[1]).all() and torch.isnan(hist[0]).all()


def test_multistep_launch_replays_from_a_graph(dev):
    """One captured launch behind cid_step_select over a 6-row table whose rows change slot, flags and noise row (the model
    output of each step is a table column too): bit-identical to six eager launches, and right against the emulator."""
    from consistentid_amd import ops
    from consistentid_amd.scheduler import pack_step_rows
    n, B = 3 * 1024, 3
    g = torch.Generator().manual_seed(21)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    rows = KERNEL_ROWS[:4] + [_row(a=0.5, b=0.5, c_x=0.95, c_m=0.4, c_hist=(0.3, -0.35, 0.2, 0.15), c_z=0.6, flags=2, z_row=1),
                              _row(a=0.1, b=1.0, c_x=1.0, c_m=-0.5, c_hist=(0.45, -0.2, 0.3, -0.25), c_z=-0.3, w=0, z_row=2)]
    eps_all, lat0, z = rnd(6, 2 * n), rnd(n), rnd(3, n)
    emu, x = RowEmulator(n, z=z.double().numpy()), lat0.double().numpy()
    for k, row in enumerate(rows):
        x = emu.step(row, x, eps_all[k, :n].double().numpy(), eps_all[k, n:].double().numpy(), 3.0)
        x = x.astype(np.float16).astype(np.float64)            # the kernel's one rounding, at the store of the latents
    row_buf = torch.zeros(16, dtype=torch.int32, device=dev)
    eps_buf = torch.zeros(2 * n, dtype=torch.float16, device=dev)
    tab = ops.StepTable([(row_buf, torch.from_numpy(pack_step_rows(np.asarray(rows)))), (eps_buf, eps_all)], dev)
    lat, hist = lat0.to(dev), torch.full((4, n), NAN, device=dev)
    saved, zd = torch.full((n,), NAN, dtype=torch.float16, device=dev), z.to(dev)

    def launch():
        tab.select()
        ops.cfg_multistep_step(eps_buf, lat, hist, saved, row_buf.view(torch.float32), 3.0, B=B, per_sample=n // B, z=zd)

    def start():
        lat.copy_(lat0)
        hist.fill_(NAN)
        saved.fill_(NAN)
        tab.reset(0)
    for _ in range(6):
        launch()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (lat, hist, saved)]
    check_close(lat, torch.from_numpy(x), "six eager multistep launches")
    start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    start()
    for _ in range(6):
        graph.replay()
    torch.cuda.synchronize()
    for got, want, what in zip((lat, hist, saved), eager, ("latents", "ring", "saved")):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), f"graph replay differs from eager launches: {what}"
    check_close(lat, torch.from_numpy(x), "six replayed multistep launches")


# ----------------------------------------------------------------------------------------------------------- trajectories
_PAIRS, _REFS = {}, {}


def _unet_pair(name, dev, rank=8):
    if name not in _PAIRS:
        from consistentid_amd.unet import HipUNet
        cfg, sd, ad = make_weights(name, rank=rank)
        _PAIRS[name] = (cfg, build_oracle(name, sd, ad, rank=rank), HipUNet(cfg, sd, ad, device=dev))
    return _PAIRS[name]


def _schedulers(sampler, noises=None):
    """(the product's scheduler, a factory of the stateful restatement)"""
    from consistentid_amd import scheduler
    if sampler == "pndm":
        return scheduler.PNDMScheduler(), PNDMRef
    if sampler == "dpm":
        return scheduler.DPMSolverMultistepScheduler(), DPMSolverPP2MRef
    return scheduler.DDIMScheduler(), lambda: DDIMEtaRef(1.0, noises)


def _case(dev, name, sampler, steps, inpaint=False, strength=1.0):
    """inputs, fp32 oracle trajectory and fp16-arm trajectory of one case: computed once, shared by the tests that run it"""
    key = (name, sampler, steps, inpaint, strength)
    if key in _REFS:
        return _REFS[key]
    from consistentid_amd import synth
    from oracle import loop
    cfg, oracle, _ = _unet_pair(name, dev)
    B, merge, g = 2, 2, 5.0
    side = cfg.sample_size * 8
    inp = synth.random_inputs(cfg, B, side, side)
    gen = torch.Generator().manual_seed(3)
    lshape = (B, 4, side // 8, side // 8)
    f = lambda k: inp[k].float()
    kw_o, kw_h = {}, {}
    if name == "tinyxl":
        kw_o = dict(add_text_embeds_null=f("pooled_null"), add_text_embeds_text=f("pooled_text"),
                    add_text_embeds_aug=f("pooled_augmented"), add_time_ids=inp["time_ids"])
        kw_h = dict(pooled_prompt_embeds=inp["pooled_augmented"], pooled_prompt_embeds_text_only=inp["pooled_text"],
                    negative_pooled_prompt_embeds=inp["pooled_null"], add_time_ids=inp["time_ids"])
    if inpaint:
        init, noise = torch.randn(lshape, generator=gen).half(), torch.randn(lshape, generator=gen).half()
        mask = (torch.rand(B, 1, *lshape[2:], generator=gen) > 0.5).half()
        kw_o.update(inpaint_mask=mask.float(), inpaint_init=init.float(), inpaint_noise=noise.float(), strength=strength)
        kw_h.update(image_latents=init.to(dev), noise=noise.to(dev), mask_latents=mask.to(dev), strength=strength)
    noises = None
    if sampler == "ddim_eta":
        noises = torch.randn(steps, *lshape, generator=gen).half()
        kw_h.update(eta=1.0, variance_noise=noises.to(dev))
    product, make_ref = _schedulers(sampler, None if noises is None else list(noises.float()))
    common = dict(num_inference_steps=steps, guidance_scale=g, start_merge_step=merge)
    ref = loop.denoise(oracle, make_ref(), f("latents"), f("null"), f("augmented"), f("text"), **common, **kw_o)
    h = lambda k: inp[k].to(dev).half()
    arm = loop.denoise(half_arm(oracle, dev), make_ref(), h("latents"), h("null"), h("augmented"), h("text"), **common,
                       **dev_half(kw_o, dev))
    call = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev), latents=inp["latents"].to(dev),
                output_type="latent", **common, **kw_h)
    _REFS[key] = (product, call, ref, arm)
    return _REFS[key]


def _run_twice(dev, pipe_cls, name, sampler, steps, use_graph, what, **case_kw):
    """two generations on one pipeline -- the second replays the cached graph -- each judged like every fp16 trajectory here"""
    product, call, ref, arm = _case(dev, name, sampler, steps, **case_kw)
    pipe = pipe_cls(_unet_pair(name, dev)[2], scheduler=product, use_graph=use_graph)
    seen = []
    for gen in range(2):
        out = pipe(**call, callback=lambda i, t, l: seen.append(i)).images
        torch.cuda.synchronize()
        assert pipe._engine.step_path == "cfg_multistep"
        check_vs_fp16_arm(out, ref, arm, f"{what}, graph={use_graph}, generation {gen}")
    return pipe, seen


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sampler,steps,evaluations", [("pndm", 6, 7), ("dpm", 6, 6), ("dpm", 2, 2), ("ddim_eta", 6, 6)])
def test_tiny_multistep_trajectory(dev, sampler, steps, evaluations, use_graph):
    """PNDM's 6 steps are 7 UNet evaluations and reach the fourth-order combination; DPM-Solver++ at 6 steps (first order,
    four second-order steps, first-order final step) and at 2 (both first order); DDIM with eta = 1 and given noise.  The
    embed switch and the callback count evaluations."""
    from consistentid_amd import pipeline
    _, seen = _run_twice(dev, pipeline.ConsistentIDStableDiffusionPipeline, "tiny", sampler, steps, use_graph,
                         f"tiny {sampler} {steps}-step trajectory")
    assert seen == 2 * list(range(evaluations))


def test_tiny_pndm_inpaint_blend(dev):
    from consistentid_amd import pipeline
    _run_twice(dev, pipeline.StableDiffusionInpaintConsistentIDPipeline, "tiny", "pndm", 4, True, "tiny PNDM inpaint blend",
               inpaint=True)


def test_tiny_dpm_inpaint_strength_window(dev):
    """strength 0.6 of 10 steps: the last 6 schedule entries, the solver's history starting empty at the first of them"""
    from consistentid_amd import pipeline
    _, seen = _run_twice(dev, pipeline.StableDiffusionInpaintConsistentIDPipeline, "tiny", "dpm", 10, True,
                         "tiny DPM-Solver++ inpaint, strength 0.6", inpaint=True, strength=0.6)
    assert seen == 2 * list(range(6))


def test_tinyxl_dpm_trajectory(dev):
    from consistentid_amd import pipeline
    _run_twice(dev, pipeline.ConsistentIDStableDiffusionXLPipeline, "tinyxl", "dpm", 4, True, "tinyxl DPM-Solver++ 4-step trajectory")


def test_eta_draws_its_noise_from_the_generator(dev):
    """eta = 1 with a generator: one randn [B, 4, h, w] fp16 per executed step in loop order (``latents`` are given, so nothing
    is drawn before the loop) -- bit-identical to the same call with that noise drawn here and passed as variance_noise"""
    from consistentid_amd import pipeline, scheduler
    _, call, _, _ = _case(dev, "tiny", "ddim_eta", 6)
    call = {k: v for k, v in call.items() if k not in ("eta", "variance_noise")}
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(_unet_pair("tiny", dev)[2], scheduler=scheduler.DDIMScheduler())
    a = pipe(**call, eta=1.0, generator=torch.Generator(dev).manual_seed(1234)).images.clone()
    g2 = torch.Generator(dev).manual_seed(1234)
    drawn = torch.stack([torch.randn(call["latents"].shape, generator=g2, device=dev, dtype=torch.float16) for _ in range(6)])
    b = pipe(**call, eta=1.0, variance_noise=drawn).images
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    c = pipe(**call, eta=1.0, generator=torch.Generator(dev).manual_seed(99)).images
    assert not torch.equal(a, c)
    with pytest.raises(ValueError, match="DDIM"):
        pipeline.ConsistentIDStableDiffusionPipeline(_unet_pair("tiny", dev)[2], scheduler=scheduler.PNDMScheduler())(**call, eta=1.0)


def test_ddim_eta0_keeps_its_step_kernel(dev):
    """DDIM at eta = 0 still runs on cid_cfg_ddim_step_f16 -- also on a pipeline that has just run PNDM and switches back: the
    4-step tiny trajectory is bit-identical before and after (its hash is printed for the record)."""
    from consistentid_amd import pipeline, scheduler, synth
    cfg, _, hip = _unet_pair("tiny", dev)
    side = cfg.sample_size * 8
    inp = synth.random_inputs(cfg, 2, side, side)
    call = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev), latents=inp["latents"].to(dev),
                num_inference_steps=4, guidance_scale=5.0, start_merge_step=1, output_type="latent")
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(hip, use_graph=True)
    first = pipe(**call).images.clone()
    assert pipe._engine.step_path == "cfg_ddim"
    pipe.scheduler = scheduler.PNDMScheduler.from_config(pipe.scheduler.config)
    pipe(**call)
    assert pipe._engine.step_path == "cfg_multistep"
    pipe.scheduler = scheduler.DDIMScheduler.from_config(pipe.scheduler.config)
    again = pipe(**call).images
    torch.cuda.synchronize()
    assert pipe._engine.step_path == "cfg_ddim" and torch.equal(first, again)
    print("[hash] tiny DDIM eta=0 4-step latents sha256 =", hashlib.sha256(first.cpu().numpy().tobytes()).hexdigest())
