"""guidance_rescale, v-prediction and zero-SNR DDIM on the GPU: cid_cfg_rescale_f16 against float64 on the same fp16 inputs,
the scaled step entries against the float64 models of their contracts with the factor applied, trajectories of the pipelines
on the tiny UNet pair against ``oracle.loop.denoise`` (unchanged) driven by tests/vpred_ref.py, and the default path: at
guidance_rescale = 0 the engine launches, captures and computes what it did before the keyword was honoured."""
import numpy as np
import pytest
import torch

from conftest import check_close, check_vs_fp16_arm, dev_half, half_arm
from multistep_ref import RowEmulator
from oracle_utils import build_oracle, make_weights
from test_gpu_multistep import KERNEL_ROWS, _device_row
from vpred_ref import DDIMRef, DPMSolverVRef, EulerRef, PNDMVRef, RescaledUNet

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 7.5
# one item; 257 items: ragged against the workgroup's 1024-thread stride and against a wave; the SD1.5 and the SDXL sample
SHAPES = [(1, 8), (3, 8 * 257), (2, 16384), (2, 65536)]
FAMILIES = [(0.0, 1.0), (3.0, 0.1), (30.0, 0.05)]
_FACTOR_MAXIMA = {}


def _factor_inputs(B, per, mean, sigma):
    g = torch.Generator().manual_seed(B * 1000003 + per + int(mean * 10))
    return (mean + sigma * torch.randn(2 * B, per, generator=g)).half()


def _factor_ref(eps, g, phi):
    """float64 on the fp16 inputs: 1 - phi + phi std(c) / std(e), e = u + g (c - u)"""
    B = eps.shape[0] // 2
    u, c = eps[:B].double(), eps[B:].double()
    e = u + g * (c - u)
    return 1.0 - phi + phi * c.std(dim=1) / e.std(dim=1)


@pytest.mark.parametrize("phi", [0.7, 1.0])
@pytest.mark.parametrize("mean,sigma", FAMILIES, ids=[f"mean{m:g}-sigma{s:g}" for m, s in FAMILIES])
@pytest.mark.parametrize("B,per", SHAPES, ids=[f"B{b}-per{p}" for b, p in SHAPES])
def test_factor_kernel_against_float64(dev, B, per, mean, sigma, phi):
    """relative error of escale <= 1e-5: ten times the worst value of a Welford / Chan reduction in fp32 on these inputs, a
    third of the best a sum / sum-of-squares reduction reaches on the offset ones.  The buffer starts as NaN (every entry is
    written) and a second launch gives the same bits (no atomics, fixed merge order)."""
    from consistentid_amd import ops
    eps = _factor_inputs(B, per, mean, sigma)
    want = _factor_ref(eps, G, phi)
    epsd = eps.to(dev)
    out = torch.full((B,), NAN, device=dev)
    ops.cfg_rescale(epsd, G, phi, out, B=B, per_sample=per)
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(NAN)
    ops.cfg_rescale(epsd, G, phi, out, B=B, per_sample=per)
    torch.cuda.synchronize()
    err = float(((out.cpu().double() - want).abs() / want.abs()).max())
    _FACTOR_MAXIMA[(mean, sigma)] = max(_FACTOR_MAXIMA.get((mean, sigma), 0.0), err)
    print(f"[parity] escale B={B} per_sample={per} mean={mean:g} sigma={sigma:g} phi={phi}: max relative error {err:.3e}; "
          f"maximum so far for this input family {_FACTOR_MAXIMA[(mean, sigma)]:.3e}")
    assert torch.isfinite(out).all(), "an escale entry was not written"
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), "two launches on the same input differ"
    assert err <= 1e-5


def test_factor_kernel_constant_sample_and_zero_rescale(dev):
    """std(e) == 0 -> exactly 1.0 (diffusers divides by zero there); the neighbouring random sample is unaffected; at
    rescale = 0 the factor is exactly 1.0 for every sample"""
    from consistentid_amd import ops
    B, per = 3, 8 * 257
    eps = _factor_inputs(B, per, 3.0, 0.1)
    eps[0], eps[B + 0] = 0.5, 1.25           # u and c constant and different: e = 0.5 + 7.5 * 0.75, the same in every element
    eps[2], eps[B + 2] = -2.0, -2.0
    out = torch.full((B,), NAN, device=dev)
    ops.cfg_rescale(eps.to(dev), G, 0.7, out, B=B, per_sample=per)
    torch.cuda.synchronize()
    got = out.cpu()
    assert got[0] == 1.0 and got[2] == 1.0
    want = _factor_ref(eps[[1, B + 1]], G, 0.7)
    assert abs(float(got[1]) - float(want[0])) <= 1e-5 * float(want[0])
    out.fill_(NAN)
    ops.cfg_rescale(eps.to(dev), G, 0.0, out, B=B, per_sample=per)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.ones(B))


# ------------------------------------------------------------------------------------------------ the scaled step entries
ESCALE = [0.5, 1.0, 1.375]
B3, PER3 = 3, 8 * 257


def _blend(g, n, dev, inpaint):
    if not inpaint:
        return {}, ()
    mask, init, noise = (torch.rand(n, generator=g) > 0.5).half(), torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
    return dict(mask=mask.to(dev), init=init.to(dev), noise=noise.to(dev)), tuple(t.double().numpy() for t in (mask, init, noise))


def _scaled_e(eps, n, g, escale):
    """the guided prediction times its sample's factor, in float64"""
    u, c = eps[:n].double().numpy(), eps[n:].double().numpy()
    return (u + g * (c - u)) * np.repeat(np.asarray(escale, dtype=np.float64), n // len(escale))


@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
def test_scaled_ddim_step_matches_its_contract(dev, inpaint):
    """x' = c_x x + c_eps e escale[sample] (+ blend), a distinct factor per sample; all factors 1.0: the unscaled entry's bits"""
    from consistentid_amd import ops
    n = B3 * PER3
    g = torch.Generator().manual_seed(11 + inpaint)
    lat0, eps = torch.randn(n, generator=g).half(), torch.randn(2 * n, generator=g).half()
    coef = torch.tensor([0.9, -0.35, 0.8, 0.6, 1.0])
    blend_h, blend_e = _blend(g, n, dev, inpaint)
    want = coef[0].item() * lat0.double().numpy() + float(coef[1]) * _scaled_e(eps, n, 2.5, ESCALE)
    if inpaint:
        k, init, noise = blend_e
        want = (1.0 - k) * (float(coef[2]) * init + float(coef[3]) * noise) + k * want
    lat = lat0.to(dev)
    ops.cfg_ddim_step(eps.to(dev), lat, coef.to(dev), 2.5, B=B3, per_sample=PER3, escale=torch.tensor(ESCALE, device=dev), **blend_h)
    torch.cuda.synchronize()
    check_close(lat, torch.from_numpy(want), f"scaled DDIM step inpaint={inpaint}")
    plain, ones = lat0.to(dev), lat0.to(dev)
    ops.cfg_ddim_step(eps.to(dev), plain, coef.to(dev), 2.5, B=B3, per_sample=PER3, **blend_h)
    ops.cfg_ddim_step(eps.to(dev), ones, coef.to(dev), 2.5, B=B3, per_sample=PER3, escale=torch.ones(B3, device=dev), **blend_h)
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.int16), ones.view(torch.int16)), "escale = 1.0 is not the unscaled entry"
    assert not torch.equal(plain, lat)


@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
def test_scaled_multistep_step_matches_the_row_contract(dev, inpaint):
    """test_multistep_kernel_matches_the_row_contract's six launches -- every ring slot, save / restore, a noise row -- with a
    distinct factor per sample, against the emulator fed e * escale (its tolerances: check_close defaults per launch, 1e-6 for
    the fp32 ring, ``saved`` a bit copy); beside them the unscaled entry and the scaled one at 1.0, bit for bit."""
    from consistentid_amd import ops
    n = B3 * PER3
    g = torch.Generator().manual_seed(31 + inpaint)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    lat = rnd(n).to(dev)
    z = torch.full((3, n), NAN, dtype=torch.float16)
    z[2] = rnd(n)
    blend_h, blend_e = _blend(g, n, dev, inpaint)
    new_state = lambda: (torch.full((4, n), NAN, device=dev), torch.full((n,), NAN, dtype=torch.float16, device=dev))
    (hist, saved), (hist_p, saved_p), (hist_1, saved_1) = new_state(), new_state(), new_state()
    lat_p, lat_1 = lat.clone(), lat.clone()
    emu = RowEmulator(n, z=z.double().numpy())
    zd, esd, ones = z.to(dev), torch.tensor(ESCALE, device=dev), torch.ones(B3, device=dev)
    for k, row in enumerate(KERNEL_ROWS):
        eps = rnd(2 * n)
        x_in = lat.cpu().double().numpy()
        e = _scaled_e(eps, n, 2.5, ESCALE)
        want = emu.step(row, x_in, e, e, 2.5, *blend_e)            # e + g (e - e) = e
        epsd, rowd = eps.to(dev), _device_row(row, dev)
        ops.cfg_multistep_step(epsd, lat, hist, saved, rowd, 2.5, B=B3, per_sample=PER3, z=zd, escale=esd, **blend_h)
        ops.cfg_multistep_step(epsd, lat_p, hist_p, saved_p, rowd, 2.5, B=B3, per_sample=PER3, z=zd, **blend_h)
        ops.cfg_multistep_step(epsd, lat_1, hist_1, saved_1, rowd, 2.5, B=B3, per_sample=PER3, z=zd, escale=ones, **blend_h)
        torch.cuda.synchronize()
        check_close(lat, torch.from_numpy(want), f"scaled multistep step inpaint={inpaint} row {k}")
        if k == 0:
            assert torch.equal(saved.cpu().double(), torch.from_numpy(x_in)), "saved is not a copy of the incoming sample"
        for a, b, what in ((lat_p, lat_1, "latents"), (hist_p, hist_1, "ring"), (saved_p, saved_1, "saved")):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"row {k}: escale = 1.0 is not the unscaled entry: {what}"
    assert torch.isfinite(hist).all()
    check_close(hist, torch.from_numpy(emu.hist), "scaled multistep ring", tol_l2=1e-6, tol_max=1e-6)   # fp32 vs float64
    assert torch.equal(saved.cpu().double(), torch.from_numpy(emu.saved))


# ----------------------------------------------------------------------------------------------------------- trajectories
_PAIRS, _REFS = {}, {}
ZERO_SNR = dict(rescale_betas_zero_snr=True, timestep_spacing="trailing")


def _unet_pair(name, dev, rank=8):
    if name not in _PAIRS:
        from consistentid_amd.unet import HipUNet
        cfg, sd, ad = make_weights(name, rank=rank)
        _PAIRS[name] = (cfg, build_oracle(name, sd, ad, rank=rank), HipUNet(cfg, sd, ad, device=dev))
    return _PAIRS[name]


def _schedulers(sampler, prediction_type, zero_snr):
    """(the product's scheduler, a factory of the stateful restatement)"""
    from consistentid_amd import scheduler
    product_cls, ref_cls = {"ddim": (scheduler.DDIMScheduler, DDIMRef), "euler": (scheduler.EulerDiscreteScheduler, EulerRef),
                            "pndm": (scheduler.PNDMScheduler, PNDMVRef),
                            "dpm": (scheduler.DPMSolverMultistepScheduler, DPMSolverVRef)}[sampler]
    kw = dict(prediction_type=prediction_type, **(ZERO_SNR if zero_snr else {}))
    return product_cls(**kw), lambda: ref_cls(**kw)


def _case(dev, name, sampler, steps, phi, prediction_type="epsilon", inpaint=False, zero_snr=False):
    """inputs, fp32 oracle trajectory and fp16-arm trajectory of one case: computed once, shared by the tests that run it.
    The oracle side is ``oracle.loop.denoise`` as it is, on a UNet wrapped by vpred_ref.RescaledUNet."""
    key = (name, sampler, steps, phi, prediction_type, inpaint, zero_snr)
    if key in _REFS:
        return _REFS[key]
    from consistentid_amd import synth
    from oracle import loop
    cfg, oracle, _ = _unet_pair(name, dev)
    B, merge, g = 2, 1, 5.0
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
        kw_o.update(inpaint_mask=mask.float(), inpaint_init=init.float(), inpaint_noise=noise.float())
        kw_h.update(image_latents=init.to(dev), noise=noise.to(dev), mask_latents=mask.to(dev))
    product, make_ref = _schedulers(sampler, prediction_type, zero_snr)
    probe = make_ref()
    probe.set_timesteps(steps)
    sigma0 = float(probe.init_noise_sigma)
    common = dict(num_inference_steps=steps, guidance_scale=g, start_merge_step=merge)
    wrap = (lambda u: RescaledUNet(u, g, phi)) if phi > 0.0 else (lambda u: u)
    ref = loop.denoise(wrap(oracle), make_ref(), f("latents") * sigma0, f("null"), f("augmented"), f("text"), **common, **kw_o)
    h = lambda k: inp[k].to(dev).half()
    arm = loop.denoise(wrap(half_arm(oracle, dev)), make_ref(), h("latents") * sigma0, h("null"), h("augmented"), h("text"),
                       **common, **dev_half(kw_o, dev))
    call = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev), latents=inp["latents"].to(dev),
                output_type="latent", **common, **kw_h)
    if phi > 0.0:
        call["guidance_rescale"] = phi
    _REFS[key] = (product, call, ref, arm)
    return _REFS[key]


def _pipe_cls(name, inpaint):
    from consistentid_amd import pipeline
    if inpaint:
        return pipeline.StableDiffusionInpaintConsistentIDPipeline
    return pipeline.ConsistentIDStableDiffusionXLPipeline if name == "tinyxl" else pipeline.ConsistentIDStableDiffusionPipeline


TRAJECTORIES = [
    # name, sampler, steps, phi, prediction type, inpaint, zero-SNR, the step launch
    ("tiny", "ddim", 4, 0.7, "epsilon", False, False, "cfg_ddim+rescale"),
    ("tiny", "dpm", 4, 0.7, "epsilon", False, False, "cfg_multistep+rescale"),
    ("tinyxl", "euler", 4, 0.7, "epsilon", False, False, "cfg_ddim+rescale"),
    ("tiny", "pndm", 4, 0.5, "epsilon", True, False, "cfg_multistep+rescale"),
    ("tiny", "ddim", 4, 0.0, "v_prediction", False, False, "cfg_ddim"),
    ("tiny", "euler", 4, 0.0, "v_prediction", False, False, "cfg_ddim"),
    ("tiny", "pndm", 4, 0.0, "v_prediction", False, False, "cfg_multistep"),
    ("tiny", "dpm", 4, 0.0, "v_prediction", False, False, "cfg_multistep"),
    ("tiny", "ddim", 4, 0.7, "v_prediction", False, True, "cfg_ddim+rescale"),
]


@pytest.mark.parametrize("name,sampler,steps,phi,prediction_type,inpaint,zero_snr,path", TRAJECTORIES,
                         ids=[f"{c[0]}-{c[1]}-phi{c[3]}-{c[4]}{'-inpaint' if c[5] else ''}{'-zero_snr' if c[6] else ''}"
                              for c in TRAJECTORIES])
def test_trajectory(dev, name, sampler, steps, phi, prediction_type, inpaint, zero_snr, path):
    """two generations on one pipeline -- eager warm-up and capture in the first, the second replays the graph -- each judged
    like every fp16 trajectory here (conftest.check_vs_fp16_arm, defaults)"""
    product, call, ref, arm = _case(dev, name, sampler, steps, phi, prediction_type, inpaint, zero_snr)
    pipe = _pipe_cls(name, inpaint)(_unet_pair(name, dev)[2], scheduler=product, use_graph=True)
    for gen in range(2):
        out = pipe(**call).images
        torch.cuda.synchronize()
        assert pipe._engine.step_path == path
        check_vs_fp16_arm(out, ref, arm, f"{name} {sampler} {steps}-step {prediction_type} guidance_rescale={phi}"
                          f"{' inpaint' if inpaint else ''}{' zero-SNR trailing' if zero_snr else ''}, generation {gen}")
    assert pipe._engine.captures, "nothing was captured, so nothing was replayed"
    if zero_snr:
        assert int(product.timesteps[0]) == 999 and product.alphas_cumprod[999] == 0.0


def test_guidance_rescale_changes_the_sample(dev):
    """the keyword is honoured: phi = 0.7 moves the tiny DDIM latents well outside the parity tolerance"""
    _, _, ref0, _ = _case(dev, "tiny", "ddim", 4, 0.0)
    _, _, ref7, _ = _case(dev, "tiny", "ddim", 4, 0.7)
    assert float((ref7 - ref0).norm() / ref0.norm()) > 1e-2


# ----------------------------------------------------------------------------------------------------------- default path
def test_default_path_is_untouched(dev):
    """guidance_rescale = 0.0 and the keyword omitted: the same bits, step launch and captures; 0 -> 0.7 -> 0 on one pipeline
    captures one more graph and returns to the first result bit for bit; guidance_scale = 1 switches the rescale off
    (diffusers' condition)"""
    from consistentid_amd import pipeline
    _, call, _, _ = _case(dev, "tiny", "ddim", 4, 0.0)
    hip = _unet_pair("tiny", dev)[2]
    omitted = pipeline.ConsistentIDStableDiffusionPipeline(hip, use_graph=True)
    a = omitted(**call).images.clone()
    zero = pipeline.ConsistentIDStableDiffusionPipeline(hip, use_graph=True)
    b = zero(**call, guidance_rescale=0.0).images.clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert omitted._engine.step_path == zero._engine.step_path == "cfg_ddim"
    assert len(omitted._engine.captures) == len(zero._engine.captures) == 1
    assert omitted._engine.captures == zero._engine.captures
    assert "escale" not in zero._engine._static
    c = zero(**call, guidance_rescale=0.7).images.clone()
    torch.cuda.synchronize()
    assert zero._engine.step_path == "cfg_ddim+rescale" and len(zero._engine.captures) == 2
    assert torch.isfinite(c.float()).all() and not torch.equal(b, c)
    d = zero(**call, guidance_rescale=0.0).images.clone()
    torch.cuda.synchronize()
    assert zero._engine.step_path == "cfg_ddim" and torch.equal(b, d)
    print(f"[engine] guidance_rescale 0 -> 0.7 -> 0: captures {len(zero._engine.captures)}")
    one = dict(call, guidance_scale=1.0)
    e = zero(**one).images.clone()
    f = zero(**one, guidance_rescale=0.7).images.clone()
    torch.cuda.synchronize()
    assert zero._engine.step_path == "cfg_ddim" and torch.equal(e, f)
    with pytest.raises(ValueError, match="guidance_rescale"):
        zero(**call, guidance_rescale=-0.5)
