"""MultiControlNet on the GPU: cid_residual_accum_f16 against an fp64 reference, HipMultiControlNet against the summed
oracle nets, the ControlNet-inpaint pipeline with two nets (per-net images, scales and guidance windows; eager and
captured) against the oracle loop, and the single-net paths beside it."""
import functools

import numpy as np
import pytest
import torch

from conftest import check_vs_fp16_arm
from engine_cases import OracleMulti as _OracleMulti, loop_inputs as _loop_inputs, models as _models

pytestmark = pytest.mark.gpu

SCALE_SET = (0.5, -1.25, 1.0, 0.3)
GRID_TILES = 2048            # the launch's grid cap; a tile is 256 lanes x 8 halves
TILE_ELEMS = 256 * 8


# --------------------------------------------------------------------------- the kernel
def _accum_case(dev, shapes, n_nets, seed, nan_net=None):
    """shapes: [(n, nr)] per segment.  Returns (got, ref fp64, magnitude fp64) per segment, all on the CPU.
    ``nan_net``: that net gets scale 0 and NaN-filled residuals."""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(seed)
    scales = [SCALE_SET[int(i)] for i in torch.randint(0, 4, (n_nets,), generator=g)]
    if n_nets == 4:
        scales = [SCALE_SET[int(i)] for i in torch.randperm(4, generator=g)]          # every value of the set
    ys = [torch.randn(n, generator=g).half() for n, _ in shapes]
    rs = [[torch.randn(nr, generator=g).half() for _, nr in shapes] for _ in range(n_nets)]
    if nan_net is not None:
        scales[nan_net] = 0.0
        rs[nan_net] = [torch.full_like(r, float("nan")) for r in rs[nan_net]]
    sc32 = torch.tensor(scales, dtype=torch.float32)
    yd = [y.to(dev) for y in ys]
    ops.residual_accum(yd, [[r.to(dev) for r in net] for net in rs], sc32.to(dev))
    torch.cuda.synchronize()
    out = []
    for j, (n, nr) in enumerate(shapes):
        ref, mag = ys[j].double(), ys[j].double().abs()
        for k in range(n_nets):
            if scales[k] == 0.0:
                continue                                   # contributes nothing; its buffers may hold anything
            term = float(sc32[k]) * rs[k][j].double().repeat(n // nr)      # the fp32 scale the kernel reads, exactly
            ref, mag = ref + term, mag + term.abs()
        out.append((yd[j].cpu(), ref, mag))
    return out, (ys, rs, scales)


def _check_bound(results, what):
    """|got - ref| <= 2^-11 |ref| + 2^-20 (|y| + sum |s_k r_k|) + 2^-24: one fp16 rounding, a generous cover for at most
    five fp32 operations (fused or not), the fp16 subnormal step"""
    worst = 0.0
    for j, (got, ref, mag) in enumerate(results):
        assert torch.isfinite(got.float()).all(), f"{what}: segment {j} is not finite"
        err = (got.double() - ref).abs()
        bound = 2.0 ** -11 * ref.abs() + 2.0 ** -20 * mag + 2.0 ** -24
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        bad = int((err > bound).sum())
        assert bad == 0, f"{what}: segment {j}: {bad} of {err.numel()} elements outside the bound (worst {ratio:.3f} x)"
    print(f"[accum] {what}: worst error / bound = {worst:.3f}")


def _halved(sizes):
    return [(n, n // 2 if (n // 2) % 8 == 0 else n) for n in sizes]


MIXED = [8, 320, 2056, 40, 65544, 16, 4096, 2048, 2040, 1288, 8200, 640, 24, 10248, 56, 131080]
ACCUM_CASES = {
    "one_segment_of_8": [(8, 8)],
    "n16_nr8": [(16, 8)],
    "three_segments": [(8, 8), (2056, 2056), (65544, 65544)],
    "three_segments_halved": _halved([8, 2056, 65544]),            # (none of the three halves is a multiple of 8)
    "three_segments_halved_16": _halved([16, 2064, 65552]),        # the neighbouring sizes whose halves are
    "13_segments": [(n, n) for n in MIXED[:13]],
    "16_segments": _halved(MIXED),
}


@pytest.mark.parametrize("n_nets", [1, 2, 4])
@pytest.mark.parametrize("case", sorted(ACCUM_CASES))
def test_residual_accum_vs_fp64(dev, case, n_nets):
    results, _ = _accum_case(dev, ACCUM_CASES[case], n_nets, seed=len(case) * 7 + n_nets)
    _check_bound(results, f"{case}, {n_nets} nets")


def test_residual_accum_more_tiles_than_the_grid(dev):
    """2049 + 2 tiles on a grid capped at 2048 workgroups: the second pass of the stride loop ends one segment and
    covers the next"""
    shapes = [((GRID_TILES + 1) * TILE_ELEMS - 32, ((GRID_TILES + 1) * TILE_ELEMS - 32) // 2), (2056, 2056)]
    assert sum(-(-n // TILE_ELEMS) for n, _ in shapes) > GRID_TILES
    results, _ = _accum_case(dev, shapes, 2, seed=5)
    _check_bound(results, "grid-stride")


def test_residual_accum_skips_a_net_at_scale_zero(dev):
    """a net at scale 0 is not read: NaN-filled residuals leave the output finite and equal, bit for bit, to the launch
    without that net"""
    from consistentid_amd import ops
    shapes = [(16, 8), (2056, 2056), (4112, 2056)]
    results, (ys, rs, scales) = _accum_case(dev, shapes, 3, seed=9, nan_net=1)
    _check_bound(results, "NaN net at scale 0")
    yd = [y.to(dev) for y in ys]
    ops.residual_accum(yd, [[r.to(dev) for r in rs[k]] for k in (0, 2)], torch.tensor([scales[0], scales[2]], device=dev))
    torch.cuda.synchronize()
    for (got, _, _), y in zip(results, yd):
        assert torch.equal(got, y.cpu())
    # a net that did not run at all (None): same bits again
    yn = [y.to(dev) for y in ys]
    ops.residual_accum(yn, [[r.to(dev) for r in rs[0]], None, [r.to(dev) for r in rs[2]]],
                       torch.tensor(scales + [0.0], device=dev))
    torch.cuda.synchronize()
    for (got, _, _), y in zip(results, yn):
        assert torch.equal(got, y.cpu())


def test_residual_accum_drops_stale_groupnorm_statistics(dev):
    from consistentid_amd import ops
    y = torch.zeros(64, dtype=torch.float16, device=dev)
    y._gn_stats = (torch.zeros(1, device=dev), 1)
    ops.residual_accum([y], [[torch.ones(64, dtype=torch.float16, device=dev)]], torch.ones(1, device=dev))
    assert not hasattr(y, "_gn_stats") and float(y.sum()) == 64.0


# --------------------------------------------------------------------------- forward
def test_multi_controlnet_forward(dev):
    """HipMultiControlNet.__call__ of two tiny nets: the 6 + 1 summed residuals against the fp32 oracle nets scaled and
    summed; the arm is each oracle net in fp16, scaled and summed in fp16 as diffusers' MultiControlNetModel does"""
    from consistentid_amd import synth
    from consistentid_amd.controlnet import HipMultiControlNet
    M = _models(str(dev))
    cfg, B, scales = M["cfg"], 2, [0.6, 1.3]
    side = cfg.sample_size * 8
    inp = synth.random_inputs(cfg, B, side, side)
    g = torch.Generator().manual_seed(17)
    imgs = [torch.rand(B, 3, side, side, generator=g).half() for _ in range(2)]
    multi = HipMultiControlNet([M["new_cn"](0), M["new_cn"](1)])
    assert len(multi.nets) == 2

    def summed(nets, f):
        down = mid = None
        for net, img, s in zip(nets, imgs, scales):
            d, m = net(f(inp["latents"]), 481, f(inp["text"]), f(img), conditioning_scale=s)
            down, mid = (d, m) if down is None else ([a + b for a, b in zip(down, d)], mid + m)
        return down + [mid]

    with torch.no_grad():
        ref = summed(M["o_cns"], lambda t: t.float())
        arm = summed(M["a_cns"], lambda t: t.to(dev))
    hd, hm = multi(inp["latents"].to(dev), 481, encoder_hidden_states=inp["text"].to(dev),
                   controlnet_cond=[i.to(dev) for i in imgs], conditioning_scale=scales, return_dict=False)
    torch.cuda.synchronize()
    assert len(hd) == 6
    for i, (h, r, a) in enumerate(zip(hd + [hm], ref, arm)):
        assert h.shape == r.shape, (i, h.shape, r.shape)
        check_vs_fp16_arm(h, r, a, f"two tiny ControlNets, summed residual {i}")
    with pytest.raises(ValueError, match="1 control images for 2 ControlNets"):
        multi(inp["latents"].to(dev), 481, encoder_hidden_states=inp["text"].to(dev), controlnet_cond=imgs[0].to(dev),
              conditioning_scale=scales)
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        multi.nets[0](inp["latents"].to(dev), 481, encoder_hidden_states=inp["text"].to(dev), controlnet_cond=imgs[0].to(dev),
                      conditioning_scale=scales)


# --------------------------------------------------------------------------- loop
STEPS, MERGE, GUIDANCE = 4, 1, 5.0
WINDOWS = {"overlap": [(0.0, 0.75), (0.25, 1.0)],       # active sets {0}, {0,1}, {0,1}, {1}
           "gap": [(0.0, 0.5), (0.75, 1.0)]}             # active sets {0}, {0}, {}, {1}
ACTIVE = {"overlap": [(0,), (0, 1), (0, 1), (1,)], "gap": [(0,), (0,), (), (1,)]}


@functools.lru_cache(maxsize=None)
def _loop_reference(dev_str, windows, scales):
    """(fp32 oracle, fp16 arm) latents of one generation; shared by the eager and the captured run"""
    from oracle import ddim, loop
    dev = torch.device(dev_str)
    M = _models(dev_str)
    inp, imgs, init, noise, mask = _loop_inputs(M["cfg"])
    out = []
    for unet, nets, f in ((M["o_unet"], M["o_cns"], lambda t: t.float()), (M["a_unet"], M["a_cns"], lambda t: t.to(dev))):
        wrap = _OracleMulti(nets, scales, WINDOWS[windows], STEPS)
        out.append(loop.denoise(unet, ddim.DDIMScheduler(), f(inp["latents"]), f(inp["null"]), f(inp["augmented"]), f(inp["text"]),
                                num_inference_steps=STEPS, guidance_scale=GUIDANCE, start_merge_step=MERGE,
                                inpaint_mask=f(mask), inpaint_init=f(init), inpaint_noise=f(noise),
                                controlnet=wrap, control_image=[f(i) for i in imgs]))
        assert wrap.calls == STEPS
    return out


@pytest.mark.parametrize("windows", sorted(WINDOWS))
@pytest.mark.parametrize("use_graph", [False, True])
def test_multi_controlnet_inpaint_loop(dev, use_graph, windows):
    """Two nets, 4 DDIM steps, merge after step 1, inpaint blend, per-net windows.  Generation 1 at scales [0.5, 0.8],
    generation 2 at [1.0, 0.2]; each must match the oracle at ITS scales.  Captured: a set of nets is warmed up eagerly the
    first time it occurs and captured the second time, so generation 2 still captures the sets generation 1 met once -- but
    nothing that was captured is captured again, and a third generation at yet other scales captures nothing at all."""
    from consistentid_amd import pipeline
    from consistentid_amd.controlnet import active_nets, align_control_guidance, controlnet_keep_table
    M = _models(str(dev))
    inp, imgs, init, noise, mask = _loop_inputs(M["cfg"])
    starts, ends = [w[0] for w in WINDOWS[windows]], [w[1] for w in WINDOWS[windows]]
    assert [active_nets(r) for r in controlnet_keep_table(STEPS, *align_control_guidance(starts, ends, 2))] == ACTIVE[windows]
    pipe = pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline(
        M["new_unet"](), controlnet=[M["new_cn"](0), M["new_cn"](1)], use_graph=use_graph)
    eng = pipe._engine
    pe = torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev)

    def generate(scales):
        out = pipe(prompt_embeds=pe, latents=inp["latents"].to(dev), control_image=[i.to(dev) for i in imgs],
                   num_inference_steps=STEPS, guidance_scale=GUIDANCE, start_merge_step=MERGE, output_type="latent",
                   image_latents=init.to(dev), noise=noise.to(dev), mask_latents=mask.to(dev),
                   controlnet_conditioning_scale=scales, control_guidance_start=starts, control_guidance_end=ends).images
        torch.cuda.synchronize()
        return out

    seen = []
    for gen, scales in enumerate(((0.5, 0.8), (1.0, 0.2))):
        out = generate(list(scales))
        ref, arm = _loop_reference(str(dev), windows, scales)
        check_vs_fp16_arm(out, ref, arm, f"two-ControlNet inpaint loop ({windows}, graph={use_graph}, generation {gen + 1})")
        seen.append((list(eng.captures), dict(eng._graphs)))
    if use_graph:
        once = [a for a in set(ACTIVE[windows]) if ACTIVE[windows].count(a) == 1]
        twice = [a for a in set(ACTIVE[windows]) if ACTIVE[windows].count(a) > 1]
        assert sorted(seen[0][0]) == sorted(twice)                               # generation 1 captured what it met twice
        assert sorted(seen[1][0]) == sorted(twice + once)                        # generation 2 only added the rest
        assert all(seen[1][1][k] is g for k, g in seen[0][1].items())            # ... and kept generation 1's graphs
        third = generate([0.3, 0.9])
        assert torch.isfinite(third.float()).all() and not torch.equal(third, out)
        assert eng.captures == seen[1][0] and all(eng._graphs[k] is g for k, g in seen[1][1].items())
    else:
        assert not eng.captures and not eng._graphs


# --------------------------------------------------------------------------- single-net consistency
def _single_reference(dev_str):
    from oracle import ddim, loop
    dev = torch.device(dev_str)
    M = _models(dev_str)
    inp, imgs, init, noise, mask = _loop_inputs(M["cfg"])
    out = []
    for unet, net, f in ((M["o_unet"], M["o_cns"][0], lambda t: t.float()), (M["a_unet"], M["a_cns"][0], lambda t: t.to(dev))):
        out.append(loop.denoise(unet, ddim.DDIMScheduler(), f(inp["latents"]), f(inp["null"]), f(inp["augmented"]), f(inp["text"]),
                                num_inference_steps=STEPS, guidance_scale=GUIDANCE, start_merge_step=MERGE,
                                inpaint_mask=f(mask), inpaint_init=f(init), inpaint_noise=f(noise),
                                controlnet=net, control_image=f(imgs[0]), conditioning_scale=0.5,
                                control_guidance_start=0.0, control_guidance_end=0.75))
    return out


def _single_call(pipe, dev, control_image):
    """the call of test_gpu_controlnet.py::test_controlnet_inpaint_loop"""
    M = _models(str(dev))
    inp, imgs, init, noise, mask = _loop_inputs(M["cfg"])
    pe = torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev)
    out = pipe(prompt_embeds=pe, latents=inp["latents"].to(dev), control_image=control_image, num_inference_steps=STEPS,
               guidance_scale=GUIDANCE, start_merge_step=MERGE, output_type="latent", image_latents=init.to(dev),
               noise=noise.to(dev), mask_latents=mask.to(dev), control_guidance_end=0.75).images
    torch.cuda.synchronize()
    return out


def _parent_loop(unet, cn, dev, scale=0.5, end=0.75):
    """The single-ControlNet denoise loop as the engine ran it before the multi path existed, restated eagerly on the
    engine's public pieces: scale folded into the zero convs, 12 + 1 cid_add_inplace_f16 launches inside
    HipUNet.forward_tokens, no scale vector anywhere."""
    from consistentid_amd import ops
    from consistentid_amd.scheduler import DDIMScheduler
    M = _models(str(dev))
    inp, imgs, init, noise, mask = _loop_inputs(M["cfg"])
    d = lambda t: t.to(dev)
    sch = DDIMScheduler()
    sch.set_timesteps(STEPS)
    ts = sch.timesteps
    n = len(ts)
    lat = (d(inp["latents"]).float() * float(sch.init_noise_sigma)).half().contiguous()
    B, per_sample = lat.shape[0], lat[0].numel()
    unet.set_context(torch.cat([d(inp["null"]), d(inp["text"]), d(inp["augmented"])], dim=0))
    cn.set_context(torch.cat([d(inp["text"]), d(inp["augmented"])], dim=0), num_tokens=0)
    coefs = torch.from_numpy(sch.coefficient_table(True)).to(dev).view(n, 5).float()
    tvals = torch.tensor(ts.astype(np.float32), device=dev)
    temb, cn_temb = unet.time_embed_table(tvals), cn.time_embed_table(tvals)
    cond = cn.cond_embedding(d(imgs[0])).clone()
    ar = torch.arange(B, dtype=torch.int32, device=dev)
    mk, i0, nz = d(mask).expand_as(lat).contiguous(), d(init).contiguous(), d(noise).contiguous()
    for i in range(n):
        merged = i > MERGE
        kvrow = torch.cat([ar, ar + (2 * B if merged else B)]).contiguous()
        cn_kvrow = (ar + B if merged else ar).contiguous()
        t_buf, coef = tvals[i:i + 1].clone(), coefs[i].clone()
        dres = mres = None
        if 1.0 - float(i / n < 0.0 or (i + 1) / n > end) > 0.0:
            dres, mres = cn.forward_tokens(lat, t_buf, cn_kvrow, B, cond, scale, temb=cn_temb[i:i + 1].clone(),
                                           in_scale=coef[4:5])
        eps = unet.forward_tokens(lat, t_buf, kvrow, 2 * B, None, dres, mres, temb=temb[i:i + 1].clone(), in_scale=coef[4:5])
        ops.cfg_ddim_step(eps, lat, coef, GUIDANCE, B=B, per_sample=per_sample, mask=mk, init=i0, noise=nz)
    torch.cuda.synchronize()
    return lat


def test_one_net_multi_matches_plain_pipeline_within_the_arm(dev):
    """HipMultiControlNet([net]) applies the scale in cid_residual_accum_f16, the plain HipControlNet in its zero-conv
    weights: not the same bits, both within the fp16 arm of the oracle"""
    from consistentid_amd import pipeline
    from consistentid_amd.controlnet import HipMultiControlNet
    M = _models(str(dev))
    _, imgs, _, _, _ = _loop_inputs(M["cfg"])
    ref, arm = _single_reference(str(dev))
    plain = pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline(M["new_unet"](), controlnet=M["new_cn"](0), use_graph=False)
    multi = pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline(
        M["new_unet"](), controlnet=HipMultiControlNet([M["new_cn"](0)]), use_graph=False)
    check_vs_fp16_arm(_single_call(plain, dev, imgs[0].to(dev)), ref, arm, "plain HipControlNet pipeline")
    check_vs_fp16_arm(_single_call(multi, dev, [imgs[0].to(dev)]), ref, arm, "HipMultiControlNet of one net")
    with pytest.raises(ValueError, match="2 entries for 1 ControlNets"):
        _single_call(multi, dev, [imgs[0].to(dev), imgs[1].to(dev)])
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        _single_call(plain, dev, [imgs[0].to(dev), imgs[1].to(dev)])


@pytest.mark.parametrize("use_graph", [False, True])
def test_plain_controlnet_pipeline_keeps_its_bits(dev, use_graph):
    """the plain HipControlNet pipeline (folded scale, add_inplace launches) against a second engine that never comes near
    the multi path: the same latents, bit for bit, in both generations"""
    from consistentid_amd import pipeline
    M = _models(str(dev))
    _, imgs, _, _, _ = _loop_inputs(M["cfg"])
    want = _parent_loop(M["new_unet"](), M["new_cn"](0), dev)
    pipe = pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline(M["new_unet"](), controlnet=M["new_cn"](0),
                                                                         use_graph=use_graph)
    for gen in range(2):
        got = _single_call(pipe, dev, imgs[0].to(dev))
        assert torch.equal(got, want), f"generation {gen + 1} (graph={use_graph}): {(got.float() - want.float()).abs().max()}"
