"""AutoencoderTiny (TAESD) on the GPU: the three kernels of csrc/taesd.hip against torch, the whole decoder against
tests/taesd_ref.py, its bit-level properties, and ``pipe.vae = HipAutoencoderTiny(...)`` on the pipelines.

Tolerances.  A single kernel accumulates in fp32 and rounds once: max abs error <= 2^-10 max|ref| + 1e-3 (one fp16 rounding
of the largest value, with a factor 2 for the fp32 summation order over K = 576; the form test_gpu_vae.py uses for single
kernels).  The whole decoder is ~30 convolutions deep and has no normalisation, so no fixed number is derivable: its relative
L2 error against the fp32 reference may be at most 2 x that of the SAME reference network with every stored activation
rounded to fp16 (computed here, on the CPU, on the same inputs); the factor 2 covers the kernels' summation order and tanh.
Measured on MI355X (printed by the tests): see DESIGN.md 4.26."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import taesd_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

T_H, T_W, GRID_CAP = 16, 32, 256          # cid_tiny_conv64_f16's output tile and grid cap (test_tile_constants holds them)
SENTINEL = 0x7e5a                         # an fp16 NaN with a payload
PAD = 64


def _rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half()


def _guarded(n, dev):
    return torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)


def _intact(buf, n, what):
    b = buf.view(torch.int16)
    assert bool((b[:PAD] == SENTINEL).all()) and bool((b[PAD + n:] == SENTINEL).all()), f"{what}: wrote outside its output"


def _tok(t):
    """NCHW -> token-major [B, H*W, C]"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous()


def _untok(t, H, W):
    return t.reshape(t.shape[0], H, W, t.shape[2]).permute(0, 3, 1, 2)


def _wtap(w):
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous()


def _check_kernel(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err, bound = float((got - ref).abs().max()), 2.0 ** -10 * float(ref.abs().max()) + 1e-3
    print(f"[taesd] {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e}"


def test_tile_constants(dev):
    from consistentid_amd import ops
    assert ops.tiny_conv64_tile() == (T_H, T_W, GRID_CAP), "the shapes below are chosen for this tile and cap"


# ----------------------------------------------------------------------------- the body kernel
@pytest.fixture(scope="module")
def conv_w():
    w = _rnd(64, 64, 3, 3, seed=11, scale=(2.0 / 576) ** 0.5)
    return w, _rnd(64, seed=12, scale=0.1)


def _run_conv(dev, conv_w, B, H, W, bias, res, relu, up, seed):
    """one launch against F.conv2d in fp32 on the same fp16 values; the output sits between sentinels"""
    from consistentid_amd import ops
    w, b = conv_w
    x = _rnd(B, 64, H, W, seed=seed)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    r = _rnd(B, 64, Ho, Wo, seed=seed + 1) if res else None
    xin = F.interpolate(x.float(), scale_factor=2, mode="nearest") if up else x.float()
    ref = F.conv2d(xin, w.float(), b.float() if bias else None, padding=1)
    if res:
        ref = ref + r.float()
    if relu:
        ref = ref.relu()
    n = B * Ho * Wo * 64
    buf = _guarded(n, dev)
    out = buf[PAD:PAD + n].view(B, Ho * Wo, 64)
    ops.tiny_conv64(_tok(x).to(dev), out, _wtap(w).to(dev), b.to(dev) if bias else None, B=B, H=H, W=W,
                    res=_tok(r).to(dev) if res else None, relu=relu, up=up)
    torch.cuda.synchronize()
    what = f"conv64 B={B} {H}x{W} bias={int(bias)} res={int(res)} relu={int(relu)} up={int(up)}"
    _intact(buf, n, what)
    _check_kernel(_untok(out, Ho, Wo), ref, what)
    return out


SHAPES = [(1, 1), (1, T_W + 1), (T_H + 1, 1), (T_H - 1, T_W - 1), (T_H, T_W), (T_H + 1, T_W + 1), (2 * T_H + 3, T_W - 2)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv64_every_epilogue(dev, conv_w, hw, B):
    """every combination of bias, residual and ReLU at the tile's edges: one pixel, one row / column past a tile, one short
    of it, exactly a tile, one past it in both directions, three tile rows with a ragged last column tile"""
    for k, (bias, res, relu) in enumerate(itertools.product((False, True), repeat=3)):
        _run_conv(dev, conv_w, B, *hw, bias, res, relu, False, seed=100 + k)


# input sizes: odd and even, up to an output of exactly one tile, one input pixel more than that (ragged second tiles), 1 x 1
UP_SHAPES = [(1, 1), (T_H // 2, T_W // 2), (T_H // 2 + 1, T_W // 2 + 1), (5, 7), (T_H + 1, 3)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", UP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv64_through_the_upsample(dev, conv_w, hw, B):
    """``up``: the nearest-2x read, as the net uses it (no bias, no activation) and with every epilogue term on"""
    _run_conv(dev, conv_w, B, *hw, False, False, False, True, seed=200)
    _run_conv(dev, conv_w, B, *hw, True, True, True, True, seed=201)


def test_conv64_more_tiles_than_the_grid(dev, conv_w):
    """3 x 10 x 9 = 270 tiles on at most 256 workgroups: the first 14 workgroups take a second tile (the halo prefetch of a
    tile in another image, the `t + gridDim.x` stride); with ``up`` 4 x 7 x 11 = 308 tiles (odd input sizes)"""
    assert 3 * 10 * 9 > GRID_CAP and 3 * 160 * 288 // (T_H * T_W) == 270
    _run_conv(dev, conv_w, 3, 10 * T_H, 9 * T_W, True, True, True, False, seed=300)
    Hi, Wi = 3 * T_H + 1, 5 * T_W + 7          # output 98 x 334: 7 x 11 tiles per image, 308 for B = 4
    assert 4 * -(-2 * Hi // T_H) * -(-2 * Wi // T_W) == 308 > GRID_CAP
    _run_conv(dev, conv_w, 4, Hi, Wi, False, False, False, True, seed=301)


def test_conv64_is_deterministic(dev, conv_w):
    a = _run_conv(dev, conv_w, 3, 2 * T_H + 3, T_W + 5, True, True, True, False, seed=400).clone()
    b = _run_conv(dev, conv_w, 3, 2 * T_H + 3, T_W + 5, True, True, True, False, seed=400)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ----------------------------------------------------------------------------- the ends
EDGES = [0.0, -0.0, 6.1e-5, -6.1e-5, 3.0, -3.0, 9.0, -9.0, 100.0, -100.0, 65504.0, -65504.0]


def _edge_latents(h, w):
    """every edge value in every channel (and, over the grid, in border and interior positions)"""
    z = torch.zeros(1, 4, h * w)
    for c in range(4):
        for i in range(h * w):
            z[0, c, i] = EDGES[(i + 3 * c) % len(EDGES)]
    return z.view(1, 4, h, w).half()


def _decode_in_ref(z, w, b):
    x = torch.tanh(z.double() / 3) * 3
    return F.conv2d(x, w.double(), b.double(), padding=1).relu()


def _run_decode_in(dev, z, w, b, what):
    from consistentid_amd import ops
    B, _, h, wd = z.shape
    n = B * h * wd * 64
    buf = _guarded(n, dev)
    out = buf[PAD:PAD + n].view(B, h * wd, 64)
    ops.tiny_decode_in(z.to(dev), out, _wtap(w).to(dev), b.to(dev))
    torch.cuda.synchronize()
    _intact(buf, n, what)
    return _untok(out, h, wd)


@pytest.mark.parametrize("shape", [(1, 4, 5, 7), (3, 4, 5, 7), (2, 4, 1, 1), (1, 4, 9, 33)], ids=lambda s: "x".join(map(str, s)))
def test_decode_in_random_latents(dev, shape):
    w, b = _rnd(64, 4, 3, 3, seed=21, scale=(2.0 / 36) ** 0.5), _rnd(64, seed=22, scale=0.1)
    z = (torch.rand(shape, generator=torch.Generator().manual_seed(23)) * 8 - 4).half()
    got = _run_decode_in(dev, z, w, b, f"decode_in {shape}")
    _check_kernel(got, _decode_in_ref(z, w, b), f"decode_in random {shape}")


@pytest.mark.parametrize("hw", [(5, 7), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_in_edge_values(dev, hw):
    """{0, -0, +-6.1e-5, +-3, +-9, +-100, +-65504} in every channel: finite everywhere and within the kernel bound of the
    float64 reference under random weights; then with weights that route tanh(z / 3) * 3 of each input channel straight to an
    output channel (and its negative to another, past the ReLU), where every element must be correct to fp16 -- |z| = 65504
    gives exactly 3, 6.1e-5 comes through as 6.1e-5"""
    h, wd = hw
    z = _edge_latents(h, wd) if h * wd > 1 else None
    w, b = _rnd(64, 4, 3, 3, seed=31, scale=(2.0 / 36) ** 0.5), _rnd(64, seed=32, scale=0.1)
    route = torch.zeros(64, 4, 3, 3)
    for c in range(4):
        route[c, c, 1, 1], route[4 + c, c, 1, 1] = 1.0, -1.0
    zero_b = torch.zeros(64).half()
    cases = [z] if z is not None else [torch.full((1, 4, 1, 1), v).half() for v in EDGES]
    for k, zz in enumerate(cases):
        got = _run_decode_in(dev, zz, w, b, f"decode_in edges {hw}")
        _check_kernel(got, _decode_in_ref(zz, w, b), f"decode_in edges {hw} #{k}")
        got = _run_decode_in(dev, zz, route.half(), zero_b, f"decode_in routed {hw}").double().cpu()
        t = torch.tanh(zz.double() / 3) * 3
        want = torch.cat([t.relu(), (-t).relu()], dim=1)
        assert torch.isfinite(got).all()
        err = (got[:, :8] - want).abs()
        assert bool((err <= 2.0 ** -11 * want.abs() + 2.0 ** -25).all()), f"tanh not correct to fp16: max err {float(err.max()):.3e}"
        assert not got[:, 8:].any()
        big = zz.float().abs() == 65504
        assert bool(((got[:, :4] + got[:, 4:8])[big] == 3.0).all()), "|z| = 65504 must give exactly 3"


def _run_decode_out(dev, x, w, b, H, W, clamp01):
    from consistentid_amd import ops
    B = x.shape[0]
    n = B * 3 * H * W
    buf = _guarded(n, dev)
    # NCHW planes need no 16-byte alignment, but the wrapper asks for an aligned base: PAD keeps it
    out = buf[PAD:PAD + n].view(B, 3, H, W)
    ops.tiny_decode_out(_tok(x).to(dev), out, _wtap(w).to(dev), b.to(dev), clamp01=clamp01)
    torch.cuda.synchronize()
    _intact(buf, n, f"decode_out {H}x{W}")
    return out


@pytest.mark.parametrize("B,hw", [(1, (40, 56)), (3, (40, 56)), (2, (8, 8)), (1, (5, 7)), (2, (1, 1))],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_decode_out_both_modes(dev, B, hw):
    H, W = hw
    x = _rnd(B, 64, H, W, seed=41).relu()                      # what a Block hands on
    w, b = _rnd(3, 64, 3, 3, seed=42, scale=0.06), torch.tensor([0.5, 0.4, 0.6]).half()
    v = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if H * W >= 64:
        assert bool((v < 0).any()) and bool((v > 1).any()) and bool(((v > 0) & (v < 1)).any()), "values must straddle 0 and 1"
    _check_kernel(_run_decode_out(dev, x, w, b, H, W, False), 2 * v - 1, f"decode_out 2x-1 B={B} {H}x{W}")
    got = _run_decode_out(dev, x, w, b, H, W, True)
    _check_kernel(got, v.clamp(0, 1), f"decode_out clamp B={B} {H}x{W}")
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


# ----------------------------------------------------------------------------- the whole decoder
@pytest.fixture(scope="module")
def tiny(dev):
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    model = R.synthetic(0)
    return model, HipAutoencoderTiny(R.config(), model.state_dict(), device=dev)


def _latents(shape, seed=1):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 1.5).half()


def _check_decoder(got, model, z, what, clamp01=False):
    ref = R.decode(model, z.float().cpu(), clamp01=clamp01)
    yard = rel_l2(R.decode(model, z.float().cpu(), fp16_activations=True, clamp01=clamp01), ref)
    err = rel_l2(got.float(), ref)
    print(f"[taesd] {what}: rel_l2 {err:.3e}; the reference with fp16 activations {yard:.3e} -> bound {2 * yard:.3e}")
    assert got.shape == ref.shape and torch.isfinite(got.float()).all()
    assert err <= 2 * yard, f"{what}: rel_l2 {err:.3e} > 2 x {yard:.3e}"


@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (3, 4, 5, 7), (2, 4, 16, 12)], ids=lambda s: "x".join(map(str, s)))
def test_whole_decoder(dev, tiny, shape):
    model, hip = tiny
    z = _latents(shape)
    out = hip.decode_tokens(z.to(dev))
    (dec,) = hip.decode(z.to(dev), return_dict=False)
    img = hip.decode_latents(z.to(dev))
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and out.shape == (shape[0], 3, 8 * shape[2], 8 * shape[3])
    _check_decoder(out, model, z, f"decode_tokens {shape}")
    assert torch.equal(dec, out), "decode(z) is decode_tokens(z): scaling_factor is 1.0"
    _check_decoder(img, model, z, f"decode_latents {shape}", clamp01=True)
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    assert hip.config.scaling_factor == 1.0 and hip.config.latent_channels == 4 and hip.config.force_upcast is False
    assert hip.dtype == torch.float16 and hip.device == dev


def test_other_block_counts(dev):
    """num_decoder_blocks (1, 2): one upsample, x2"""
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    model = R.synthetic(2, (1, 2))
    hip = HipAutoencoderTiny(R.config((1, 2)), model.state_dict(), device=dev)
    z = _latents((2, 4, 9, 6), seed=5)
    out = hip.decode_tokens(z.to(dev))
    assert out.shape == (2, 3, 18, 12)
    _check_decoder(out, model, z, "decode_tokens, blocks (1, 2)")


def test_bit_level_properties(dev, tiny):
    model, hip = tiny
    z = _latents((3, 4, 5, 7), seed=9).to(dev)
    a = hip.decode_tokens(z).clone()
    b = hip.decode_tokens(z)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the same input decoded twice differs"
    for s in range(3):
        one = hip.decode_tokens(z[s:s + 1])
        assert torch.equal(one[0].view(torch.int16), a[s].view(torch.int16)), f"sample {s} of the batch differs from its own decode"


def test_second_call_allocates_nothing(dev, tiny):
    """The intermediate buffers are kept per shape: around a second call of the same shape ``memory_allocated`` does not
    move, and while it runs it rises by the returned image only (the caller owns that tensor; 512-byte allocator blocks)."""
    model, hip = tiny
    z = _latents((2, 4, 16, 12), seed=3).to(dev)
    out = hip.decode_latents(z)
    torch.cuda.synchronize()
    del out
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = hip.decode_latents(z)
    torch.cuda.synchronize()
    image_bytes = -(-out.numel() * 2 // 512) * 512
    assert torch.cuda.memory_allocated(dev) == before + image_bytes
    assert torch.cuda.max_memory_allocated(dev) == before + image_bytes
    del out
    assert torch.cuda.memory_allocated(dev) == before


# ----------------------------------------------------------------------------- pipelines
def _pipeline_call(which, dev):
    """(pipeline class, UNet, keyword arguments without output_type) on the tiny models of engine_cases"""
    import engine_cases as E
    spec = E.Spec(pipe=which, steps=2)
    inp = E.inputs(spec, str(dev))
    d = lambda t: t.to(dev)
    kw = dict(prompt_embeds=d(torch.cat([inp["null"], inp["augmented"], inp["text"]])), latents=d(inp["latents"]),
              num_inference_steps=2, guidance_scale=spec.guidance, start_merge_step=spec.merge)
    if which == "inpaint":
        kw.update(image_latents=d(inp["init"]), noise=d(inp["noise"]), mask_latents=d(inp["mask"]), strength=1.0)
    if which == "sdxl":
        kw.update(pooled_prompt_embeds=inp["pooled_augmented"], pooled_prompt_embeds_text_only=inp["pooled_text"],
                  negative_pooled_prompt_embeds=inp["pooled_null"], add_time_ids=inp["time_ids"])
    return E.pipeline_class(spec), E.new_unet(str(dev), spec.name), kw


def _nchw(images):
    """"pt" of the image_processor pipelines is the [B, 3, H, W] tensor; the SD1.5 pipeline answers every pixel type it does not
    know with NHWC numpy (pipeline._postprocess_checked)"""
    return images if torch.is_tensor(images) else torch.from_numpy(images).permute(0, 3, 1, 2)


def _kl_decoder(which, dev):
    from consistentid_amd import synth, vae_spec
    from consistentid_amd.vae import make_vae_decoder
    cfg = vae_spec.tiny_vae_config()
    if which == "sdxl":                          # the SDXL pipeline's default decoder is the fp32 one (force_upcast)
        cfg = vae_spec.VAEConfig(block_out_channels=(64, 128), layers_per_block=1, scaling_factor=0.13025, force_upcast=True)
    return make_vae_decoder(cfg, synth.random_vae_state_dict(cfg, seed=5, device="cpu"), device=dev)


@pytest.mark.parametrize("which", ["txt2img", "sdxl", "inpaint"])
def test_pipeline_with_the_tiny_decoder(dev, tiny, which):
    """``pipe.vae = HipAutoencoderTiny(...)`` and nothing else: 2 steps, "pt" against taesd_ref on the same call's latents;
    back on the KL decoder the KL image returns bit for bit"""
    model, hip = tiny
    cls, unet, kw = _pipeline_call(which, dev)
    kl = _kl_decoder(which, dev)
    pipe = cls(unet, vae=kl)
    kl_before = _nchw(pipe(output_type="pt", **kw).images).clone()
    pipe.vae = hip
    lat = pipe(output_type="latent", **kw).images
    img = _nchw(pipe(output_type="pt", **kw).images)
    torch.cuda.synchronize()
    B, _, h, w = lat.shape
    assert img.shape == (B, 3, 8 * h, 8 * w)
    _check_decoder(img, model, lat, f"{which} pipeline, output_type=pt", clamp01=True)
    pipe.vae = kl
    kl_after = _nchw(pipe(output_type="pt", **kw).images)
    assert kl_after.dtype == kl_before.dtype and torch.equal(kl_after, kl_before), "the KL decoder's image changed"


def test_safety_checker_still_runs(dev, tiny):
    """a safety checker on the SD1.5 pipeline sees the tiny decoder's images: nsfw_content_detected is filled"""
    import safety_ref
    from consistentid_amd.safety import HipSafetyChecker
    from test_gpu_safety import SMALL
    from transformers import CLIPVisionConfig
    model, hip = tiny
    cls, unet, kw = _pipeline_call("txt2img", dev)
    sd = safety_ref.SafetyCheckerRef(CLIPVisionConfig(**SMALL), seed=5).checkpoint_state_dict()
    vc = {"vision_config": {k: SMALL[k] for k in ("num_attention_heads", "patch_size")}}
    pipe = cls(unet, safety_checker=HipSafetyChecker(vc, sd, device=dev), feature_extractor={"size": SMALL["image_size"]})
    pipe.vae = hip
    r = pipe(output_type="np", **kw)
    assert isinstance(r.nsfw_content_detected, list) and len(r.nsfw_content_detected) == kw["latents"].shape[0]
    assert all(isinstance(f, (bool, np.bool_)) for f in r.nsfw_content_detected)
    assert isinstance(r.images, np.ndarray) and r.images.shape[0] == kw["latents"].shape[0] and np.isfinite(r.images).all()
    assert pipe(output_type="latent", **kw).nsfw_content_detected is None


# ----------------------------------------------------------------------------- the few-step configuration
def few_step_spec():
    """LCM at guidance_scale 1 (the single pass) with one community LoRA merged -- LCM-LoRA on a base model, the configuration
    profiles/lcm_cost.txt and profiles/taesd_cost.txt are about; tests/test_lcm_engine_host.py holds the LoRA to its threshold.
    v-prediction, because the tiny UNet has random weights and is no denoiser: an epsilon LCM step at t = 999 divides by
    sqrt(alphas_cumprod) = 0.07 and the final latents come out at std 16, where the decoder's tanh(z / 3) is +-1 everywhere and
    taesd_ref.decode refuses its own activations (1.1e3 > ACT_LIMIT); the v-prediction latents have std 0.6"""
    import engine_cases as E
    return E.Spec(scheduler="lcm", steps=4, merge=1, guidance=1.0, loras=((11, 1.0),), prediction="v_prediction")


class _AsPixels:
    """``pipe(**kw)`` of engine_cases.call_pipeline with output_type "pt" in place of "latent\""""

    def __init__(self, pipe):
        self.pipe = pipe

    def __call__(self, **kw):
        return self.pipe(**{**kw, "output_type": "pt"})


def test_few_step_configuration(dev, tiny):
    """4-step LCM single pass + LoRA + the tiny decoder on one graph pipeline.  The latents are held like every engine
    scenario (engine_cases.run_scenario: the fresh eager bits, the fp16 arm of the fp32 oracle with the LoRA merged, the step
    launch and the B UNet rows); the image by ``_check_decoder`` on those latents.  Then B = 1 and B = 2 again: the decoder
    releases and rebuilds its per-shape buffers and the engine its static ones, and the third image is the first bit for bit."""
    import engine_cases as E
    model, hip = tiny
    spec = few_step_spec()
    pipe = E.pipeline_class(spec)(E.new_unet(str(dev), keep_base=True), use_graph=True)
    pipe.vae = hip
    (lat,) = E.run_scenario(dev, "few-step configuration", [E.Gen("LCM, LoRA, tiny decoder", spec, oracle=True, guidance_vs=2.0)], pipe)
    images = []
    for B in (2, 1, 2):
        s = spec.but(B=B)
        img = _nchw(E.call_pipeline(_AsPixels(pipe), s, dev)[0]).clone()
        want = lat if B == 2 else E.fresh_eager(s, str(dev))[0]
        assert img.shape == (B, 3, 8 * want.shape[2], 8 * want.shape[3]) and hip._bufs[0][0].shape[0] == B
        _check_decoder(img, model, want, f"few-step configuration, B = {B}, output_type=pt", clamp01=True)
        images.append(img)
    assert pipe._engine.step_path == "multistep" and pipe._engine.captures
    assert torch.equal(images[2], images[0]), "B = 2 after B = 1 gives another image than the first B = 2"
