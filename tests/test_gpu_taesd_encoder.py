"""AutoencoderTiny's encoder on the GPU: the three encoder kernels of csrc/taesd.hip against torch, the whole encoder against
tests/taesd_enc_ref.py, its bit-level properties, and ``pipe.vae_encoder = HipAutoencoderTinyEncoder(...)`` on the inpaint
pipelines.

Tolerances (those of tests/test_gpu_taesd.py).  A single kernel accumulates in fp32 and rounds once: max abs error <= 2^-10
max|ref| + 1e-3 against fp32 ``conv2d`` on the same fp16 values.  The whole encoder is 35 convolutions deep and has no
normalisation: its relative L2 error against the fp32 reference may be at most 2 x that of the SAME reference network with
every stored activation rounded to fp16 (computed beside it, on the CPU, on the same inputs, and printed).  A CPU check supports
the factor 2: on these shapes the yardstick is 0.75e-3 - 1.33e-3 and a second fp16-activation realisation (float64
convolutions, rounded at the same places) lands at 0.94 - 1.04 x it.  Measured on MI355X: DESIGN.md 4.27."""
import pytest
import torch
import torch.nn.functional as F

import taesd_enc_ref as E
from conftest import rel_l2
from test_gpu_taesd import PAD, _check_kernel, _guarded, _intact, _rnd, _tok, _untok, _wtap

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------- encode_in
@pytest.fixture(scope="module")
def head_w():
    return _rnd(64, 3, 3, 3, seed=51, scale=(2.0 / 27) ** 0.5), _rnd(64, seed=52, scale=0.1)


MASK_VALUES = [0.0, 0.3, 0.49999997, 0.5, 0.50000006, 0.8, 1.0]         # both sides of 0.5, and 0.5 itself (= repaint)


def _mask(Bm, H, W, seed):
    idx = torch.randint(0, len(MASK_VALUES), (Bm, 1, H, W), generator=torch.Generator().manual_seed(seed))
    return torch.tensor(MASK_VALUES, dtype=torch.float32)[idx]


def _u_of(image, normalize, keep=None):
    """the kernel's per-pixel semantics in torch: v = half(2x - 1 | x), masked, u = half(v + 1) / 2 in fp16 arithmetic"""
    v = (image * 2 - 1 if normalize else image).half()
    if keep is not None:
        v = v * keep.half()
    return ((v + 1) / 2).float()


def _run_encode_in(dev, image, w, b, mask, normalize, blocks, mask_latents=None):
    from consistentid_amd import ops
    Bi, _, H, W = image.shape
    nb = 2 if blocks == 3 else 1
    n = nb * Bi * H * W * 64
    buf = _guarded(n, dev)
    out = buf[PAD:PAD + n].view(nb * Bi, H * W, 64)
    ops.tiny_encode_in(image.to(dev), out, _wtap(w).to(dev), b.to(dev), mask=None if mask is None else mask.to(dev),
                       normalize=normalize, blocks=blocks, mask_latents=mask_latents)
    torch.cuda.synchronize()
    _intact(buf, n, f"encode_in {tuple(image.shape)} blocks={blocks}")
    return _untok(out, H, W)


@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 5, 7), (1, 3, 9, 33), (2, 3, 16, 24)], ids=lambda s: "x".join(map(str, s)))
def test_encode_in_every_mode(dev, head_w, shape):
    """normalize on / off, one mask for the batch / one per image, blocks 1 / 2 / 3 (the image block first), and no mask"""
    w, b = head_w
    Bi, _, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    unit = torch.rand(shape, generator=g)
    for normalize in (True, False):
        image = unit if normalize else unit * 2 - 1
        for Bm in sorted({1, Bi}):
            mask = _mask(Bm, H, W, seed=Bm)
            keep = (mask < 0.5).expand(Bi, 1, H, W)
            refs = {1: F.conv2d(_u_of(image, normalize), w.float(), b.float(), padding=1),
                    2: F.conv2d(_u_of(image, normalize, keep), w.float(), b.float(), padding=1)}
            for blocks in (1, 2, 3):
                got = _run_encode_in(dev, image, w, b, mask, normalize, blocks)
                ref = torch.cat([refs[k] for k in (1, 2) if blocks & k])
                _check_kernel(got, ref, f"encode_in {shape} normalize={int(normalize)} Bm={Bm} blocks={blocks}")
        got = _run_encode_in(dev, image, w, b, None, normalize, 1)
        _check_kernel(got, refs[1], f"encode_in {shape} normalize={int(normalize)} without a mask")


def test_encode_in_pads_u_not_the_image(dev, head_w):
    """a constant image x = 1 (u = 1): with zero padding of u an outside tap contributes 0, with zero padding of the IMAGE it
    would be u = 0.5.  The two differ at every border pixel by half the sum of the outside taps' weights; a fully masked
    image is u = 0.5 inside and still 0 outside."""
    w, b = head_w
    image = torch.ones(1, 3, 6, 9)
    ones = torch.ones(1, 3, 6, 9)
    pad_u = F.conv2d(ones, w.float(), b.float(), padding=1)
    pad_image = F.conv2d(F.pad(ones, (1, 1, 1, 1), value=0.5), w.float(), b.float())
    border = torch.ones(6, 9, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    gap = (pad_u - pad_image).abs()[0].amax(0)
    bound = 2.0 ** -10 * float(pad_u.abs().max()) + 1e-3
    assert float(gap[border].min()) > 20 * bound and float(gap[~border].max()) < 1e-5, "the case does not separate the two"
    mask = torch.ones(1, 1, 6, 9)
    got = _run_encode_in(dev, image, w, b, mask, False, 3)
    _check_kernel(got[:1], pad_u, "encode_in, x = 1: zero padding of u")
    _check_kernel(got[1:], 0.5 * (pad_u - b.float().view(1, 64, 1, 1)) + b.float().view(1, 64, 1, 1),
                  "encode_in, x = 1 fully masked: u = 0.5 inside, 0 outside")


@pytest.mark.parametrize("Bm", [1, 2])
def test_encode_in_mask_latents(dev, head_w, Bm):
    """bit-equal to F.interpolate(binarised mask, size=(H / 8, W / 8)) (nearest) at 16 x 24, written between sentinels"""
    w, b = head_w
    image = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(7))
    mask = _mask(Bm, 16, 24, seed=70 + Bm)
    mask[:, :, 8, 16] = 0.5                                       # exactly 0.5 at a sampled position: repaint
    mask[:, :, 0, 8] = 0.49999997
    n = Bm * 2 * 3
    buf = _guarded(n, dev)
    ml = buf[PAD:PAD + n].view(Bm, 1, 2, 3)
    _run_encode_in(dev, image, w, b, mask, True, 3, mask_latents=ml)
    _intact(buf, n, "mask_latents")
    want = F.interpolate((mask >= 0.5).float(), size=(2, 3)).half()
    assert torch.equal(ml.cpu(), want) and float(want[0, 0, 1, 2]) == 1.0 and float(want[0, 0, 0, 1]) == 0.0


# ----------------------------------------------------------------------------- the stride-2 convolution
@pytest.fixture(scope="module")
def conv_w():
    return _rnd(64, 64, 3, 3, seed=61, scale=(2.0 / 576) ** 0.5)


def _run_s2(dev, w, B, H, W, seed):
    """one launch against F.conv2d(stride=2, padding=1) in fp32 on the same fp16 values; the output sits between sentinels"""
    from consistentid_amd import ops
    x = _rnd(B, 64, H, W, seed=seed)
    ref = F.conv2d(x.float(), w.float(), None, stride=2, padding=1)
    Ho, Wo = -(-H // 2), -(-W // 2)
    assert ref.shape == (B, 64, Ho, Wo)
    n = B * Ho * Wo * 64
    buf = _guarded(n, dev)
    out = buf[PAD:PAD + n].view(B, Ho * Wo, 64)
    ops.tiny_conv64_s2(_tok(x).to(dev), out, _wtap(w).to(dev), B=B, H=H, W=W)
    torch.cuda.synchronize()
    what = f"conv64_s2 B={B} {H}x{W} -> {Ho}x{Wo}"
    _intact(buf, n, what)
    _check_kernel(_untok(out, Ho, Wo), ref, what)
    return out


# input sizes in terms of the output tile (th, tw): one pixel, the smallest even and odd grids, exactly one output tile, one
# input pixel short of it (odd sizes: the last output reads no right / bottom padding), one more (a second, one-pixel tile
# row and column), and several ragged tile rows beside a short tile column
S2_SHAPES = {"1x1": lambda th, tw: (1, 1), "2x2": lambda th, tw: (2, 2), "3x5": lambda th, tw: (3, 5),
             "tile": lambda th, tw: (2 * th, 2 * tw), "tile-1": lambda th, tw: (2 * th - 1, 2 * tw - 1),
             "tile+1": lambda th, tw: (2 * th + 1, 2 * tw + 1), "ragged": lambda th, tw: (4 * th + 3, 2 * tw - 4)}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(S2_SHAPES))
def test_conv64_s2_at_the_tile_edges(dev, conv_w, name, B):
    from consistentid_amd import ops
    th, tw, _ = ops.tiny_conv64_s2_tile()
    _run_s2(dev, conv_w, B, *S2_SHAPES[name](th, tw), seed=500 + B)


def test_conv64_s2_more_tiles_than_the_grid(dev, conv_w):
    """odd input sizes and more tiles than workgroups (for the 8 x 16 tile and a cap of 256: B = 3, 161 x 287 -> 81 x 144 =
    11 x 9 tiles per image, 297 in all): the first workgroups take a second tile, whose halo is prefetched from another image"""
    from consistentid_amd import ops
    th, tw, cap = ops.tiny_conv64_s2_tile()
    H, W = 2 * (10 * th + 1) - 1, 2 * (9 * tw) - 1
    tiles = 3 * -(-(-(-H // 2)) // th) * -(-(-(-W // 2)) // tw)
    assert tiles > cap and H % 2 and W % 2, (tiles, cap)
    _run_s2(dev, conv_w, 3, H, W, seed=600)


def test_conv64_s2_is_deterministic_and_refuses_aliasing(dev, conv_w):
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    a = _run_s2(dev, conv_w, 3, 37, 45, seed=700).clone()
    b = _run_s2(dev, conv_w, 3, 37, 45, seed=700)
    assert torch.equal(_bits(a), _bits(b))
    x = torch.zeros(1, 1, 64, dtype=torch.float16, device=dev)                    # 1 x 1 -> 1 x 1: the shapes agree
    with pytest.raises(CidError, match="alias"):
        ops.tiny_conv64_s2(x, x, _wtap(conv_w).to(dev), B=1, H=1, W=1)


# ----------------------------------------------------------------------------- encode_out
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("B,hw", [(1, (1, 1)), (3, (5, 7)), (2, (8, 8))], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_encode_out(dev, B, hw, scale):
    from consistentid_amd import ops
    H, W = hw
    x = _rnd(B, 64, H, W, seed=81).relu()                      # what a Block hands on
    w, b = _rnd(4, 64, 3, 3, seed=82, scale=0.06), torch.tensor([0.5, -0.4, 0.1, -0.2]).half()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) * scale
    n = B * 4 * H * W
    buf = _guarded(n, dev)
    out = buf[PAD:PAD + n].view(B, 4, H, W)
    ops.tiny_encode_out(_tok(x).to(dev), out, _wtap(w).to(dev), b.to(dev), scale=scale)
    torch.cuda.synchronize()
    _intact(buf, n, f"encode_out {H}x{W}")
    _check_kernel(out, ref, f"encode_out B={B} {H}x{W} scale={scale}")


# ----------------------------------------------------------------------------- the whole encoder
@pytest.fixture(scope="module")
def tiny(dev):
    from consistentid_amd.vae_tiny import HipAutoencoderTinyEncoder
    model = E.synthetic(0)
    return model, HipAutoencoderTinyEncoder(E.config(), model.state_dict(), device=dev)


def _image(shape, seed=1):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _check_encoder(got, model, x, what):
    ref = E.encode(model, x.float().cpu())
    yard = rel_l2(E.encode(model, x.float().cpu(), fp16_activations=True), ref)
    err = rel_l2(got.float(), ref)
    print(f"[taesd-enc] {what}: rel_l2 {err:.3e}; the reference with fp16 activations {yard:.3e} -> bound {2 * yard:.3e}")
    assert got.shape == ref.shape and got.dtype == torch.float16 and torch.isfinite(got.float()).all()
    assert err <= 2 * yard, f"{what}: rel_l2 {err:.3e} > 2 x {yard:.3e}"


@pytest.mark.parametrize("shape", [(32, 3, 8, 8), (3, 3, 40, 56), (2, 3, 23, 37)], ids=lambda s: "x".join(map(str, s)))
def test_whole_encoder(dev, tiny, shape):
    """8 x 8 -> 1 x 1 latents (every deep conv sees mostly padding), 40 x 56 -> 5 x 7, 23 x 37 -> 3 x 5 (odd at every level)"""
    model, hip = tiny
    x = _image(shape)
    out = hip.encode(x.to(dev))
    (lat,) = hip.encode(x.to(dev), return_dict=False)
    torch.cuda.synchronize()
    B, _, H, W = shape
    assert out.latents.shape == (B, 4, -(-H // 8), -(-W // 8))
    _check_encoder(out.latents, model, x, f"encode {shape}")
    assert torch.equal(_bits(lat), _bits(out.latents))
    assert hip.config.scaling_factor == 1.0 and hip.config.latent_channels == 4 and hip.config.force_upcast is False
    assert hip.dtype == torch.float16 and hip.device == dev and hip.downscale == 8


def test_encode_inpaint_against_the_reference(dev, tiny):
    """[2, 3, 16, 24] in [0, 1] with a per-image mask: the reference is fed x and x * (mask < 0.5)"""
    model, hip = tiny
    image = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(4))
    mask = _mask(2, 16, 24, seed=5)
    r = hip.encode_inpaint(image.to(dev), mask.to(dev), normalize=True, eps_image=torch.zeros(2, 4, 2, 3), eps_masked=None)
    torch.cuda.synchronize()
    x = (image * 2 - 1).half()
    _check_encoder(r["image_latents"], model, x, "encode_inpaint image_latents")
    _check_encoder(r["masked_image_latents"], model, x * (mask < 0.5).half(), "encode_inpaint masked_image_latents")
    assert torch.equal(r["mask_latents"].cpu(), F.interpolate((mask >= 0.5).float(), size=(2, 3)).half())
    only = hip.encode_inpaint(image.to(dev), mask[:1].to(dev), normalize=True, encode_image=False)
    assert only["image_latents"] is None and only["mask_latents"].shape == (1, 1, 2, 3)
    _check_encoder(only["masked_image_latents"], model, x * (mask[:1] < 0.5).half(), "encode_inpaint, masked image only, Bm = 1")
    with pytest.raises(ValueError, match="multiples of 8"):
        hip.encode_inpaint(image[..., :20].to(dev), mask[..., :20].to(dev))


def test_other_block_counts(dev):
    """num_encoder_blocks (1, 2): one stride-2 conv, / 2 -- ``encode`` works, ``encode_inpaint`` refuses (it needs / 8)"""
    from consistentid_amd.vae_tiny import HipAutoencoderTinyEncoder
    model = E.synthetic(2, (1, 2))
    hip = HipAutoencoderTinyEncoder(E.config((1, 2)), model.state_dict(), device=dev)
    x = _image((2, 3, 9, 6), seed=5)
    out = hip.encode(x.to(dev)).latents
    assert out.shape == (2, 4, 5, 3) and hip.downscale == 2
    _check_encoder(out, model, x, "encode, blocks (1, 2)")
    with pytest.raises(ValueError, match="downsamples by 2"):
        hip.encode_inpaint(torch.rand(1, 3, 16, 16, device=dev), torch.zeros(1, 1, 16, 16, device=dev))


def test_bit_level_properties(dev, tiny):
    model, hip = tiny
    x = _image((3, 3, 24, 40), seed=9).to(dev)
    a = hip.encode(x).latents.clone()
    b = hip.encode(x).latents
    assert torch.equal(_bits(a), _bits(b)), "the same input encoded twice differs"
    for s in range(3):
        one = hip.encode(x[s:s + 1]).latents
        assert torch.equal(_bits(one[0]), _bits(a[s])), f"sample {s} of the batch differs from its own encode"
    mask = _mask(1, 24, 40, seed=3).to(dev)
    r = hip.encode_inpaint(x, mask, normalize=False)              # both blocks in one pass; scaling_factor is 1.0
    assert torch.equal(_bits(r["image_latents"]), _bits(a)), "image_latents of the two-block pass differ from encode(x)"
    assert not torch.equal(_bits(r["masked_image_latents"]), _bits(a))


def test_second_call_allocates_only_what_it_returns(dev, tiny):
    """The intermediate buffers are kept per shape: around a second call of the same shape ``memory_allocated`` rises by the
    returned tensors only, also at the peak (512-byte allocator blocks; fp32 device inputs are read where they are)."""
    model, hip = tiny
    x = _image((2, 3, 32, 24), seed=3).to(dev)
    mask = torch.zeros(2, 1, 32, 24, device=dev)
    blk = lambda n: -(-n * 2 // 512) * 512
    for call, returned in ((lambda: hip.encode(x), blk(2 * 4 * 4 * 3)),
                           (lambda: hip.encode_inpaint(x, mask, normalize=False), blk(4 * 4 * 4 * 3) + blk(2 * 4 * 3))):
        out = call()
        torch.cuda.synchronize()
        del out
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = call()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(dev) == before + returned
        assert torch.cuda.max_memory_allocated(dev) == before + returned
        del out
        assert torch.cuda.memory_allocated(dev) == before


# ----------------------------------------------------------------------------- pipelines
@pytest.mark.parametrize("kind", ["four", "nine", "controlnet"])
def test_inpaint_pipeline_with_the_tiny_encoder(dev, tiny, kind):
    """``vae_encoder=<tiny encoder>``: pipe(image=, mask_image=, generator=seed) equals, bit for bit, the same pipeline called
    with the explicit tensors built from ``encode_inpaint`` and the replayed draws (eps, noise, eps in ``inpaint_draws``'
    order; the eps are drawn and unused); two calls with one seed agree; the KL encoder swapped in and out returns its own
    result; ``pipe.vae = <tiny decoder>`` leaves the encoder alone"""
    import taesd_ref as R
    from consistentid_amd import pipeline, synth
    from consistentid_amd.unet import HipUNet
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    from oracle_utils import make_weights
    from test_gpu_vae_encode import _vae
    model, enc = tiny
    kl = _vae(dev, "small")[2]
    in_ch = 9 if kind == "nine" else 4
    cfg, sd, ad = make_weights("tiny", rank=8, in_channels=in_ch)
    unet = HipUNet(cfg, sd, ad, device=dev)
    B, Bi, side, steps = 2, 1, 128, 3
    h8 = side // 8
    strength = 0.6 if kind == "nine" else 1.0
    inp = synth.random_inputs(make_weights("tiny")[0], B, side, side)
    image = torch.rand(Bi, 3, side, side, generator=torch.Generator().manual_seed(21))
    mask = torch.zeros(Bi, 1, side, side)
    mask[:, :, 32:96, 40:104] = 0.8
    pe = torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev)
    kw = dict(prompt_embeds=pe, num_inference_steps=steps, guidance_scale=7.5, start_merge_step=1, strength=strength,
              output_type="latent")
    if kind == "controlnet":
        shapes = [(64, 16), (64, 16), (64, 8), (128, 8), (128, 4), (128, 4)]
        rr = torch.Generator().manual_seed(11)
        dres = [(torch.randn(B, c, s, s, generator=rr) * 0.1).half() for c, s in shapes]
        mres = (torch.randn(B, 128, 4, 4, generator=rr) * 0.1).half()
        kw.update(down_block_res_samples=[_tok(t).to(dev) for t in dres], mid_block_res_sample=_tok(mres).to(dev))
    cls = (pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline if kind == "controlnet"
           else pipeline.StableDiffusionInpaintConsistentIDPipeline)
    pipe = cls(unet, vae_encoder=enc)
    call = lambda: pipe(image=image.to(dev), mask_image=mask.to(dev), generator=torch.Generator().manual_seed(1234),
                        **kw).images.clone()
    got = call()
    # the explicit tensors: one encoder pass, and the draws replayed -- eps(image) [4-channel UNet, or strength < 1], noise, eps(masked)
    r = torch.Generator().manual_seed(1234)
    draw = lambda *shape: torch.randn(shape, generator=r, dtype=torch.float16)
    draw(Bi, 4, h8, h8)
    noise = draw(B, 4, h8, h8)
    draw(Bi, 4, h8, h8)
    e = enc.encode_inpaint(image.to(dev), mask.to(dev), normalize=True, encode_image=True, encode_masked=kind == "nine")
    rep = lambda t: None if t is None else t.repeat(B // t.shape[0], 1, 1, 1)
    assert (e["masked_image_latents"] is None) == (kind != "nine")
    explicit = pipe(image_latents=rep(e["image_latents"]), noise=noise.to(dev), mask_latents=rep(e["mask_latents"]),
                    masked_image_latents=rep(e["masked_image_latents"]), **kw).images.clone()
    torch.cuda.synchronize()
    assert got.shape == (B, 4, h8, h8) and torch.isfinite(got.float()).all()
    assert torch.equal(_bits(got), _bits(explicit)), "image= / mask_image= differs from the explicit latents"
    pipe.vae_encoder = kl
    kl_first = call()
    assert not torch.equal(kl_first, got), "the KL encoder gives other latents than the tiny one"
    pipe.vae_encoder = enc
    pipe.vae = HipAutoencoderTiny(R.config(), R.synthetic(0).state_dict(), device=dev)
    assert pipe.vae_encoder is enc, "pipe.vae = <tiny decoder> replaced the encoder"
    assert torch.equal(_bits(call()), _bits(got)), "two calls with one seed differ"
    pipe.vae_encoder = kl
    assert torch.equal(_bits(call()), _bits(kl_first)), "the KL encoder's result changed"
