"""The safety checker on the GPU: cid_clip_head_f16 against an fp64 evaluation of the same fp16 inputs and the Python
threshold loop, cid_blackout_f16, the quick-GELU vision tower and ``image_embeds`` against transformers, HipSafetyChecker
end to end against tests/safety_ref.py, and the SD1.5 / inpaint pipelines filling ``nsfw_content_detected``.

Decisions are compared exactly.  Their thresholds come from the REFERENCE's cosines, placed so that image 0's scores sit
0.005 either side of zero; every test first asserts that all B x K reference scores are at least 0.003 away from the
rounding boundary 0.0005 -- more than ten times the cosine error of an fp16 tower (measured 6.6e-4 relative on cosines
below 0.27 for the toy tower: 1.7e-4 absolute; the stock-fp16 arm is at 1.0e-3)."""
import numpy as np
import pytest
import torch

import safety_ref
from conftest import check_close, check_vs_fp16_arm, half_arm

pytestmark = pytest.mark.gpu

SMALL = safety_ref.SMALL
VIT_L = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
             patch_size=14, projection_dim=768)


# ------------------------------------------------------------------------------------------------------------ head kernel
def _run_head(dev, case, thresholds=None, embeds=True):
    from consistentid_amd import ops
    d = lambda t: None if t is None else t.to(dev)
    out = torch.empty(case["B"], case["P"], dtype=torch.float16, device=dev) if embeds else None
    thr = None if thresholds is None else torch.from_numpy(np.asarray(thresholds, np.float32)).to(dev)
    r = ops.clip_head(d(case["x"]), d(case["gamma"]), d(case["beta"]), d(case["w"]), B=case["B"], ldx=case["ldx"],
                      eps=safety_ref.HEAD_EPS, concepts=d(case["concepts"]) if thr is not None else None, thresholds=thr,
                      n_special=case["n_special"], embeds=out)
    torch.cuda.synchronize()
    return r, out


@pytest.mark.parametrize("name", list(safety_ref.HEAD_CASES))
def test_clip_head(dev, name):
    case = safety_ref.head_inputs(name)
    e_ref, cos_ref = safety_ref.head_ref64(case)
    K, ns = case["K"], case["n_special"]
    if K == 0:
        got, out = _run_head(dev, case)
        assert got is out
        check_close(out, e_ref, f"clip_head {name} embeds")
        return
    cos32 = cos_ref.numpy().astype(np.float32)
    first = True
    for dname, margins in safety_ref.decision_cases(K, ns).items():
        thr = safety_ref.thresholds_for(cos32[0], margins)
        s_ref, hits_ref, flags_ref = safety_ref.decide(cos32, thr, ns)
        safety_ref.assert_clear_of_boundary(s_ref)                       # all B x K entries, before anything is compared
        assert np.array_equal(hits_ref[0], safety_ref.expected_hits0(dname, K, ns))
        (cos, scores, flags), out = _run_head(dev, case, thr, embeds=first)
        if first:                                                        # embeds / cos do not depend on the thresholds
            check_close(out, e_ref, f"clip_head {name} embeds")
            check_close(cos, cos_ref, f"clip_head {name} cos")
            first = False
        scores = scores.cpu().numpy()
        print(f"[safety] clip_head {name} {dname}: max |score - ref| = {np.abs(scores - s_ref).max():.2e}")
        hits = np.rint(scores * np.float32(1000.0)) >= 1                 # the kernel's own test, on the scores it stored
        assert np.array_equal(hits, hits_ref), (name, dname, scores, s_ref)
        assert flags.cpu().tolist() == [int(f) for f in flags_ref], (name, dname)
        # fp32 sums of at most 1024 products of O(1) terms against fp64: a few 1e-7; 1e-5 is 300 times below the clearance
        assert np.abs(scores - s_ref).max() < 1e-5


# --------------------------------------------------------------------------------------------------------------- blackout
@pytest.mark.parametrize("per_image", [300, 1152, 7])
def test_blackout(dev, per_image):
    """300 (% 8 == 4): the 2-byte path; 1152 = 8 * 144: the 16-byte path; 7: less than one vector"""
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(per_image)
    x = (torch.randn(3, per_image, generator=g) + 3).half()
    y = x.to(dev)
    assert ops.blackout_(y, torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)) is y
    torch.cuda.synchronize()
    y = y.cpu()
    assert not y[1].any() and torch.equal(y[0], x[0]) and torch.equal(y[2], x[2])


def test_blackout_unaligned_base(dev):
    """per_image % 8 == 0 on a base that is only 2-byte aligned: the 2-byte path, and nothing outside the images is written"""
    from consistentid_amd import ops
    keep = (torch.randn(1 + 3 * 304 + 1, generator=torch.Generator().manual_seed(1)) + 3).half()
    buf = keep.to(dev)
    view = buf[1:-1].view(3, 304)
    assert view.data_ptr() % 16 == 2
    ops.blackout_(view, torch.tensor([1, 0, 1], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    got, want = buf.cpu(), keep.clone()
    want[1:-1].view(3, 304)[[0, 2]] = 0
    assert torch.equal(got, want)


def test_checker_blacks_out_numpy_and_tensor(dev):
    """HipSafetyChecker.__call__: the device tensor in place by the kernel, a numpy array / a list of arrays on the host"""
    chk, ref, clip_input, thr = _small_checker(dev, "concept_hit_image1")
    imgs = (torch.rand(2, 3, 10, 30, generator=torch.Generator().manual_seed(2)) + 0.1).half()
    t = imgs.to(dev)
    out, has = chk(clip_input=clip_input, images=t)
    assert out is t and has == [False, True]
    assert not t[1].any() and torch.equal(t[0].cpu(), imgs[0])
    arr = imgs.float().permute(0, 2, 3, 1).numpy().copy()
    out, has = chk(clip_input, arr)
    assert out is arr and has == [False, True] and not arr[1].any() and np.array_equal(arr[0], imgs[0].float().permute(1, 2, 0).numpy())
    lst = [a.copy() for a in imgs.float().permute(0, 2, 3, 1).numpy()]
    out, has = chk(clip_input, lst)
    assert has == [False, True] and not out[1].any() and out[1].shape == (10, 30, 3) and out[0].any()
    f32 = imgs.float().to(dev)                                           # not fp16: zeroed from the host list, like diffusers
    out, has = chk(clip_input, f32)
    assert has == [False, True] and not out[1].any() and torch.equal(out[0].cpu(), imgs[0].float())


# ------------------------------------------------------------------------------------------------------------------ tower
@pytest.mark.parametrize("name", ["small", "vit_l"])
def test_quick_gelu_tower_and_image_embeds(dev, name):
    """HipCLIPVision(hidden_act="quick_gelu"): hidden_states(-1) and image_embeds against transformers'
    CLIPVisionModelWithProjection on random weights -- the toy tower and the ViT-L/14 geometry of the safety checker"""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from consistentid_amd.clip_vision import HipCLIPVision
    cfg = CLIPVisionConfig(hidden_act="quick_gelu", **(SMALL if name == "small" else VIT_L))
    torch.manual_seed(3)
    ref = CLIPVisionModelWithProjection(cfg).eval()
    with torch.no_grad():
        for _, p in ref.named_parameters():
            if p.ndim == 1:
                p.add_(torch.randn_like(p) * 0.05)
            p.copy_(p.half().float())
    hip = HipCLIPVision(ref.state_dict(), num_heads=cfg.num_attention_heads, patch_size=cfg.patch_size, device=dev,
                        hidden_act="quick_gelu")
    B = 2 if name == "small" else 1
    img = torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(4)).half()
    with torch.no_grad():
        o = ref(img.float(), output_hidden_states=True)
        a = half_arm(ref, dev)(img.to(dev), output_hidden_states=True)
    hs = hip.hidden_states(img.to(dev), -1)
    emb = hip.image_embeds(img.to(dev))
    torch.cuda.synchronize()
    assert hs.shape == o.hidden_states[-1].shape and emb.shape == o.image_embeds.shape and emb.dtype == torch.float16
    check_vs_fp16_arm(hs, o.hidden_states[-1], a.hidden_states[-1], f"CLIP vision quick_gelu {name} hidden_states[-1]")
    check_vs_fp16_arm(emb, o.image_embeds, a.image_embeds, f"CLIP vision quick_gelu {name} image_embeds")
    if name == "small":                 # the activation is really the other one
        gelu = HipCLIPVision(ref.state_dict(), num_heads=cfg.num_attention_heads, patch_size=cfg.patch_size, device=dev)
        assert not torch.equal(gelu.hidden_states(img.to(dev), -1), hs)
        with pytest.raises(NotImplementedError):
            HipCLIPVision(ref.state_dict(), num_heads=2, device=dev, hidden_act="relu")


# ----------------------------------------------------------------------------------------------------- checker end to end
_small_ref = safety_ref.small_ref


def _small_checker(dev, dname):
    """HipSafetyChecker of the toy reference with the thresholds of one decision case (built from the reference cosines)"""
    from consistentid_amd.safety import HipSafetyChecker
    ref, x, cos = _small_ref()
    K, ns = cos.shape[1], safety_ref.N_SPECIAL
    if dname == "concept_hit_image1":               # image 1 hits concept column ns, image 0 does not: [False, True]
        k = ns + int(np.argmax(cos[1, ns:] - cos[0, ns:]))
        gap = float(cos[1, k] - cos[0, k])
        assert gap >= 0.008, f"the toy images' cosines differ by {gap:.4f} at most: pick other seeds"
        thr = np.full(K, 2.0, np.float32)
        thr[k] = np.float32((float(cos[1, k]) + float(cos[0, k])) / 2)
    else:
        thr = safety_ref.thresholds_for(cos[0], safety_ref.decision_cases(K, ns)[dname])
    sd = ref.checkpoint_state_dict()
    sd["special_care_embeds_weights"], sd["concept_embeds_weights"] = torch.from_numpy(thr[:ns].copy()), torch.from_numpy(thr[ns:].copy())
    chk = HipSafetyChecker({"vision_config": {k: SMALL[k] for k in ("num_attention_heads", "patch_size")}}, sd, device=dev)
    return chk, ref, x.to(dev), thr


def test_checker_cosines_and_decisions(dev):
    ref, x, cos_ref = _small_ref()
    K, ns = cos_ref.shape[1], safety_ref.N_SPECIAL
    arm = half_arm(ref, dev).cosines(x.to(dev).half())
    printed = False
    for dname in safety_ref.decision_cases(K, ns):
        chk, _, xin, thr = _small_checker(dev, dname)
        s_ref, hits_ref, flags_ref = safety_ref.decide(cos_ref, thr, ns)
        safety_ref.assert_clear_of_boundary(s_ref)
        cos, scores, flags = chk.cosines(xin)
        torch.cuda.synchronize()
        if not printed:
            e2, e_arm = check_vs_fp16_arm(cos, torch.from_numpy(cos_ref), arm, "safety checker cosines (toy tower)")
            print(f"[safety] cosine error vs the fp32 reference: HIP {e2:.2e}, stock-fp16 arm {e_arm:.2e}; "
                  f"largest |cos| {np.abs(cos_ref).max():.3f}")
            printed = True
        hits = np.rint(scores.cpu().numpy() * np.float32(1000.0)) >= 1
        assert np.array_equal(hits, hits_ref), (dname, scores.cpu().numpy(), s_ref)
        assert flags.cpu().tolist() == [int(f) for f in flags_ref], dname
        _, has = chk(xin, np.ones((2, 4, 4, 3), np.float32))
        assert has == [bool(f) for f in flags_ref]


# --------------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def engines(dev):
    from consistentid_amd import synth, vae_spec
    from consistentid_amd.unet import HipUNet
    from consistentid_amd.vae import HipVAEDecoder
    from oracle_utils import make_weights
    vcfg = vae_spec.tiny_vae_config()
    vae = HipVAEDecoder(vcfg, synth.random_vae_state_dict(vcfg, seed=5), device=dev)
    cfg, sd, ad = make_weights("tiny", rank=8)
    unet = HipUNet(cfg, sd, ad, device=dev)
    inp = synth.random_inputs(cfg, 2, cfg.sample_size * 8, cfg.sample_size * 8)
    kw = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev), latents=inp["latents"].to(dev),
              num_inference_steps=2, guidance_scale=5.0, start_merge_step=1)
    return unet, vae, kw


def _as_array(images):
    """any output_type -> float NHWC numpy (PIL: / 255)"""
    if torch.is_tensor(images):
        return images.float().permute(0, 2, 3, 1).cpu().numpy()
    if isinstance(images, list):
        return np.stack([np.asarray(p) for p in images]).astype(np.float32) / 255
    return images


@pytest.mark.parametrize("which", ["sd15", "inpaint"])
def test_pipeline_fills_nsfw_content_detected(dev, engines, which):
    """A checker crafted from the cosines of the unchecked run's own images flags exactly the second of two images: the
    field is [False, True], the flagged image is black and the other one bit-identical for every pixel output type;
    latents are never checked; without a checker everything is as before."""
    from consistentid_amd import pipeline
    from consistentid_amd.face_prep import clip_preprocess
    from consistentid_amd.safety import HipSafetyChecker
    from transformers import CLIPVisionConfig
    unet, vae, kw = engines
    cls = pipeline.ConsistentIDStableDiffusionPipeline if which == "sd15" else pipeline.StableDiffusionInpaintConsistentIDPipeline
    types = ("pil", "np", "pt")
    plain = cls(unet, vae=vae, safety_checker=None)
    base = {}
    for ot in types + ("latent",):
        r = plain(output_type=ot, **kw)
        assert r.nsfw_content_detected is None
        base[ot] = r.images.clone() if torch.is_tensor(r.images) else r.images
    assert plain(output_type="np", return_dict=False, **kw)[1] is None
    # the checker: toy tower, thresholds from the cosines of these two images
    ref = safety_ref.SafetyCheckerRef(CLIPVisionConfig(**SMALL), seed=5)
    sd = ref.checkpoint_state_dict()
    vc = {"vision_config": {k: SMALL[k] for k in ("num_attention_heads", "patch_size")}}
    probe = HipSafetyChecker(vc, sd, device=dev)
    pil = plain._numpy_to_pil(_as_array(base["np"]))
    clip_input = torch.from_numpy(np.stack([clip_preprocess(p, probe.image_size) for p in pil]))
    cos = probe.cosines(clip_input)[0].cpu().numpy()
    ns = safety_ref.N_SPECIAL
    k = ns + int(np.argmax(cos[1, ns:] - cos[0, ns:]))
    gap = float(cos[1, k] - cos[0, k])
    print(f"[safety] pipeline {which}: cosine gap between the two images at concept {k - ns}: {gap:.4f}")
    assert gap >= 0.008, "the two generated images are too alike for this checker: pick other seeds"
    thr = np.full(cos.shape[1], 2.0, np.float32)
    thr[k] = np.float32((float(cos[1, k]) + float(cos[0, k])) / 2)
    sd["special_care_embeds_weights"], sd["concept_embeds_weights"] = torch.from_numpy(thr[:ns].copy()), torch.from_numpy(thr[ns:].copy())
    checked = cls(unet, vae=vae, safety_checker=HipSafetyChecker(vc, sd, device=dev), feature_extractor={"size": SMALL["image_size"]})
    for ot in types:
        r = checked(output_type=ot, **kw)
        assert r.nsfw_content_detected == [False, True], ot
        got, want = _as_array(r.images), _as_array(base[ot])
        assert type(r.images) is type(base[ot]) and got.shape == want.shape
        assert not got[1].any(), f"{ot}: the flagged image is not black"
        assert np.array_equal(got[0], want[0]), f"{ot}: the unflagged image changed"
    images, nsfw = checked(output_type="np", return_dict=False, **kw)
    assert nsfw == [False, True] and not images[1].any()
    r = checked(output_type="latent", **kw)
    assert r.nsfw_content_detected is None and torch.equal(r.images, base["latent"])
