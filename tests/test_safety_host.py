"""Safety checker, host side (no GPU): the C ABI of csrc/safety.hip refuses bad arguments before any launch, the header,
the exports and the ctypes table agree, the decision formula of the kernel is the Python loop's, the test cases of
test_gpu_safety.py clear the rounding boundary, and loader.py / safety.py read a checker folder the way diffusers means
its keywords."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import safety_ref

ROOT = Path(__file__).resolve().parents[1]
SMALL = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=70,
             patch_size=14, projection_dim=64)
CLIP_PRE = {"crop_size": 224, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True, "do_resize": True,
            "feature_extractor_type": "CLIPFeatureExtractor", "image_mean": [0.48145466, 0.4578275, 0.40821073],
            "image_std": [0.26862954, 0.26130258, 0.27577711], "resample": 3, "size": 224}     # the SD1.5 base model's file


def test_header_exports_and_bindings_agree(lib):
    from consistentid_amd import _lib
    names = set(re.findall(r"\b(cid_[a-z0-9_]+)\s*\(", (ROOT / "include" / "cid.h").read_text()))
    assert {"cid_clip_head_f16", "cid_blackout_f16"} <= names
    assert names == set(_lib.SIGNATURES)
    for n in names:
        assert hasattr(lib, n), f"libcid.so does not export {n}"
    assert lib.cid_version() >= 107


def test_clip_head_refusals_without_gpu(lib):
    err = lib.cid_last_error
    A = 64        # a 16-byte-aligned stand-in address: every call below is refused before anything is launched

    def head(x=A, ldx=128, g=A, b=A, w=A, con=A, thr=A, B=1, C=128, P=64, K=5, ns=2, emb=A, cos=A, sc=A, fl=A):
        return lib.cid_clip_head_f16(x, ldx, g, b, 1e-5, w, con, thr, B, C, P, K, ns, emb, cos, sc, fl, None)

    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(w=None)):
        assert head(**kw) == -22 and b"null pointer" in err(), kw
    for kw in (dict(con=None), dict(thr=None), dict(cos=None), dict(sc=None), dict(fl=None)):
        assert head(**kw) == -22 and b"required with K > 0" in err(), kw
    assert head(K=0, ns=0, con=None, thr=None, cos=None, sc=None, fl=None, emb=None) == -22 and b"K == 0 without embeds" in err()
    assert head(C=124, ldx=128) == -22 and b"C must be a multiple of 8" in err()
    assert head(C=4104, ldx=4104) == -22 and b"at most 4096" in err()
    assert head(P=60) == -22 and b"P must be a multiple of 8" in err()
    assert head(ldx=132) == -22 and b"ldx must be a multiple of 8" in err()
    assert head(ldx=120) == -22 and b"at least C" in err()
    assert head(K=65) == -22 and b"K must be in [0, 64]" in err()
    assert head(K=5, ns=6) == -22 and b"n_special must be in [0, K]" in err()
    assert head(ns=-1) == -22
    for B in (0, -3):
        assert head(B=B) == -22 and b"B must be positive" in err()
    assert head(x=A + 2) == -22 and b"16-byte aligned" in err()
    assert head(w=A + 8) == -22 and b"16-byte aligned" in err()
    assert lib.cid_blackout_f16(None, A, 1, 8, None) == -22 and b"null pointer" in err()
    assert lib.cid_blackout_f16(A, None, 1, 8, None) == -22
    assert lib.cid_blackout_f16(A, A, 0, 8, None) == -22 and b"per_image at least 1" in err()
    assert lib.cid_blackout_f16(A, A, 1, 0, None) == -22
    assert lib.cid_blackout_f16(A + 1, A, 1, 3, None) == -22 and b"2-byte aligned" in err()


def test_python_front_end_refuses_cpu_tensors(lib):
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    x = torch.zeros(2, 128, dtype=torch.float16)
    with pytest.raises(CidError):
        ops.clip_head(x, x[0], x[0], torch.zeros(64, 128, dtype=torch.float16), B=2, ldx=128, embeds=torch.zeros(2, 64).half())
    with pytest.raises(CidError):
        ops.blackout_(x, torch.zeros(2, dtype=torch.int32))


def test_kernel_decision_formula_is_pythons_round():
    """the kernel tests rintf(s * 1000.f) >= 1.f; the checker tests round(np.float32, 3) > 0.  Same answer on a fine float32
    grid around zero, at the half-even tie (0.0005 -> 0.0) and at the neighbours of every tie."""
    ties = np.arange(-20, 21, dtype=np.float64) * 1e-3 + 5e-4
    grid = np.concatenate([np.linspace(-0.02, 0.02, 40001), ties, [0.0, -0.0, 0.0005, 0.0015, 0.00049999, 0.00050001, 1.0, -1.0]])
    s = grid.astype(np.float32)
    s = np.unique(np.concatenate([s, np.nextafter(s, np.float32(1)), np.nextafter(s, np.float32(-1))]))
    kernel = np.rint(s * np.float32(1000.0)) >= np.float32(1.0)
    python = np.array([round(v, 3) > 0 for v in s])
    assert type(round(s[0], 3)) is np.float32
    assert np.array_equal(kernel, python), s[kernel != python][:8]
    assert not (round(np.float32(0.0005), 3) > 0) and (round(np.float32(0.0015), 3) > 0)


def test_decide_restates_the_special_care_adjustment():
    cos = np.zeros((1, 5), np.float32)
    for name, margins in safety_ref.decision_cases(5, 3).items():
        scores, hits, flags = safety_ref.decide(cos, safety_ref.thresholds_for(cos[0], margins), 3)
        assert np.array_equal(hits[0], safety_ref.expected_hits0(name, 5, 3)), name
        assert bool(flags[0]) == (name in ("concept_hit", "special_lifts_concept")), name
        safety_ref.assert_clear_of_boundary(scores)


@pytest.mark.parametrize("name", [n for n, c in safety_ref.HEAD_CASES.items() if c[3]])
def test_head_cases_clear_the_rounding_boundary(name):
    """every one of the B x K reference scores of every decision case of test_gpu_safety.py lies >= 0.003 from 0.0005 (the
    thresholds come from image 0, so the other images' scores are wherever the seed puts them), and image 0 hits what the
    case is built to hit"""
    case = safety_ref.head_inputs(name)
    _, cos = safety_ref.head_ref64(case)
    cos = cos.numpy().astype(np.float32)
    K, ns = case["K"], case["n_special"]
    cases = safety_ref.decision_cases(K, ns)
    assert ("special_1_lifts_2_not_0" in cases) == (ns >= 3)
    for dname, margins in cases.items():
        scores, hits, _ = safety_ref.decide(cos, safety_ref.thresholds_for(cos[0], margins), ns)
        safety_ref.assert_clear_of_boundary(scores)
        assert np.array_equal(hits[0], safety_ref.expected_hits0(dname, K, ns)), (name, dname)


def test_end_to_end_cases_clear_the_rounding_boundary():
    """the same for the toy checker of test_gpu_safety.py: both images, all 20 columns, every decision case"""
    _, _, cos = safety_ref.small_ref()
    ns = safety_ref.N_SPECIAL
    for dname, margins in safety_ref.decision_cases(cos.shape[1], ns).items():
        scores, hits, _ = safety_ref.decide(cos, safety_ref.thresholds_for(cos[0], margins), ns)
        safety_ref.assert_clear_of_boundary(scores)
        assert np.array_equal(hits[0], safety_ref.expected_hits0(dname, cos.shape[1], ns)), dname
    assert float((cos[1, ns:] - cos[0, ns:]).max()) >= 0.008          # room for a threshold between the two images


# ------------------------------------------------------------------------------------------------------ loader / safety.py
def _checker_ref(seed=0):
    from transformers import CLIPVisionConfig
    return safety_ref.SafetyCheckerRef(CLIPVisionConfig(**SMALL), seed=seed)


def _write_checker(root, ref, vision_config):
    from safetensors.torch import save_file
    d = root / "safety_checker"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({"_class_name": "StableDiffusionSafetyChecker", "projection_dim": 64,
                                               "vision_config": vision_config}))
    save_file({k: v.contiguous() for k, v in ref.checkpoint_state_dict().items()}, str(d / "model.safetensors"))


def test_prefix_stripping_and_concept_table():
    from consistentid_amd import safety
    ref = _checker_ref()
    sd = ref.checkpoint_state_dict()
    assert "vision_model.vision_model.embeddings.class_embedding" in sd
    tower = safety.tower_state_dict(sd)
    inner = [k for k in sd if k.startswith("vision_model.vision_model.")]
    assert set(tower) == {k[len("vision_model."):] for k in inner} | {"visual_projection.weight"}
    assert "vision_model.embeddings.patch_embedding.weight" in tower and "vision_model.post_layernorm.weight" in tower
    assert not any(k.startswith("concept") or k.startswith("special") for k in tower)
    with pytest.raises(KeyError):
        safety.tower_state_dict({"vision_model.embeddings.class_embedding": torch.zeros(4), "visual_projection.weight": torch.zeros(4, 4)})
    sd["concept_embeds_weights"] = torch.linspace(0.1, 0.3, 17)
    sd["special_care_embeds_weights"] = torch.tensor([0.5, 0.6, 0.7])
    rows, thr, n_special = safety.concept_table(sd)
    assert n_special == 3 and rows.shape == (20, 64) and rows.dtype == thr.dtype == torch.float32
    assert torch.allclose(rows.norm(dim=-1), torch.ones(20), atol=1e-6)
    assert torch.equal(rows[:3], torch.nn.functional.normalize(sd["special_care_embeds"].float(), dim=-1))      # special-care first
    assert torch.equal(thr[:3], sd["special_care_embeds_weights"]) and torch.equal(thr[3:], sd["concept_embeds_weights"])
    with pytest.raises(NotImplementedError):
        safety.concept_table(dict(sd, concept_embeds=torch.randn(70, 64), concept_embeds_weights=torch.ones(70)))


def test_checker_reads_geometry_from_shapes_and_the_rest_from_config(tmp_path):
    """HipSafetyChecker on the CPU (packing only, nothing is launched): geometry from the tensors, heads / patch / eps /
    activation from vision_config, transformers' defaults for what it leaves out"""
    from consistentid_amd import loader, safety
    ref = _checker_ref()
    _write_checker(tmp_path, ref, {"num_attention_heads": 2, "patch_size": 14, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-6})
    chk = loader.load_safety_checker(tmp_path / "safety_checker", device="cpu")
    assert isinstance(chk, safety.HipSafetyChecker)
    v = chk.vision
    assert (v.C, v.heads, v.d, v.P, v.n_layers, v.eps) == (128, 2, 64, 14, 2, 1e-6)
    assert v._act.__name__ == "quick_gelu_" and chk.image_size == 70 and chk.n_special == 3
    assert v.visual_projection.shape == (64, 128) and v.post_ln[0].shape == (128,)
    assert chk.concepts.shape == (20, 64) and chk.concepts.dtype == torch.float32 and chk.thresholds.shape == (20,)
    # config.json without the keys: CLIPVisionConfig defaults (12 heads, patch 32) do not fit these tensors -> named
    with pytest.raises(ValueError, match="patch_size 32"):
        safety.HipSafetyChecker({}, ref.checkpoint_state_dict(), device="cpu")
    d = safety.HipSafetyChecker({"vision_config": {"patch_size": 14, "num_attention_heads": 4}}, ref.checkpoint_state_dict(), device="cpu")
    assert (d.vision.heads, d.vision.eps, d.vision._act.__name__) == (4, 1e-5, "quick_gelu_")
    with pytest.raises(NotImplementedError, match="hidden_act"):
        safety.HipSafetyChecker({"vision_config": {"patch_size": 14, "num_attention_heads": 2, "hidden_act": "relu"}},
                                ref.checkpoint_state_dict(), device="cpu")


def test_preprocessor_settings_and_refusals(tmp_path):
    from consistentid_amd import loader
    assert loader.preprocessor_settings(CLIP_PRE) == {"size": 224}
    assert loader.preprocessor_settings({}) == {"size": 224}                                     # CLIPImageProcessor defaults
    new_style = dict(CLIP_PRE, size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, do_rescale=True,
                     rescale_factor=1 / 255)
    assert loader.preprocessor_settings(new_style) == {"size": 224}
    assert loader.preprocessor_settings(loader.preprocessor_settings(dict(CLIP_PRE, size=70, crop_size=70))) == {"size": 70}
    for key, bad in (("resample", 2), ("do_center_crop", False), ("image_mean", [0.5, 0.5, 0.5]), ("image_std", [0.5, 0.5, 0.5]),
                     ("size", 256), ("crop_size", {"height": 224, "width": 200}), ("do_normalize", False),
                     ("do_resize", False), ("rescale_factor", 1 / 256)):
        with pytest.raises(NotImplementedError, match=key):
            loader.preprocessor_settings(dict(CLIP_PRE, **{key: bad}))
    d = tmp_path / "feature_extractor"
    d.mkdir()
    with pytest.raises(FileNotFoundError):
        loader.read_feature_extractor(d)
    (d / "preprocessor_config.json").write_text(json.dumps(CLIP_PRE))
    assert loader.read_feature_extractor(d) == {"size": 224}


def test_safety_keywords_follow_diffusers(tmp_path):
    """folder there and no keyword -> loaded; safety_checker=None -> not loaded (and no feature extractor either); a ready
    object is kept; no folder -> nothing"""
    from consistentid_amd import loader, safety
    assert loader.read_safety_components(tmp_path) == {}
    _write_checker(tmp_path, _checker_ref(), {"num_attention_heads": 2, "patch_size": 14})
    (tmp_path / "feature_extractor").mkdir()
    (tmp_path / "feature_extractor" / "preprocessor_config.json").write_text(json.dumps(dict(CLIP_PRE, size=70, crop_size=70)))
    got = loader.read_safety_components(tmp_path, device="cpu")
    assert isinstance(got["safety_checker"], safety.HipSafetyChecker) and got["feature_extractor"] == {"size": 70}
    assert loader.read_safety_components(tmp_path, device="cpu", given={"safety_checker": None}) == {}
    ready = object()
    got = loader.read_safety_components(tmp_path, device="cpu", given={"safety_checker": ready, "feature_extractor": CLIP_PRE})
    assert got["safety_checker"] is ready and got["feature_extractor"] == {"size": 224}
    got = loader.read_safety_components(tmp_path, device="cpu", given={"safety_checker": ready, "feature_extractor": None})
    assert got == {"safety_checker": ready}
    (tmp_path / "feature_extractor" / "preprocessor_config.json").write_text(json.dumps(dict(CLIP_PRE, resample=2)))
    with pytest.raises(NotImplementedError, match="resample"):
        loader.read_safety_components(tmp_path, device="cpu")


def test_pipeline_without_checker_reports_none():
    """run_safety_checker without a checker is diffusers': the image as it came, None"""
    from types import SimpleNamespace
    from consistentid_amd import pipeline
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(SimpleNamespace(device="cpu"), use_graph=False)
    arr = np.random.default_rng(0).random((2, 8, 8, 3), dtype=np.float32)
    out, nsfw = pipe.run_safety_checker(arr, "cpu", torch.float16)
    assert out is arr and nsfw is None
    assert pipe._output(arr, False) == (arr, None) and pipe._output(arr, True).nsfw_content_detected is None

    class Stub:                     # a ready checker object with diffusers' call: flags the brighter image
        image_size = 28

        def __call__(self, images, clip_input):
            assert clip_input.shape == (2, 3, 28, 28) and clip_input.dtype == torch.float32
            has = [bool(v) for v in (clip_input.mean(dim=(1, 2, 3)) > clip_input.mean())]
            for i, h in enumerate(has):
                if h:
                    images[i] = np.zeros(images[i].shape)
            return images, has

    arr[1] = arr[1] * 0.5 + 0.5
    keep = arr.copy()
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(SimpleNamespace(device="cpu"), use_graph=False, safety_checker=Stub())
    out, nsfw = pipe.run_safety_checker(arr)
    assert nsfw == [False, True] and not out[1].any() and np.array_equal(out[0], keep[0])
    assert pipe._output(out, True, nsfw).nsfw_content_detected == [False, True]
