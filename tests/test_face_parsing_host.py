"""Face parser and its host pre-processing without a GPU: the BatchNorm fold, checkpoint handling, the C entry points'
argument checks (cid_gemm_desc.act and the csrc/parsing.hip entries), mask extraction / key selection, the masked crop and
the CLIP image pre-processing."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from bisenet_ref import random_state_dict


# --------------------------------------------------------------------------- BN fold / checkpoint
def test_bn_fold_matches_fp64_conv_bn():
    from consistentid_amd.face_parsing import fold_bn
    g = torch.Generator().manual_seed(1)
    sd = {"c.weight": torch.randn(32, 16, 3, 3, generator=g), "b.weight": torch.rand(32, generator=g) + 0.5,
          "b.bias": torch.randn(32, generator=g), "b.running_mean": torch.randn(32, generator=g),
          "b.running_var": torch.rand(32, generator=g) + 0.1}
    w, b = fold_bn(sd, "c", "b")
    assert w.dtype == torch.float32 and b.dtype == torch.float32
    x = torch.randn(2, 16, 9, 9, generator=g, dtype=torch.float64)
    d = {k: v.double() for k, v in sd.items()}
    ref = F.batch_norm(F.conv2d(x, d["c.weight"], padding=1), d["b.running_mean"], d["b.running_var"], d["b.weight"],
                       d["b.bias"], False, 0.0, 1e-5)
    got = F.conv2d(x, w.double(), b.double(), padding=1)
    assert (got - ref).abs().max().item() < 1e-5 * ref.abs().max().item()


def test_state_dict_prefix_ignored_heads_and_missing_key():
    from consistentid_amd.face_parsing import HipBiSeNet, clean_state_dict
    sd = random_state_dict(seed=3)
    assert any(k.startswith("conv_out16.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    clean = clean_state_dict({"module." + k: v for k, v in sd.items()})
    assert not any(k.startswith(("module.", "conv_out16.", "conv_out32.")) or k.endswith("num_batches_tracked") for k in clean)
    assert "cp.resnet.conv1.weight" in clean and "conv_out.conv_out.weight" in clean
    a = HipBiSeNet({"module." + k: v for k, v in sd.items()}, device="cpu")
    b = HipBiSeNet(random_state_dict(seed=3, aux_heads=False), device="cpu")
    assert a.W.keys() == b.W.keys()
    assert all(torch.equal(a.W[k], b.W[k]) for k in a.W)
    # the 1x1 stride-2 shortcut is a 3x3 weight that is zero outside the centre tap; the head is padded to 32 rows
    dw = a.W["cp.resnet.layer2.0.down.w"].reshape(128, 9, 64)
    assert dw[:, 4].abs().sum() > 0 and dw[:, [0, 1, 2, 3, 5, 6, 7, 8]].abs().sum() == 0
    assert a.W["head.out.w"].shape == (32, 256) and a.W["head.out.w"][19:].abs().sum() == 0
    bad = dict(sd)
    del bad["cp.arm16.bn_atten.running_var"]
    with pytest.raises(KeyError, match="cp.arm16.bn_atten.running_var"):
        HipBiSeNet(bad, device="cpu")


# --------------------------------------------------------------------------- C ABI
def test_new_entries_are_exported_and_refuse_bad_shapes(lib):
    from consistentid_amd._lib import GemmDesc
    assert lib.cid_version() >= 102
    for n in ("cid_parse_stem_f16", "cid_chan_mean_f16", "cid_chan_gate_f32", "cid_chan_affine_f16", "cid_parse_head_f16"):
        assert hasattr(lib, n)
    assert lib.cid_parse_stem_f16(64, 64, 64, 64, 1, 500, 512, None) == -22 and b"multiples of 32" in lib.cid_last_error()
    assert lib.cid_parse_stem_f16(None, 64, 64, 64, 1, 512, 512, None) == -22 and b"null" in lib.cid_last_error()
    assert lib.cid_chan_mean_f16(64, 64, 1, 16, 12, 12, None) == -22 and b"bad shape" in lib.cid_last_error()
    assert lib.cid_chan_gate_f32(64, 64, 64, None, None, None, 1, 1024, 128, 128, 1, None) == -22
    assert b"512" in lib.cid_last_error()
    assert lib.cid_chan_gate_f32(64, 64, 64, None, None, None, 1, 256, 128, 64, 1, None) == -22       # N != N1 without w2
    assert lib.cid_chan_gate_f32(64, 64, 64, None, None, None, 1, 256, 128, 128, 3, None) == -22
    assert b"act" in lib.cid_last_error()
    assert lib.cid_chan_affine_f16(64, 64, 64, 64, 64, 1, 16, 64, None) == -22 and b"not both" in lib.cid_last_error()
    assert lib.cid_chan_affine_f16(64, 64, None, None, 64, 1, 16, 60, None) == -22
    assert lib.cid_parse_head_f16(64, 16, 19, 1, 64, 64, 512, 512, 64, None, None) == -22 and b"ncls" in lib.cid_last_error()

    def desc(**kw):
        d = GemmDesc()
        d.x1, d.w, d.out = 64, 64, 64
        d.c1, d.ld1, d.ldo, d.M, d.N, d.taps = 128, 128, 128, 4096, 128, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert lib.cid_gemm_f16(C.byref(desc(act=2)), None) == -22 and b"bad act" in lib.cid_last_error()
    assert lib.cid_gemm_f16(C.byref(desc(act=1, mode=1)), None) == -22 and b"act 1" in lib.cid_last_error()
    assert lib.cid_gemm_f16(C.byref(desc(act=1, gn_stats=64)), None) == -22 and b"act 1" in lib.cid_last_error()
    assert lib.cid_gemm_f16(C.byref(desc(act=1, ws=64, ws_bytes=1 << 26)), None) == -22 and b"ws" in lib.cid_last_error()
    # an act-1 launch never promises GroupNorm statistics
    conv = dict(taps=9, c1=320, ld1=320, ldo=320, N=320, M=8 * 64 * 64, Hi=64, Wi=64, Ho=64, Wo=64, stride=1)
    assert lib.cid_gemm_stats_rows(C.byref(desc(**conv))) > 0
    assert lib.cid_gemm_stats_rows(C.byref(desc(act=1, **conv))) == 0


# --------------------------------------------------------------------------- masks and key selection
def _names(d):
    return list(d.keys())


def test_masks_fill_holes_like_external_contours():
    from consistentid_amd.face_prep import masks_for_unique_values
    lab = np.zeros((12, 14), np.uint8)
    lab[1:6, 1:6] = 1            # ring of value 1 with a hole of value 4 ...
    lab[2:5, 2:5] = 4
    lab[3, 3] = 0                # ... which holds a background pixel
    lab[7:12, 2] = 10            # a U of value 10 open to the bottom border
    lab[7:12, 6] = 10
    lab[7, 2:7] = 10
    lab[8:12, 3:6] = 13          # the inside of the U touches the border: not a hole
    lab[0, 10:12] = 5            # two components of value 5
    lab[9:11, 10:12] = 5
    lab[3, 9] = 12               # diagonal-touching pixels around a background pixel
    lab[4, 8] = 12
    lab[4, 10] = 12
    lab[5, 9] = 12
    m = masks_for_unique_values(lab)
    assert _names(m) == ["WithoutBackground", "Background", "Face", "Left_Eye", "Right_Eye", "Nose", "Upper_Lip",
                         "Lower_Lip"]
    arr = {k: np.asarray(v) for k, v in m.items()}
    assert all(a.dtype == np.uint8 and set(np.unique(a)) <= {0, 255} and v.mode == "L" for (k, a), v in zip(arr.items(), m.values()))
    face = np.zeros_like(lab)
    face[1:6, 1:6] = 255
    assert np.array_equal(arr["Face"], face)                       # hole filled, including the value-4 and value-0 pixels
    assert np.array_equal(arr["Left_Eye"] == 255, np.pad(np.ones((3, 3), bool), ((2, 7), (2, 9))))
    assert np.array_equal(arr["Nose"] == 255, lab == 10)           # open U: nothing to fill
    assert np.array_equal(arr["Right_Eye"] == 255, lab == 5)       # both components
    lips = lab == 12
    lips[4, 9] = True                                              # 8-connected ring: its 4-connected inside is a hole
    assert np.array_equal(arr["Upper_Lip"] == 255, lips)
    assert np.array_equal(arr["WithoutBackground"] == 255, arr["Background"] != 255)


def test_unknown_values_and_key_selection_dedupe():
    from consistentid_amd.face_prep import masks_for_unique_values, select_face_masks
    lab = np.array([[1, 1, 4, 5], [7, 8, 10, 12], [13, 2, 3, 30], [6, 9, 11, 14]], np.uint8)
    m = masks_for_unique_values(lab)
    assert "WithoutBackground" not in m and not any(k.startswith("Unknown") for k in m)
    assert _names(m)[:4] == ["Face", "Left_Eyebrow", "Right_Eyebrow", "Left_Eye"]
    sel = select_face_masks(m)
    # Left_Eye (4) comes before Right_Eye (5), Left_Ear (7) before Right_Ear (8): one of each pair.  The rule keys on the
    # word after the first "_", so Lower_Lip (13) goes as the partner of Upper_Lip (12), as in the reference
    assert _names(sel) == ["Face", "Left_Eye", "Left_Ear", "Nose", "Upper_Lip"]
    only_right = select_face_masks(masks_for_unique_values(np.array([[0, 5], [8, 1]], np.uint8)))
    assert _names(only_right) == ["Face", "Right_Eye", "Right_Ear"]


# --------------------------------------------------------------------------- crops and CLIP pre-processing
def _img(w, h, seed):
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


def test_fetch_mask_raw_image_matches_pil():
    from consistentid_amd.face_prep import fetch_mask_raw_image
    raw = _img(300, 220, 0)
    mask = Image.fromarray((np.random.default_rng(1).random((512, 512)) > 0.5).astype(np.uint8) * 255)
    got = fetch_mask_raw_image(raw, mask)
    ref = Image.composite(raw, Image.new("RGB", raw.size, (0, 0, 0)), mask.resize(raw.size))
    assert got.size == raw.size and np.array_equal(np.asarray(got), np.asarray(ref))


@pytest.mark.parametrize("wh", [(224, 224), (512, 512), (301, 199), (199, 301), (640, 97), (97, 640), (225, 224)])
def test_clip_preprocess_matches_transformers(wh):
    transformers = pytest.importorskip("transformers")
    from consistentid_amd.face_prep import clip_preprocess
    img = _img(*wh, seed=wh[0] * 7 + wh[1])
    ref = transformers.CLIPImageProcessor()(images=img, return_tensors="np").pixel_values[0]
    got = clip_preprocess(img)
    assert got.shape == ref.shape == (3, 224, 224) and got.dtype == np.float32
    assert np.abs(got - ref).max() <= 1e-5
