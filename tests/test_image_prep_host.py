"""image_prep.py on the host: the PIL branch of diffusers 0.23.0 VaeImageProcessor.preprocess restated step by step with
PIL and numpy (diffusers is not installed, so the module is held to the steps its docstring states, not to diffusers itself),
and the no-op memory / progress-bar methods of the pipeline classes."""
import numpy as np
import pytest
import torch
from PIL import Image

from consistentid_amd import image_prep


def _rand(h, w, mode="RGB", seed=0):
    shape = (h, w, len(mode)) if len(mode) > 1 else (h, w)
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8), mode)


def _chw(arr):
    """uint8 HWC / HW -> fp32 [1, C, H, W] / 255"""
    a = np.asarray(arr).astype(np.float32) / 255.0
    a = a[..., None] if a.ndim == 2 else a
    return a.transpose(2, 0, 1)[None]


def test_image_without_resampling():
    img = _rand(96, 64, seed=1)
    got = image_prep.preprocess_image(img, height=96, width=64)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 96, 64)
    assert np.array_equal(got.numpy(), _chw(img) * 2 - 1)
    assert got.min() >= -1 and got.max() <= 1 and got.min() < 0


def test_image_resize_and_rounding():
    img = _rand(40, 56, seed=2)                                  # height 40, width 56
    want = _chw(img.resize((48, 64), Image.LANCZOS)) * 2 - 1    # PIL sizes are (width, height)
    got = image_prep.preprocess_image(img, height=64, width=48)
    assert tuple(got.shape) == (1, 3, 64, 48)                    # a swapped height / width fails here
    assert np.array_equal(got.numpy(), want)
    rounded = image_prep.preprocess_image(img, height=70, width=50)      # down to multiples of 8
    assert tuple(rounded.shape) == (1, 3, 64, 48) and torch.equal(rounded, got)
    own = image_prep.preprocess_image(_rand(45, 61, seed=3))     # no size: the image's own, rounded down
    assert tuple(own.shape) == (1, 3, 40, 56)


def test_image_modes_are_converted_to_rgb():
    rgba, grey = _rand(32, 24, "RGBA", seed=4), _rand(32, 24, "L", seed=5)
    assert np.array_equal(image_prep.preprocess_image(rgba).numpy(), _chw(rgba.convert("RGB")) * 2 - 1)
    g = image_prep.preprocess_image(grey)
    assert tuple(g.shape) == (1, 3, 32, 24) and torch.equal(g[:, 0], g[:, 1]) and torch.equal(g[:, 0], g[:, 2])


def test_mask_converts_before_it_resizes():
    m = _rand(40, 56, seed=6)                                    # a noisy RGB mask
    convert_first = np.asarray(m.convert("L").resize((48, 64), Image.LANCZOS)) >= 128
    resize_first = np.asarray(m.resize((48, 64), Image.LANCZOS).convert("L")) >= 128
    assert (convert_first != resize_first).any()                 # the two orders are distinguishable on this input
    got = image_prep.preprocess_mask(m, height=64, width=48)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, 64, 48)
    assert np.array_equal(got.numpy()[0, 0], convert_first.astype(np.float32))
    assert set(np.unique(got.numpy()).tolist()) == {0.0, 1.0}


def test_mask_threshold():
    grey = Image.fromarray(np.array([[127, 128] * 4] * 8, dtype=np.uint8), "L")      # 8 x 8, no resampling
    got = image_prep.preprocess_mask(grey)
    assert tuple(got.shape) == (1, 1, 8, 8)
    assert (got[0, 0, :, 0::2] == 0).all() and (got[0, 0, :, 1::2] == 1).all()


def test_control_image():
    c = _rand(40, 56, "L", seed=7)
    got = image_prep.preprocess_control(c, height=64, width=48)
    assert tuple(got.shape) == (1, 3, 64, 48)
    assert np.array_equal(got.numpy(), _chw(c.convert("RGB").resize((48, 64), Image.LANCZOS)))
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
    assert got.min() >= 0 and got.max() <= 1 and got.max() > 0.5          # [0, 1]: not normalised


def test_lists():
    a, b = _rand(32, 24, seed=8), _rand(32, 24, seed=9)
    got = image_prep.preprocess_image([a, b])
    assert tuple(got.shape) == (2, 3, 32, 24)
    assert torch.equal(got[:1], image_prep.preprocess_image(a)) and torch.equal(got[1:], image_prep.preprocess_image(b))
    assert tuple(image_prep.preprocess_mask([a, b], 16, 16).shape) == (2, 1, 16, 16)
    sized = image_prep.preprocess_image([a, _rand(48, 40, seed=10)], height=32, width=24)     # a given size reconciles them
    assert tuple(sized.shape) == (2, 3, 32, 24)


def test_refused_inputs():
    arr = np.zeros((32, 24, 3), np.uint8)
    for f in (image_prep.preprocess_image, image_prep.preprocess_mask, image_prep.preprocess_control):
        with pytest.raises(NotImplementedError):
            f(arr)
        with pytest.raises(NotImplementedError):
            f([_rand(8, 8), arr])
    with pytest.raises(ValueError, match="different sizes"):
        image_prep.preprocess_image([_rand(32, 24), _rand(24, 32)])
    with pytest.raises(ValueError):
        image_prep.preprocess_image(_rand(32, 24), height=7, width=24)       # rounds down to nothing


def test_memory_and_progress_bar_methods_do_nothing():
    from consistentid_amd import pipeline
    names = ("enable_model_cpu_offload", "enable_sequential_cpu_offload", "enable_vae_slicing", "enable_vae_tiling",
             "enable_xformers_memory_efficient_attention", "set_progress_bar_config")
    for cls in (pipeline.ConsistentIDStableDiffusionPipeline, pipeline.ConsistentIDStableDiffusionXLPipeline,
                pipeline.StableDiffusionInpaintConsistentIDPipeline,
                pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline):
        pipe = object.__new__(cls)                               # the methods touch no state: no engine needed
        for name in names:
            assert callable(getattr(cls, name)), (cls.__name__, name)
            assert getattr(pipe, name)() is None
            assert getattr(pipe, name)("cuda:1", 3, disable=True, gpu_id=0) is None
        assert pipe.__dict__ == {}
