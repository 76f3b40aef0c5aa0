"""The parsing colour overlay (the reference's parsing_face_mask visualisation) without a GPU."""
import numpy as np


def test_parsing_overlay_blend_and_rounding():
    from consistentid_amd.face_prep import PART_COLORS, parsing_overlay
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (6, 7)).astype(np.uint8)
    lab[0, 0] = 0
    out = parsing_overlay(img, lab)
    assert out.shape == img.shape and out.dtype == np.uint8
    color = np.array([(255, 255, 255)] + list(PART_COLORS[1:]), np.float32)[lab]
    want = np.clip(np.rint(img[..., ::-1].astype(np.float32) * np.float32(0.4) + color * np.float32(0.6)), 0, 255)
    assert np.array_equal(out, want.astype(np.uint8))
    assert np.array_equal(out[0, 0], np.rint(img[0, 0, ::-1] * np.float32(0.4) + np.float32(153)).astype(np.uint8))
    # x.5 rounds to even, like cv2's saturate_cast: 0.4 * 5 + 0.6 * 0 = 2.0, 0.4 * 255 + 0.6 * 0 = 102.0
    edge = parsing_overlay(np.full((1, 1, 3), 5, np.uint8), np.full((1, 1), 11, np.uint8))     # colour (85, 0, 255)
    assert edge[0, 0].tolist() == [int(np.rint(np.float32(2) + np.float32(51))), 2, int(np.rint(np.float32(2) + np.float32(153)))]
