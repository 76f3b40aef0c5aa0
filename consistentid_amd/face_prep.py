"""Host-side pre-processing around the face parser: what the reference does with the parsing labels before the CLIP
vision tower and the FacialEncoder see the face (once per image, CPU; numpy / scipy / PIL, no cv2 or torchvision).

* ``masks_for_unique_values``: one filled mask per label value (functions.py:361-387 with the value -> part-name table of
  :333-359).  cv2 fills the external contours of each value's region, i.e. the region with its holes filled; here that
  is ``scipy.ndimage.binary_fill_holes``, whose 4-connected background is the complement of cv2's 8-connected contours.
  Value 0 also yields the inverted "WithoutBackground" mask, ahead of "Background", as in the reference.
* ``select_face_masks``: the key selection of ``get_prepare_facemask`` (pipline_StableDiffusion_ConsistentID.py:289-309),
  in ``np.unique`` order, with its Left / Right dedupe: of "Left_Eye" / "Right_Eye" (and the ears) only the first found
  is kept.
* ``fetch_mask_raw_image``: functions.py:326-331 (PIL resize with its default filter, then ``Image.composite``).
* ``clip_preprocess``: the default ``CLIPImageProcessor()`` the reference builds in ``get_prepare_clip_image`` (:355,
  :363): shortest edge 224 (bicubic), centre crop 224, rescale by 1/255, OpenAI CLIP mean / std -> fp32 [3, 224, 224].
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict

import numpy as np
from PIL import Image

# value -> part name of the 19-class parser's label map (and the six further values the reference's table names)
PART_NAMES = {
    0: "Background", 1: "Face", 2: "Left_Eyebrow", 3: "Right_Eyebrow", 4: "Left_Eye", 5: "Right_Eye", 6: "Hair",
    7: "Left_Ear", 8: "Right_Ear", 9: "Mouth_External Contour", 10: "Nose", 11: "Mouth_Inner_Contour", 12: "Upper_Lip",
    13: "Lower_Lip", 14: "Neck", 15: "Neck_Inner Contour", 16: "Cloth", 17: "Hat", 18: "Earring", 19: "Necklace",
    20: "Glasses", 21: "Hand", 22: "Wristband", 23: "Clothes_Upper", 24: "Clothes_Lower",
}
FACE_KEYS = ("Face", "Left_Ear", "Right_Ear", "Left_Eye", "Right_Eye", "Nose", "Upper_Lip", "Lower_Lip")

CLIP_SIZE = 224
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def fill_holes(region: np.ndarray) -> np.ndarray:
    """bool region -> the region plus every hole in it (background not 4-connected to the border)"""
    from scipy import ndimage
    return ndimage.binary_fill_holes(region)


def masks_for_unique_values(labels) -> "OrderedDict[str, Image.Image]":
    """label map (uint8 [H, W], array or PIL) -> {part name: mode-L PIL mask, 255 inside}, in ``np.unique`` order"""
    arr = np.asarray(labels)
    out: "OrderedDict[str, Image.Image]" = OrderedDict()
    for value in np.unique(arr):
        mask = np.where(fill_holes(arr == value), 255, 0).astype(arr.dtype)
        if value == 0:
            out["WithoutBackground"] = Image.fromarray(np.where(mask == 255, 0, 255).astype(arr.dtype))
        name = PART_NAMES.get(int(value))
        if name is None:
            continue
        out[name] = Image.fromarray(mask)
    return out


def select_face_masks(masks: Dict[str, Image.Image]) -> "OrderedDict[str, Image.Image]":
    """the facial parts the reference crops, in the order of ``masks``; one of each Left / Right pair (the first met)"""
    out: "OrderedDict[str, Image.Image]" = OrderedDict()
    seen = set()
    for key, m in masks.items():
        if key not in FACE_KEYS:
            continue
        if "_" in key:
            part = key.split("_")[1]
            if part in seen:
                continue
            seen.add(part)
        out[key] = m
    return out


def fetch_mask_raw_image(raw_image: Image.Image, mask_image: Image.Image) -> Image.Image:
    """``raw_image`` where the (resized) mask is set, black elsewhere"""
    mask_image = mask_image.resize(raw_image.size)
    return Image.composite(raw_image, Image.new("RGB", raw_image.size, (0, 0, 0)), mask_image)


def clip_resize_shape(height: int, width: int, size: int = CLIP_SIZE):
    """(height, width) after scaling the shorter edge to ``size`` (the longer edge truncated, as transformers does)"""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def clip_preprocess(image: Image.Image, size: int = CLIP_SIZE) -> np.ndarray:
    """fp32 [3, size, size] pixel values of the default CLIPImageProcessor"""
    image = image.convert("RGB")
    h, w = clip_resize_shape(image.height, image.width, size)
    x = np.asarray(image.resize((w, h), resample=Image.BICUBIC))
    top, left = (h - size) // 2, (w - size) // 2
    x = x[top:top + size, left:left + size]
    x = (x.astype(np.float64) * (1 / 255)).astype(np.float32)
    x = (x - np.asarray(CLIP_MEAN, dtype=np.float32)) / np.asarray(CLIP_STD, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


# colour of label value v at PART_COLORS[v] (value 0 and values past the table stay white); a label map's colour overlay
# is the reference's parsing_face_mask visualisation (pipline_StableDiffusion_ConsistentID.py:246-262)
PART_COLORS = ((255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 0, 85), (255, 0, 170), (0, 255, 0), (85, 255, 0),
               (170, 255, 0), (0, 255, 85), (0, 255, 170), (0, 0, 255), (85, 0, 255), (170, 0, 255), (0, 85, 255),
               (0, 170, 255), (255, 255, 0), (255, 255, 85), (255, 255, 170), (255, 0, 255), (255, 85, 255),
               (255, 170, 255), (0, 255, 255), (85, 255, 255), (170, 255, 255))


def parsing_overlay(image_rgb: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """uint8 [H, W, 3]: 0.4 x the image in BGR order + 0.6 x the part colours (white where unlabelled), summed in fp32 and
    rounded half to even with saturation, as cv2.addWeighted does for 8-bit images"""
    labels = np.asarray(labels, dtype=np.uint8)
    color = np.full(labels.shape + (3,), 255, np.uint8)
    for v in range(1, min(int(labels.max(initial=0)), len(PART_COLORS) - 1) + 1):
        color[labels == v] = PART_COLORS[v]
    bgr = np.ascontiguousarray(np.asarray(image_rgb, dtype=np.uint8)[..., ::-1])
    mix = bgr.astype(np.float32) * np.float32(0.4) + color.astype(np.float32) * np.float32(0.6)
    return np.clip(np.rint(mix), 0, 255).astype(np.uint8)
