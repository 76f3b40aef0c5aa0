"""Host-side image pre-processing of the inpaint pipelines: the PIL branch of diffusers 0.23.0
``VaeImageProcessor.preprocess`` for the three processors the reference pipelines construct (once per image, CPU; numpy /
PIL, like face_prep.py):

  ``preprocess_image``    image_processor          resize, normalize                       fp32 [B, 3, H, W] in [-1, 1]
  ``preprocess_mask``     mask_processor           do_convert_grayscale, resize,           fp32 [B, 1, H, W] in {0, 1}
                                                   do_normalize=False, do_binarize
  ``preprocess_control``  control_image_processor  do_convert_rgb, resize,                 fp32 [B, 3, H, W] in [0, 1]
                                                   do_normalize=False

(inpaint ref :232-239; ControlNet ref :255-280.)  The order of the steps, as diffusers 0.23.0 does them:

  1. mode conversion first: ``convert("RGB")`` / ``convert("L")``;
  2. ``get_default_height_width``: the given ``height`` / ``width``, each rounded DOWN to a multiple of 8
     (vae_scale_factor); without them the first image's own size, rounded down;
  3. ``image.resize((width, height), resample=PIL.Image.LANCZOS)``;
  4. ``np.array(img).astype(np.float32) / 255.0``;
  5. HWC -> CHW;
  6. ``2x - 1`` when normalizing;
  7. binarise: ``< 0.5 -> 0``, ``>= 0.5 -> 1`` -- for a uint8 grey value that is ``>= 128``.

diffusers is not a dependency of this project and is not installed where its tests run, so none of these facts is pinned
by a test against diffusers itself: they are stated from its 0.23.0 source (image_processor.py), and the tests hold this
module to the steps as written here.  The order of steps 1 and 3 is observable: on a noisy RGB mask, converting before
resizing and resizing before converting disagree after binarisation (about half a percent of the pixels of a random 40 x 56
image resized to 48 x 64).

Two deliberate differences:
* the reference's ``image_processor`` converts no modes, so an RGBA or L init image fails later inside its VAE; here the
  init image is converted to RGB;
* images of different sizes in one list, with no ``height`` / ``width`` to bring them to, raise ValueError (diffusers
  resizes all of them to the first image's size).

Accepted inputs: one PIL image or a list of them.  numpy arrays raise NotImplementedError (diffusers' numpy convention is
NHWC, which nothing in this project uses); float tensors never come here -- the pipelines take them as they are.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
from PIL import Image

VAE_SCALE_FACTOR = 8


def is_pil(x) -> bool:
    """one PIL image, or a non-empty list / tuple of them"""
    if isinstance(x, (list, tuple)):
        return len(x) > 0 and all(isinstance(i, Image.Image) for i in x)
    return isinstance(x, Image.Image)


def _as_list(images, what: str) -> List[Image.Image]:
    if is_pil(images):
        return list(images) if isinstance(images, (list, tuple)) else [images]
    raise NotImplementedError(f"{what}: one PIL image or a list of PIL images expected, got {type(images).__name__} "
                              "(numpy arrays are not taken; float tensors go to the pipelines as they are)")


def default_height_width(images: List[Image.Image], height: Optional[int], width: Optional[int]) -> Tuple[int, int]:
    """diffusers' get_default_height_width: the given size, else the images' own, rounded down to multiples of 8"""
    if height is None or width is None:
        sizes = {im.size for im in images}
        if len(sizes) > 1:
            raise ValueError(f"images of different sizes {sorted(sizes)} (width, height) need height= and width=")
    height = images[0].height if height is None else int(height)
    width = images[0].width if width is None else int(width)
    height, width = height - height % VAE_SCALE_FACTOR, width - width % VAE_SCALE_FACTOR
    if height <= 0 or width <= 0:
        raise ValueError(f"height x width {height} x {width} after rounding down to multiples of {VAE_SCALE_FACTOR}")
    return height, width


def _preprocess(images, height, width, mode: str, what: str) -> torch.Tensor:
    imgs = [im.convert(mode) for im in _as_list(images, what)]                      # 1
    height, width = default_height_width(imgs, height, width)                        # 2
    arrs = [np.array(im.resize((width, height), resample=Image.LANCZOS)).astype(np.float32) / 255.0 for im in imgs]   # 3, 4
    x = np.stack([a[..., None] if a.ndim == 2 else a for a in arrs])
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))          # 5


def preprocess_image(image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
    """the init image: fp32 [B, 3, H, W] in [-1, 1]"""
    return 2.0 * _preprocess(image, height, width, "RGB", "image") - 1.0            # 6


def preprocess_mask(mask_image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
    """the inpaint mask: fp32 [B, 1, H, W] in {0, 1}, 1 = repaint"""
    return (_preprocess(mask_image, height, width, "L", "mask_image") >= 0.5).float()    # 7


def preprocess_control(control_image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
    """the ControlNet's condition image: fp32 [B, 3, H, W] in [0, 1]"""
    return _preprocess(control_image, height, width, "RGB", "control_image")
