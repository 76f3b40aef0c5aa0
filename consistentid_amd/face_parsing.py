"""HIP execution engine for the face parser (BiSeNet, 19 classes).

The reference parses every ID image once: ``self.bise_net(img)[0]`` on a 512 x 512 PIL bilinear resize, ToTensor and the
ImageNet Normalize, then ``.argmax(0)`` over the classes (pipline_StableDiffusion_ConsistentID.py:229-244; the network is
models/BiSeNet/model.py + resnet.py).  Only the main head is read: the ``conv_out16`` / ``conv_out32`` heads the reference
computes and discards are not computed here.

Every BatchNorm (eval, eps 1e-5) is folded into its convolution on the host, W' = W g / sqrt(v + eps),
b' = b - m g / sqrt(v + eps), in fp32 and rounded once.  Activations are token-major fp16 ``[B, H*W, C]`` like the rest of
the engine.  Kernels (include/cid.h):

* stem (normalisation, conv 7x7/2, ReLU, maxpool 3x3/2): ``cid_parse_stem_f16``, one launch;
* every other convolution: ``cid_gemm_f16`` with the ReLU in its epilogue (``act=1``) and the BasicBlock residual as ``res``;
  3x3 stride 1 / 2, the nearest-2x upsample of the context path (``up=1``), the FFM concat (``x2``); the 1x1 stride-2
  shortcut is a taps-9 stride-2 convolution whose weight is zero outside the centre tap;
* the pooled branches: ``cid_chan_mean_f16`` -> ``cid_chan_gate_f32`` (conv_avg, the ARM attention, the FFM squeeze /
  excite, fp32) -> ``cid_chan_affine_f16`` (x * s + t | res | x);
* the head: 1x1 256 -> 19 (zero rows to 32) by ``cid_gemm_f16``, bilinear ``align_corners=True`` + argmax by
  ``cid_parse_head_f16``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

BN_EPS = 1e-5
PARSE_SIZE = 512          # the reference's resize (pipline_StableDiffusion_ConsistentID.py:238)
HEAD_LD = 32              # the 19 logits padded to the GEMM's 32-channel granularity
IGNORED_PREFIXES = ("conv_out16.", "conv_out32.")


def clean_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the checkpoint's tensors without a leading ``module.`` (DataParallel saves), the discarded auxiliary heads and the
    BatchNorm ``num_batches_tracked`` counters"""
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k.startswith(IGNORED_PREFIXES) or k.endswith("num_batches_tracked"):
            continue
        out[k] = v
    return out


def _get(sd: Dict[str, torch.Tensor], key: str) -> torch.Tensor:
    if key not in sd:
        raise KeyError(f"BiSeNet state dict is missing {key!r}")
    return sd[key]


def fold_bn(sd: Dict[str, torch.Tensor], conv: str, bn: str, eps: float = BN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 (W', b') of ``conv``.weight (bias-free) followed by the eval-mode BatchNorm ``bn``"""
    w = _get(sd, f"{conv}.weight").float()
    g, b = _get(sd, f"{bn}.weight").float(), _get(sd, f"{bn}.bias").float()
    m, v = _get(sd, f"{bn}.running_mean").float(), _get(sd, f"{bn}.running_var").float()
    s = g / torch.sqrt(v + eps)
    return w * s.reshape(-1, *([1] * (w.dim() - 1))), b - m * s


def _taps(w: torch.Tensor) -> torch.Tensor:
    """[O, I, kh, kw] -> the GEMM's [O, kh * kw * I] (k = tap * I + c)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def _centre_tap(w: torch.Tensor) -> torch.Tensor:
    """1x1 [O, I, 1, 1] -> a 3x3 [O, 9 * I] that is zero outside the centre tap (the stride-2 shortcut as a taps-9 conv)"""
    o, i = w.shape[:2]
    out = torch.zeros(o, 9, i, dtype=w.dtype)
    out[:, 4] = w.reshape(o, i)
    return out.reshape(o, 9 * i)


LAYERS = ((64, 64, 1), (64, 128, 2), (128, 256, 2), (256, 512, 2))    # (in, out, stride) of resnet layer1..4, 2 blocks each


class HipBiSeNet:
    """``HipBiSeNet(state_dict)(images)`` -> uint8 labels [B, H, W] on the device (the reference's ``parsing_anno``);
    ``logits=True`` also returns the upsampled fp32 logits [B, n_classes, H, W] (its ``out``).

    ``state_dict``: the ``face_parsing.pth`` tensors under the checkpoint's own names (``cp.resnet.*``, ``cp.arm16.*``,
    ``cp.arm32.*``, ``cp.conv_head16/32.*``, ``cp.conv_avg.*``, ``ffm.*``, ``conv_out.*``); see ``clean_state_dict`` for
    what is ignored.  A missing tensor raises ``KeyError`` naming it."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], n_classes: int = 19, device="cuda:0"):
        if not 0 < n_classes <= HEAD_LD:
            raise ValueError(f"n_classes must be in 1..{HEAD_LD} (got {n_classes})")
        sd = clean_state_dict(state_dict)
        dev = torch.device(device)
        self.device, self.n_classes = dev, n_classes
        h = lambda t: t.to(dev, torch.float16).contiguous()
        f = lambda t: t.to(dev, torch.float32).contiguous()
        W: Dict[str, torch.Tensor] = {}
        w, b = fold_bn(sd, "cp.resnet.conv1", "cp.resnet.bn1")
        W["stem.w"], W["stem.b"] = f(w.permute(0, 2, 3, 1)), f(b)
        for li, (cin, cout, stride) in enumerate(LAYERS, start=1):
            for bi in range(2):
                n = f"cp.resnet.layer{li}.{bi}"
                for c in ("1", "2"):
                    w, b = fold_bn(sd, f"{n}.conv{c}", f"{n}.bn{c}")
                    W[f"{n}.conv{c}.w"], W[f"{n}.conv{c}.b"] = h(_taps(w)), h(b)
                if bi == 0 and (cin != cout or stride != 1):
                    w, b = fold_bn(sd, f"{n}.downsample.0", f"{n}.downsample.1")
                    W[f"{n}.down.w"], W[f"{n}.down.b"] = h(_centre_tap(w)), h(b)
        for n in ("cp.arm32", "cp.arm16"):
            w, b = fold_bn(sd, f"{n}.conv.conv", f"{n}.conv.bn")
            W[f"{n}.conv.w"], W[f"{n}.conv.b"] = h(_taps(w)), h(b)
            w, b = fold_bn(sd, f"{n}.conv_atten", f"{n}.bn_atten")
            W[f"{n}.att.w"], W[f"{n}.att.b"] = f(w.reshape(w.shape[0], -1)), f(b)
        for n in ("cp.conv_head32", "cp.conv_head16"):
            w, b = fold_bn(sd, f"{n}.conv", f"{n}.bn")
            W[f"{n}.w"], W[f"{n}.b"] = h(_taps(w)), h(b)
        w, b = fold_bn(sd, "cp.conv_avg.conv", "cp.conv_avg.bn")
        W["cp.conv_avg.w"], W["cp.conv_avg.b"] = f(w.reshape(w.shape[0], -1)), f(b)
        w, b = fold_bn(sd, "ffm.convblk.conv", "ffm.convblk.bn")
        W["ffm.convblk.w"], W["ffm.convblk.b"] = h(_taps(w)), h(b)
        for c in ("conv1", "conv2"):
            w = _get(sd, f"ffm.{c}.weight").float()
            W[f"ffm.{c}.w"] = f(w.reshape(w.shape[0], -1))
        w, b = fold_bn(sd, "conv_out.conv.conv", "conv_out.conv.bn")
        W["head.conv.w"], W["head.conv.b"] = h(_taps(w)), h(b)
        wo = _get(sd, "conv_out.conv_out.weight").float()
        if wo.shape[0] != n_classes:
            raise ValueError(f"conv_out.conv_out.weight has {wo.shape[0]} classes, expected {n_classes}")
        pad = torch.zeros(HEAD_LD, wo.shape[1])
        pad[:n_classes] = wo.reshape(n_classes, -1)
        W["head.out.w"] = h(pad)
        self.W = W

    # ------------------------------------------------------------------ building blocks
    def _conv(self, x, name: str, *, B: int, Hi: int, Wi: int, cin: int, cout: int, taps: int = 9, stride: int = 1,
              up: int = 0, act: int = 1, res=None, bias: bool = True, x2=None, c2: int = 0):
        Ho, Wo = ((Hi << up) // stride, (Wi << up) // stride) if taps == 9 else (Hi, Wi)
        out = torch.empty(B, Ho * Wo, cout, dtype=torch.float16, device=self.device)
        ops.gemm(x, self.W[f"{name}.w"], out, M=B * Ho * Wo, N=cout, c1=cin, x2=x2, c2=c2,
                 bias=self.W[f"{name}.b"] if bias else None, res=res, taps=taps, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo,
                 stride=stride, up=up, act=act)
        return out

    def _mean(self, x, *, B: int, HW: int, C: int):
        m = torch.empty(B, C, dtype=torch.float32, device=self.device)
        return ops.chan_mean(x, m, B=B, HW=HW, C_=C)

    def _gate(self, m, w1, b1=None, w2=None, *, act: int):
        out = torch.empty(m.shape[0], (w2 if w2 is not None else w1).shape[0], dtype=torch.float32, device=self.device)
        return ops.chan_gate(m, out, w1, b1, w2, act=act)

    def _arm(self, x, name: str, *, B: int, Hs: int, Ws: int, cin: int, t=None, res=None):
        """AttentionRefinementModule f * sigmoid(BN(W mean(f))), f = CBR3x3(x), plus ``t`` (per channel) or ``res``"""
        f = self._conv(x, f"{name}.conv", B=B, Hi=Hs, Wi=Ws, cin=cin, cout=128)
        s = self._gate(self._mean(f, B=B, HW=Hs * Ws, C=128), self.W[f"{name}.att.w"], self.W[f"{name}.att.b"], act=2)
        return ops.chan_affine(f, s, f, B=B, HW=Hs * Ws, C_=128, t=t, res=res)

    # ------------------------------------------------------------------ forward
    def forward(self, img: torch.Tensor, logits: bool = False):
        """``img``: uint8 [B, H, W, 3] RGB on the device, H and W multiples of 32"""
        B, H, Wd, _ = img.shape
        if H % 32 or Wd % 32:
            raise ValueError(f"HipBiSeNet: H and W must be multiples of 32 (got {H} x {Wd})")
        W = self.W
        h, w = H // 4, Wd // 4
        x = torch.empty(B, h * w, 64, dtype=torch.float16, device=self.device)
        ops.parse_stem(img, x, W["stem.w"], W["stem.b"])
        feats = []
        for li, (cin, cout, stride) in enumerate(LAYERS, start=1):
            for bi in range(2):
                n = f"cp.resnet.layer{li}.{bi}"
                s = stride if bi == 0 else 1
                c_in = cin if bi == 0 else cout
                t = self._conv(x, f"{n}.conv1", B=B, Hi=h, Wi=w, cin=c_in, cout=cout, stride=s)
                sc = x
                if f"{n}.down.w" in W:
                    sc = self._conv(x, f"{n}.down", B=B, Hi=h, Wi=w, cin=c_in, cout=cout, stride=s, act=0)
                h, w = h // s, w // s
                x = self._conv(t, f"{n}.conv2", B=B, Hi=h, Wi=w, cin=cout, cout=cout, res=sc)
            feats.append((x, h, w))
        (feat8, h8, w8), (feat16, h16, w16), (feat32, h32, w32) = feats[1:]
        # context path (model.py:104-124)
        avg = self._gate(self._mean(feat32, B=B, HW=h32 * w32, C=512), W["cp.conv_avg.w"], W["cp.conv_avg.b"], act=1)
        sum32 = self._arm(feat32, "cp.arm32", B=B, Hs=h32, Ws=w32, cin=512, t=avg)
        up32 = self._conv(sum32, "cp.conv_head32", B=B, Hi=h32, Wi=w32, cin=128, cout=128, up=1)
        sum16 = self._arm(feat16, "cp.arm16", B=B, Hs=h16, Ws=w16, cin=256, res=up32)
        cp8 = self._conv(sum16, "cp.conv_head16", B=B, Hi=h16, Wi=w16, cin=128, cout=128, up=1)
        # feature fusion (model.py:200-210): f = CBR1x1(cat(feat8, cp8)); f * sigmoid(W2 relu(W1 mean(f))) + f
        f = self._conv(feat8, "ffm.convblk", B=B, Hi=h8, Wi=w8, cin=128, cout=256, taps=1, x2=cp8, c2=128)
        s = self._gate(self._mean(f, B=B, HW=h8 * w8, C=256), W["ffm.conv1.w"], None, W["ffm.conv2.w"], act=2)
        fuse = ops.chan_affine(f, s, f, B=B, HW=h8 * w8, C_=256)
        # head (model.py:44-46, :251) + the pipeline's argmax
        y = self._conv(fuse, "head.conv", B=B, Hi=h8, Wi=w8, cin=256, cout=256)
        lg = self._conv(y, "head.out", B=B, Hi=h8, Wi=w8, cin=256, cout=HEAD_LD, taps=1, act=0, bias=False)
        labels = torch.empty(B, H, Wd, dtype=torch.uint8, device=self.device)
        up = torch.empty(B, self.n_classes, H, Wd, dtype=torch.float32, device=self.device) if logits else None
        ops.parse_head(lg, labels, ncls=self.n_classes, B=B, h=h8, w=w8, H=H, W=Wd, ld=HEAD_LD, logits_out=up)
        return (labels, up) if logits else labels

    def __call__(self, images, logits: bool = False, size: Optional[int] = PARSE_SIZE):
        """``images``: uint8 [B, H, W, 3] / [H, W, 3] tensor (taken as it is), or a PIL image / list of PIL images (RGB,
        resized to ``size`` x ``size`` with PIL's bilinear filter first, as the reference does; ``size=None`` keeps them)"""
        return self.forward(to_pixels(images, size).to(self.device), logits=logits)


def to_pixels(images, size: Optional[int] = PARSE_SIZE) -> torch.Tensor:
    """uint8 [B, H, W, 3] from a tensor or PIL image(s) (the reference's ``raw_image.resize((512, 512), Image.BILINEAR)``)"""
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or images.shape[-1] != 3:
            raise ValueError(f"expected uint8 [..., H, W, 3] pixels (got {images.dtype} {tuple(images.shape)})")
        return (images if images.dim() == 4 else images.unsqueeze(0)).contiguous()
    from PIL import Image
    seq: Sequence = [images] if isinstance(images, Image.Image) else images
    arrs: List[np.ndarray] = []
    for im in seq:
        im = im.convert("RGB")
        if size is not None:
            im = im.resize((size, size), Image.BILINEAR)
        arrs.append(np.asarray(im, dtype=np.uint8))
    return torch.from_numpy(np.stack(arrs))
