"""Test helper: a plain-PyTorch restatement of the 19-class BiSeNet face parser, written from its architecture (ResNet-18
backbone, attention-refinement and feature-fusion modules, main head; BatchNorm in eval mode), plus random checkpoints
that carry the real key names and shapes.  It is the checker of consistentid_amd.face_parsing, never product code."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
LAYERS = ((64, 64, 1), (64, 128, 2), (128, 256, 2), (256, 512, 2))


def _bn_keys(sd, p, c, g):
    sd[f"{p}.weight"] = torch.rand(c, generator=g) + 0.5                   # gamma ~ U(0.5, 1.5)
    sd[f"{p}.bias"] = (torch.rand(c, generator=g) - 0.5) * 0.4
    sd[f"{p}.running_mean"] = torch.randn(c, generator=g) * 0.1
    sd[f"{p}.running_var"] = torch.rand(c, generator=g) + 0.5
    sd[f"{p}.num_batches_tracked"] = torch.tensor(0)


def _conv(sd, k, o, i, ks, g):
    sd[f"{k}.weight"] = torch.randn(o, i, ks, ks, generator=g) / (i * ks * ks) ** 0.5


def random_state_dict(n_classes: int = 19, seed: int = 0, aux_heads: bool = True) -> Dict[str, torch.Tensor]:
    """a face_parsing.pth-shaped state dict (fp32, CPU) with random weights"""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    _conv(sd, "cp.resnet.conv1", 64, 3, 7, g)
    _bn_keys(sd, "cp.resnet.bn1", 64, g)
    for li, (cin, cout, stride) in enumerate(LAYERS, start=1):
        for bi in range(2):
            n = f"cp.resnet.layer{li}.{bi}"
            ci = cin if bi == 0 else cout
            _conv(sd, f"{n}.conv1", cout, ci, 3, g)
            _bn_keys(sd, f"{n}.bn1", cout, g)
            _conv(sd, f"{n}.conv2", cout, cout, 3, g)
            _bn_keys(sd, f"{n}.bn2", cout, g)
            if bi == 0 and (cin != cout or stride != 1):
                _conv(sd, f"{n}.downsample.0", cout, cin, 1, g)
                _bn_keys(sd, f"{n}.downsample.1", cout, g)
    for n, c in (("cp.arm16", 256), ("cp.arm32", 512)):
        _conv(sd, f"{n}.conv.conv", 128, c, 3, g)
        _bn_keys(sd, f"{n}.conv.bn", 128, g)
        _conv(sd, f"{n}.conv_atten", 128, 128, 1, g)
        _bn_keys(sd, f"{n}.bn_atten", 128, g)
    for n in ("cp.conv_head32", "cp.conv_head16"):
        _conv(sd, f"{n}.conv", 128, 128, 3, g)
        _bn_keys(sd, f"{n}.bn", 128, g)
    _conv(sd, "cp.conv_avg.conv", 128, 512, 1, g)
    _bn_keys(sd, "cp.conv_avg.bn", 128, g)
    _conv(sd, "ffm.convblk.conv", 256, 256, 1, g)
    _bn_keys(sd, "ffm.convblk.bn", 256, g)
    _conv(sd, "ffm.conv1", 64, 256, 1, g)
    _conv(sd, "ffm.conv2", 256, 64, 1, g)
    heads = [("conv_out", 256, 256)] + ([("conv_out16", 128, 64), ("conv_out32", 128, 64)] if aux_heads else [])
    for n, cin, mid in heads:
        _conv(sd, f"{n}.conv.conv", mid, cin, 3, g)
        _bn_keys(sd, f"{n}.conv.bn", mid, g)
        _conv(sd, f"{n}.conv_out", n_classes, mid, 1, g)
    return sd


class _Net:
    """functional forward over a state dict; ``calibrate=True`` first sets every BatchNorm's running statistics to the
    batch statistics it sees (pooled 1x1 inputs: mean 0 and the mean square over the channels), so that a random
    network keeps its activations O(1)"""

    def __init__(self, sd, dtype=torch.float32, calibrate=False):
        self.sd, self.dtype, self.calibrate = sd, dtype, calibrate

    def w(self, k):
        return self.sd[f"{k}.weight"].to(self.dtype)

    def bn(self, x, p):
        sd = self.sd
        if self.calibrate:
            if x.shape[2] * x.shape[3] > 1:
                m, v = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
            else:
                m, v = torch.zeros_like(x[0, :, 0, 0]), x.pow(2).mean().expand(x.shape[1]).clone()
            sd[f"{p}.running_mean"], sd[f"{p}.running_var"] = m.float().clone(), v.float().clamp_min(1e-4).clone()
        c = lambda k: sd[f"{p}.{k}"].to(self.dtype)
        return F.batch_norm(x, c("running_mean"), c("running_var"), c("weight"), c("bias"), False, 0.0, 1e-5)

    def cbr(self, x, p, stride=1, pad=1):
        return F.relu(self.bn(F.conv2d(x, self.w(f"{p}.conv"), stride=stride, padding=pad), f"{p}.bn"))

    def block(self, x, n, stride):
        r = F.relu(self.bn(F.conv2d(x, self.w(f"{n}.conv1"), stride=stride, padding=1), f"{n}.bn1"))
        r = self.bn(F.conv2d(r, self.w(f"{n}.conv2"), padding=1), f"{n}.bn2")
        sc = x
        if f"{n}.downsample.0.weight" in self.sd:
            sc = self.bn(F.conv2d(x, self.w(f"{n}.downsample.0"), stride=stride), f"{n}.downsample.1")
        return F.relu(r + sc)

    def arm(self, x, n):
        f = self.cbr(x, f"{n}.conv")
        a = F.avg_pool2d(f, f.shape[2:])
        a = torch.sigmoid(self.bn(F.conv2d(a, self.w(f"{n}.conv_atten")), f"{n}.bn_atten"))
        return f * a

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] -> upsampled logits [B, n_classes, H, W] (the main head)"""
        x = img.permute(0, 3, 1, 2).to(self.dtype) / 255
        c = lambda v: torch.tensor(v, dtype=self.dtype, device=x.device).view(1, 3, 1, 1)
        x = (x - c(MEAN)) / c(STD)
        H, W = x.shape[2:]
        x = F.relu(self.bn(F.conv2d(x, self.w("cp.resnet.conv1"), stride=2, padding=3), "cp.resnet.bn1"))
        x = F.max_pool2d(x, 3, 2, 1)
        feats = []
        for li, (_, _, stride) in enumerate(LAYERS, start=1):
            x = self.block(x, f"cp.resnet.layer{li}.0", stride)
            x = self.block(x, f"cp.resnet.layer{li}.1", 1)
            feats.append(x)
        feat8, feat16, feat32 = feats[1:]
        avg = self.cbr(F.avg_pool2d(feat32, feat32.shape[2:]), "cp.conv_avg", pad=0)
        s32 = self.arm(feat32, "cp.arm32") + F.interpolate(avg, feat32.shape[2:], mode="nearest")
        up32 = self.cbr(F.interpolate(s32, feat16.shape[2:], mode="nearest"), "cp.conv_head32")
        s16 = self.arm(feat16, "cp.arm16") + up32
        cp8 = self.cbr(F.interpolate(s16, feat8.shape[2:], mode="nearest"), "cp.conv_head16")
        f = self.cbr(torch.cat([feat8, cp8], 1), "ffm.convblk", pad=0)
        a = F.avg_pool2d(f, f.shape[2:])
        a = torch.sigmoid(F.conv2d(F.relu(F.conv2d(a, self.w("ffm.conv1"))), self.w("ffm.conv2")))
        f = f * a + f
        y = self.cbr(f, "conv_out.conv")
        y = F.conv2d(y, self.w("conv_out.conv_out"))
        return F.interpolate(y, (H, W), mode="bilinear", align_corners=True)


def forward(sd, img: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    with torch.no_grad():
        return _Net(sd, dtype).forward(img)


def calibrate(sd, img: torch.Tensor) -> None:
    """set every BatchNorm's running statistics from one pass over ``img`` (in place)"""
    with torch.no_grad():
        _Net(sd, torch.float32, calibrate=True).forward(img)


def make_image(B: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """smooth random uint8 RGB [B, H, W, 3]: low-frequency blobs plus noise, so that neighbouring pixels correlate"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(H // 32, 2), max(W // 32, 2), generator=g)
    x = F.interpolate(low, (H, W), mode="bilinear", align_corners=False) * 200 + torch.rand(B, 3, H, W, generator=g) * 55
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
