"""Plain-torch restatement of the Upsample2D weight fold (cid_upconv_fold_f16) and of the four 2x2 phase convolutions that
csrc/conv3x3.hip runs for it -- shared by the host and the GPU tests of the fold."""
import torch
import torch.nn.functional as F

# along one axis: (parity, folded tap) -> source taps, in summation order
SRC = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def fold_ref(w9: torch.Tensor, round_fp16: bool = True) -> torch.Tensor:
    """w9 [N, 9 * C] (tap = 3 ty + tx, weights._conv3 layout) -> [4 * N, 4 * C]: W4[parity = 2 py + px][n][tap4 = 2 ry + rx][c],
    every entry the fp32 sum of its source taps added one by one, ty-major then tx, rounded to fp16 once"""
    N, C = w9.shape[0], w9.shape[1] // 9
    w = w9.float().reshape(N, 3, 3, C)
    out = torch.empty(2, 2, N, 2, 2, C, dtype=torch.float32)
    for py in (0, 1):
        for px in (0, 1):
            for ry in (0, 1):
                for rx in (0, 1):
                    acc = None
                    for ty in SRC[(py, ry)]:
                        for tx in SRC[(px, rx)]:
                            acc = w[:, ty, tx].clone() if acc is None else acc + w[:, ty, tx]
                    out[py, px, :, ry, rx] = acc
    out = out.reshape(4 * N, 4 * C)
    return out.half() if round_fp16 else out


def phase_conv_ref(x: torch.Tensor, w4: torch.Tensor, bias=None) -> torch.Tensor:
    """x [B, C, H, W] (any float dtype), w4 [4 * N, 4 * C] -> the upsampled convolution [B, N, 2 H, 2 W] in fp32 as four 2x2
    convolutions of the input: parity (py, px), folded tap (ry, rx) reads input pixel (y + ry + py - 1, x + rx + px - 1)"""
    B, C, H, W = x.shape
    N = w4.shape[0] // 4
    k = w4.float().reshape(2, 2, N, 2, 2, C).permute(0, 1, 2, 5, 3, 4)          # [py][px][N][C][ry][rx]
    out = torch.empty(B, N, 2 * H, 2 * W, dtype=torch.float32)
    xp = F.pad(x.float(), (1, 1, 1, 1))
    for py in (0, 1):
        for px in (0, 1):
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], k[py, px])
    if bias is not None:
        out += bias.float()[None, :, None, None]
    return out
