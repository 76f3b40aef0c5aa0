"""numpy model of the long-context cross-attention operands (include/cid.h, cid_kv_pack_long_f16 / cid_kv_pack_long_elems),
shared by tests/test_xattn_long_host.py and tests/test_gpu_xattn_long.py.  Written from the header's index formula, not from
the kernel: key slots in tiles of 32, the ID keys on a tile of their own behind the last text tile."""
import numpy as np
import torch


XL_WAVES = 4             # units -- (sample, head, 32 tokens) -- per workgroup of the core (csrc/xattn_long.hip)
PACK_GRID_CAP = 2048     # blocks of 256 threads cid_kv_pack_long_f16 launches at the most; the rest is a grid-stride loop


def units(B, heads, N):
    """units of one core launch"""
    return B * heads * (N // 32)


def core_blocks(B, heads, N):
    return -(-units(B, heads, N) // XL_WAVES)


def pack_blocks(k_elems, v_elems, R):
    """256-thread blocks that one thread per 16-byte chunk of both images of R context rows would need"""
    return -(-(R * (k_elems + v_elems) // 8) // 256)


def tiles(n_txt, n_ip):
    """(NT text tiles, NK key tiles)"""
    nt = (n_txt + 31) // 32
    return nt, nt + (1 if n_ip > 0 else 0)


def long_elems(C, heads, n_txt, n_ip):
    """halfs of one packed K row / V^T row"""
    d = C // heads
    qks, dvt = (d + 15) // 16, (d + 31) // 32
    nk = tiles(n_txt, n_ip)[1]
    return heads * nk * qks * 512, heads * dvt * 2 * nk * 512


def slot_rows(kv_txt, kv_ip, R, C, n_txt, n_ip):
    """[R, 32 NK, 2 C + 1] fp16: the [K | V] row every key slot reads (zeros for an absent slot), plus a zero column that
    every absent head dim reads"""
    L = n_txt + n_ip
    nt, nk = tiles(n_txt, n_ip)
    t = kv_txt.numpy().reshape(R, L, 2 * C)
    i = kv_ip.numpy().reshape(R, L, 2 * C)
    src = np.zeros((R, 32 * nk, 2 * C + 1), dtype=np.float16)
    src[:, :n_txt, :2 * C] = t[:, :n_txt]
    if n_ip:
        src[:, 32 * nt:32 * nt + n_ip, :2 * C] = i[:, n_txt:]
    return src


def kv_pack_long_ref(kv_txt, kv_ip, R, C, heads, n_txt, n_ip):
    """(K image [R, heads NK QKS 512], V^T image [R, heads DVT 2NK 512]) as torch fp16 on the CPU"""
    d = C // heads
    qks, dvt = (d + 15) // 16, (d + 31) // 32
    nk = tiles(n_txt, n_ip)[1]
    src = slot_rows(kv_txt, kv_ip, R, C, n_txt, n_ip)
    ZERO = 2 * C
    lane, i8 = np.arange(64), np.arange(8)
    idx, hi = lane & 31, lane >> 5
    h = np.arange(heads)[:, None, None, None, None]
    # K [h][kt][kk][lane][i]: slot 32 kt + idx, head dim 16 kk + 8 hi + i
    slot = (np.arange(nk)[:, None] * 32 + idx[None, :])[None, :, None, :, None]
    dc = (np.arange(qks)[:, None] * 16 + hi[None, :] * 8)[None, None, :, :, None] + i8
    col = np.where(dc < d, h * d + dc, ZERO)
    slot, col = np.broadcast_arrays(slot, col)
    kp = src[:, slot, col]
    # V^T [h][dt][ks][lane][i]: head dim 32 dt + idx, slot 16 ks + 4 hi + (i & 3) + 8 (i >> 2)
    dd = (np.arange(dvt)[:, None] * 32 + idx[None, :])[None, :, None, :, None]
    slotv = (np.arange(2 * nk)[:, None] * 16 + 4 * hi[None, :])[None, None, :, :, None] + (i8 & 3) + 8 * (i8 >> 2)
    colv = np.where(dd < d, C + h * d + dd, ZERO)
    slotv, colv = np.broadcast_arrays(slotv, colv)
    vp = src[:, slotv, colv]
    return torch.from_numpy(kp.reshape(R, -1).copy()), torch.from_numpy(vp.reshape(R, -1).copy())
