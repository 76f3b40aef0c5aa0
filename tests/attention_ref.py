"""Plain-PyTorch restatements of the attention kernels' operations, shared by tests/test_gpu_attention_edges.py and
tests/test_attention_ref_host.py: the permuted V^T image, fp64 self-attention (key count, causal), the two-stream identity
cross-attention (core and whole processor, any context split including no ID keys), the packed K / V^T operands of
cid_kv_pack_f16 as an index formula, and the sentinel-guarded output buffers of tests/test_gpu_gemm_census.py."""
import math

import torch
import torch.nn.functional as F

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2

SENTINEL = 0x7e5a       # an fp16 NaN with a payload: unwritten outputs are non-finite, guards compare bit for bit
GUARD = 8               # sentinel rows in front of row 0 and behind the last row


def guarded(rows, ld, dev):
    """[GUARD + rows + GUARD, ld] fp16, every element the sentinel"""
    return torch.full(((rows + 2 * GUARD) * ld,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16).view(rows + 2 * GUARD, ld)


def guards_intact(buf, rows, width, what):
    bits = buf.view(torch.int16).cpu()
    assert (bits[:GUARD] == SENTINEL).all(), f"{what}: rows in front of row 0 were written"
    assert (bits[GUARD + rows:] == SENTINEL).all(), f"{what}: rows behind the last row were written"
    assert (bits[GUARD:GUARD + rows, width:] == SENTINEL).all(), f"{what}: columns beyond the output width were written"


def sentinel_like(n, dev):
    """n fp16 elements, every one the sentinel NaN"""
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)


def token_pos(n):
    """position of token t on the key axis of the V^T image (include/cid.h, cid_self_attn_f16)"""
    t = torch.arange(n)
    return (t & ~15) | (8 * ((t >> 2) & 1) + 4 * ((t >> 3) & 1) + (t & 3))


def vt_image(v, dvp, pad_value=0.0, n_keys=None):
    """v [B, N, heads, d] -> the permuted V^T image [B, heads, dvp, N] (rows d .. dvp - 1 zero).  With n_keys, the columns
    of tokens >= n_keys hold pad_value instead of v"""
    B, N, heads, d = v.shape
    vt = torch.zeros(B, heads, dvp, N, dtype=v.dtype)
    src = v.permute(0, 2, 3, 1).clone()
    if n_keys is not None:
        src[..., n_keys:] = pad_value
    vt[:, :, :d][..., token_pos(N)] = src
    return vt


def self_attn_ref(q, k, v, n_keys=None, causal=False):
    """q, k, v [B, N, heads, d]; q pre-scaled in log2 units.  fp64 softmax2(q k^T) v over keys j < n_keys (and j <= i when
    causal) -> [B, N, heads, d]"""
    qd, kd, vd = q.double(), k.double(), v.double()
    N = q.shape[1]
    s = torch.einsum("bihd,bjhd->bhij", qd, kd)
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    hidden = j >= (N if n_keys is None else n_keys)
    if causal:
        hidden = hidden | (j > i)
    s = s.masked_fill(hidden, -float("inf"))
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s * LN2, -1), vd)


def _softmax2_pv(qd, k, v):
    s = torch.einsum("bihd,bjhd->bhij", qd, k.double())
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s * LN2, -1), v.double())


def two_stream_ref(q, k_txt, v_txt, k_ip, v_ip, ip_scale):
    """q [B, N, heads, d] (log2 units), k / v [B, n, heads, d]: fp64 softmax2(q Kt^T) Vt + ip_scale * softmax2(q Kip^T) Vip;
    the ID term is absent when there are no ID keys (k_ip None or empty)"""
    qd = q.double()
    o = _softmax2_pv(qd, k_txt, v_txt)
    if k_ip is not None and k_ip.shape[1] > 0:
        o = o + ip_scale * _softmax2_pv(qd, k_ip, v_ip)
    return o


def merged_xattn_weights(W, d):
    """LoRA-merged projections of the processor (fp32): query (with d^-0.5 * log2(e) folded in), key, value, output"""
    mq = (W["q"] + W["q_up"] @ W["q_down"]) * (d ** -0.5 * LOG2E)
    mk, mv = W["k"] + W["k_up"] @ W["k_down"], W["v"] + W["v_up"] @ W["v_down"]
    mo = W["o"] + W["out_up"] @ W["out_down"]
    return mq, mk, mv, mo


def xattn_block_ref(x, ehs, W, heads, n_txt, n_ip, ip_scale, ln=None, residual=False, dtype=torch.float64, device="cpu"):
    """The whole identity cross-attention processor on x [B, N, C] and ehs [B, n_txt + n_ip, Dc]: optional LayerNorm,
    LoRA-merged projections, the two softmaxes over text and ID keys (the ID term absent when n_ip == 0), Wo, bo, optional
    residual -- in `dtype` on `device` (fp64 / fp32 on the CPU: reference; fp16 on the GPU: the stock-precision arm)"""
    C = x.shape[-1]
    d = C // heads
    assert ehs.shape[1] == n_txt + n_ip
    c = lambda t: t.to(device).to(dtype)
    mq, mk, mv, mo = (c(w) for w in merged_xattn_weights(W, d))
    h = c(x)
    if ln is not None:
        h = F.layer_norm(h, (C,), c(ln[0]), c(ln[1]), 1e-5)
    e = c(ehs)
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, d).transpose(1, 2)
    qh = sp(h @ mq.T)                                       # log2 units: softmax2(s) = softmax(s * ln 2)

    def stream(rows, wk, wv):
        p = torch.softmax((qh @ sp(rows @ wk.T).transpose(-1, -2)) * LN2, -1)
        return p @ sp(rows @ wv.T)

    o = stream(e[:, :n_txt], mk, mv)
    if n_ip > 0:
        o = o + ip_scale * stream(e[:, n_txt:], c(W["kip"]), c(W["vip"]))
    o = o.transpose(1, 2).reshape(x.shape) @ mo.T + c(W["bo"])
    if residual:
        o = o + c(x)
    return o


def kv_pack_ref(kv_txt, kv_ip, R, C, heads, n_txt, n_ip):
    """the packed operands of cid_kv_pack_f16 from [R * L, 2 C] rows of [K | V] (text projection / ID projection), as an index
    formula: K image [R][heads][3 key tiles][ceil(d / 16)][64 lanes][8], lane (idx, hi) holds key 32 kt + idx, head dims
    16 kk + 8 hi ..; V^T image [R][heads][ceil(d / 32)][6][64 lanes][8], lane (idx, hi) holds head dim 32 dt + idx, keys
    16 ks + 4 hi + (i & 3) + 8 (i >> 2).  Slots of keys >= n_txt + n_ip and head dims >= d are zero."""
    L, D = n_txt + n_ip, C // heads
    QKS, DVT = (D + 15) // 16, (D + 31) // 32
    src = torch.zeros(R, 96, 2 * C, dtype=torch.float16)
    src[:, :n_txt] = kv_txt.reshape(R, L, 2 * C)[:, :n_txt]
    src[:, n_txt:L] = kv_ip.reshape(R, L, 2 * C)[:, n_txt:]
    src = torch.cat([src, torch.zeros(R, 96, 1, dtype=torch.float16)], -1)          # column 2 C: the zero every absent slot reads
    ZERO = 2 * C
    lane, i8 = torch.arange(64), torch.arange(8)
    idx, hi = lane & 31, lane >> 5
    # K
    h, kt, kk = torch.arange(heads), torch.arange(3), torch.arange(QKS)
    key = (kt[:, None] * 32 + idx[None, :])[None, :, None, :, None]                 # [1, 3, 1, 64, 1]
    dc = (kk[:, None] * 16 + hi[None, :] * 8)[None, None, :, :, None] + i8          # [1, 1, QKS, 64, 8]
    col = torch.where(dc < D, h[:, None, None, None, None] * D + dc, ZERO)
    key, col = torch.broadcast_tensors(key, col)
    kp = src[:, key, col]
    # V^T
    dt, ks = torch.arange(DVT), torch.arange(6)
    dd = (dt[:, None] * 32 + idx[None, :])[None, :, None, :, None]                  # [1, DVT, 1, 64, 1]
    keyv = (ks[:, None] * 16 + 4 * hi[None, :])[None, None, :, :, None] + (i8 & 3) + 8 * (i8 >> 2)
    colv = torch.where(dd < D, C + h[:, None, None, None, None] * D + dd, ZERO)
    keyv, colv = torch.broadcast_tensors(keyv, colv)
    vp = src[:, keyv, colv]
    return kp.reshape(R, -1), vp.reshape(R, -1)
