"""tests/attention_ref.py against the oracle and against itself, on the CPU: the restated processor equals
oracle.processors.Consistent_IPAttProcessor where the oracle's slicing can express the context, the two-stream core and the
self-attention reference agree with a per-row loop, and the index formulas (V^T image, packed K / V^T) put every element
where include/cid.h and csrc/xattn.hip say."""
import pytest
import torch

import attention_ref as ar
from conftest import max_rel, rel_l2
from test_gpu_kernels import _xattn_reference, _xattn_weights, rnd


@pytest.mark.parametrize("ln_res", [False, True])
@pytest.mark.parametrize("C,heads,Dc", [(64, 2, 128), (320, 8, 768)])
@pytest.mark.parametrize("n_txt,n_ip", [(77, 4), (77, 16)])
def test_block_ref_equals_oracle_processor(n_txt, n_ip, C, heads, Dc, ln_res):
    B, N, ip_scale = 2, 48, 0.8
    W = _xattn_weights(C, Dc, 8, seed=C + heads)
    x, ehs = rnd(B, N, C, seed=1, scale=1.5), rnd(B, n_txt + n_ip, Dc, seed=2)
    ln = ((1 + 0.1 * rnd(C, seed=3).float()).half(), rnd(C, seed=4, scale=0.1)) if ln_res else None
    want = _xattn_reference(x, ehs, W, heads, n_ip, ip_scale, ln, residual=ln_res)
    got = ar.xattn_block_ref(x, ehs, W, heads, n_txt, n_ip, ip_scale, ln, ln_res, torch.float32, "cpu")
    e2, em = rel_l2(got, want), max_rel(got, want)
    print(f"[ref] n_txt={n_txt} n_ip={n_ip} C={C}: rel_l2={e2:.2e} max_rel={em:.2e}")
    assert e2 <= 1e-5 and em <= 1e-5


def test_block_ref_without_id_keys_is_the_text_stream():
    """n_ip == 0 (what the oracle's `[:, :end]` slicing cannot express): the text stream alone, whatever ip_scale is --
    equal to the (n_txt, 4) block with ip_scale = 0 on the same text rows"""
    C, heads, Dc, n_txt = 64, 2, 128, 33
    W = _xattn_weights(C, Dc, 8, seed=5)
    x, ehs = rnd(2, 32, C, seed=1), rnd(2, n_txt + 4, Dc, seed=2)
    a = ar.xattn_block_ref(x, ehs[:, :n_txt], W, heads, n_txt, 0, 0.8)
    b = ar.xattn_block_ref(x, ehs, W, heads, n_txt, 4, 0.0)
    assert torch.equal(a, b)
    c = ar.xattn_block_ref(x, ehs, W, heads, n_txt, 4, 0.8)
    assert rel_l2(c, a) > 1e-2          # (and the ID term is really there otherwise)


def test_two_stream_and_self_attention_refs_against_a_row_loop():
    g = torch.Generator().manual_seed(3)
    B, N, heads, d = 2, 6, 2, 8
    q, k, v = (torch.randn(B, N, heads, d, generator=g).half() for _ in range(3))
    for n_keys, causal in ((None, False), (4, False), (1, False), (5, True), (1, True)):
        ref = ar.self_attn_ref(q, k, v, n_keys, causal)
        for b in range(B):
            for h in range(heads):
                for i in range(N):
                    hi = min(N if n_keys is None else n_keys, i + 1 if causal else N)
                    s = (k[b, :hi, h].double() @ q[b, i, h].double())
                    p = torch.exp2(s - s.max())
                    assert torch.allclose(ref[b, i, h], (p / p.sum()) @ v[b, :hi, h].double(), rtol=1e-12, atol=1e-14)
    kt, vt_, ki, vi = (torch.randn(B, n, heads, d, generator=g).half() for n in (5, 5, 3, 3))
    both = ar.two_stream_ref(q, kt, vt_, ki, vi, 0.7)
    txt = ar.two_stream_ref(q, kt, vt_, None, None, 0.7)
    assert torch.equal(txt, ar.two_stream_ref(q, kt, vt_, ki[:, :0], vi[:, :0], 0.7))
    idt = ar.two_stream_ref(q, ki, vi, None, None, 0.0)
    assert torch.allclose(both, txt + 0.7 * idt, rtol=1e-12, atol=1e-14)
    one = ar.two_stream_ref(q, kt[:, :1], vt_[:, :1], None, None, 1.0)
    assert torch.equal(one, vt_[:, :1].double().expand(B, N, heads, d))      # one key: its V row, exactly


def test_vt_image_positions():
    B, N, heads, d, dvp = 2, 48, 3, 40, 64
    v = torch.arange(B * N * heads * d, dtype=torch.float32).reshape(B, N, heads, d).half()
    vt = ar.vt_image(v, dvp)
    assert vt.shape == (B, heads, dvp, N) and (vt[:, :, d:] == 0).all()
    for t in (0, 3, 4, 7, 8, 12, 15, 16, 29, 47):
        pos = (t & ~15) | (8 * ((t >> 2) & 1) + 4 * ((t >> 3) & 1) + (t & 3))
        assert torch.equal(vt[:, :, :d, pos], v[:, t])
    assert sorted(ar.token_pos(N).tolist()) == list(range(N))
    pad = ar.vt_image(v, dvp, pad_value=60000.0, n_keys=21)
    assert torch.equal(pad[..., ar.token_pos(N)[:21]], vt[..., ar.token_pos(N)[:21]])
    assert (pad[:, :, :d][..., ar.token_pos(N)[21:]] == 60000.0).all() and (pad[:, :, d:] == 0).all()


@pytest.mark.parametrize("C,heads,n_txt,n_ip", [(64, 2, 33, 3), (320, 8, 92, 4), (128, 2, 1, 0)])
def test_kv_pack_ref_slots(lib, C, heads, n_txt, n_ip):
    """kv_pack_ref against the slot formulas written out per element, and its sizes against cid_kv_pack_elems"""
    R, L, D = 2, n_txt + n_ip, C // heads
    kv_txt, kv_ip = rnd(R * L, 2 * C, seed=1), rnd(R * L, 2 * C, seed=2)
    kp, vp = ar.kv_pack_ref(kv_txt, kv_ip, R, C, heads, n_txt, n_ip)
    assert kp.shape[1] == lib.cid_kv_pack_elems(C, heads, 0) and vp.shape[1] == lib.cid_kv_pack_elems(C, heads, 1)
    QKS, DVT = (D + 15) // 16, (D + 31) // 32
    kp6, vp6 = kp.reshape(R, heads, 3, QKS, 64, 8), vp.reshape(R, heads, DVT, 6, 64, 8)
    row = lambda r, key: (kv_txt if key < n_txt else kv_ip)[r * L + key]
    g = torch.Generator().manual_seed(0)
    for _ in range(300):
        r, h, kt, kk, lane, i = (int(torch.randint(0, n, (1,), generator=g)) for n in (R, heads, 3, QKS, 64, 8))
        key, dc = kt * 32 + (lane & 31), kk * 16 + (lane >> 5) * 8 + i
        want = row(r, key)[h * D + dc] if key < L and dc < D else 0.0
        assert kp6[r, h, kt, kk, lane, i] == want
        dt, ks = (int(torch.randint(0, n, (1,), generator=g)) for n in (DVT, 6))
        dd, keyv = dt * 32 + (lane & 31), ks * 16 + 4 * (lane >> 5) + (i & 3) + 8 * (i >> 2)
        want = row(r, keyv)[C + h * D + dd] if keyv < L and dd < D else 0.0
        assert vp6[r, h, dt, ks, lane, i] == want
    # every real element appears exactly once, everything else is zero
    assert int((kp != 0).sum()) == int((kv_txt.reshape(R, L, -1)[:, :n_txt, :C] != 0).sum() + (kv_ip.reshape(R, L, -1)[:, n_txt:, :C] != 0).sum())
    assert int((vp != 0).sum()) == int((kv_txt.reshape(R, L, -1)[:, :n_txt, C:] != 0).sum() + (kv_ip.reshape(R, L, -1)[:, n_txt:, C:] != 0).sum())


def test_guards():
    buf = ar.guarded(5, 24, "cpu")
    assert buf.shape == (5 + 2 * ar.GUARD, 24) and not torch.isfinite(buf.float()).any()
    buf[ar.GUARD:ar.GUARD + 5, :16] = 1.0
    ar.guards_intact(buf, 5, 16, "guards")
    for r, c in ((ar.GUARD - 1, 0), (ar.GUARD + 5, 3), (ar.GUARD + 2, 16)):
        bad = buf.clone()
        bad[r, c] = 0.0
        with pytest.raises(AssertionError):
            ar.guards_intact(bad, 5, 16, "guards")
