"""ff2 + proj_out of a transformer's tail as one GEMM over the shared [M, 5c] row [ff | h3] on the GPU:
the pitched launches that fill the buffer (bit-identical to their contiguous forms, nothing outside their columns touched),
the folded GEMM at the three variants the benchmark's shape reaches, and one tiny UNet with the fold forced on / off."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import gemm_census
from conftest import max_rel, rel_l2
from test_ff2_fold_host import BENCH_FOLDS, auto_rule, replay, tail_operands, tail_reference     # noqa: F401  (auto_rule: fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7e5a       # an fp16 NaN with a payload (tests/test_gpu_gemm_census.py)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def sentinel(rows, ld, dev):
    return torch.full((rows * ld,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16).view(rows, ld)


def bits(t):
    return t.contiguous().view(torch.int16)


def untouched(t):
    return bool((bits(t) == SENTINEL).all())


# ----------------------------------------------------------------------------- pitched launches
@pytest.mark.parametrize("M,C", [(72, 320),            # one row per wave (layernorm_kernel)
                                 (32768, 320)])        # the smallest launch on layernorm_rows_kernel<8> (M * C = 8 Mi)
def test_layernorm_pitched(dev, M, C):
    from consistentid_amd import ops
    x = rnd(M, C, seed=1, scale=1.5).to(dev)
    g, b = (1 + 0.1 * rnd(C, seed=2).float()).half().to(dev), rnd(C, seed=3, scale=0.1).to(dev)
    want = torch.empty(M, C, dtype=torch.float16, device=dev)
    ops.layernorm(x, want, g, b, M=M, C_=C)
    src, dst = sentinel(M, 5 * C, dev), sentinel(M, 5 * C, dev)
    src[:, 4 * C:] = x                      # where h3 lives in the shared buffer
    before = src.clone()
    ops.layernorm(src[:, 4 * C:], dst[:, C:2 * C], g, b, M=M, C_=C, ldx=5 * C, ldo=5 * C)
    torch.cuda.synchronize()
    assert torch.equal(bits(dst[:, C:2 * C]), bits(want)), "pitched LayerNorm differs from the contiguous launch"
    assert untouched(dst[:, :C]) and untouched(dst[:, 2 * C:]), "columns outside the output block were written"
    assert torch.equal(bits(src), bits(before)), "the input buffer was written"
    # the engine's call: pitched input, contiguous output
    out = torch.empty(M, C, dtype=torch.float16, device=dev)
    ops.layernorm(src[:, 4 * C:], out, g, b, M=M, C_=C, ldx=5 * C)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


def test_id_xattn3_pitched(dev):
    from consistentid_amd import ops, xattn_pack
    from consistentid_amd.weights import LOG2E
    from test_gpu_kernels import _xattn_weights
    B, N, C, heads, Dc, L, n_ip, ip_scale = 2, 128, 320, 8, 768, 81, 4, 0.8
    n_txt, M = L - n_ip, B * N
    W = _xattn_weights(C, Dc, 8, seed=C + heads)
    x = rnd(B, N, C, seed=1, scale=1.5).to(dev)
    e = rnd(B + 1, L, Dc, seed=2).to(dev)
    kvrow = torch.tensor([(i + 1) % (B + 1) for i in range(B)], dtype=torch.int32, device=dev)
    ln = ((1 + 0.1 * rnd(C, seed=3).float()).half().to(dev), rnd(C, seed=4, scale=0.1).to(dev))
    mq = (W["q"] + W["q_up"] @ W["q_down"]) * ((C // heads) ** -0.5 * LOG2E)
    mk, mv = W["k"] + W["k_up"] @ W["k_down"], W["v"] + W["v_up"] @ W["v_down"]
    mo = W["o"] + W["out_up"] @ W["out_down"]
    R = B + 1
    kv_txt = torch.empty(R * L, 2 * C, dtype=torch.float16, device=dev)
    kv_ip = torch.empty(R * L, 2 * C, dtype=torch.float16, device=dev)
    ops.gemm(e, torch.cat([mk, mv]).half().to(dev), kv_txt, M=R * L, N=2 * C, c1=Dc)
    ops.gemm(e, torch.cat([W["kip"], W["vip"]]).half().to(dev), kv_ip, M=R * L, N=2 * C, c1=Dc)
    ke, ve = ops.kv_pack2_elems(C, heads)
    kp = torch.empty(R * ke, dtype=torch.float16, device=dev)
    vp = torch.empty(R * ve, dtype=torch.float16, device=dev)
    ops.kv_pack2(kv_txt, kv_ip, kp, vp, R=R, L=L, C_=C, heads=heads, n_txt=n_txt, n_ip=n_ip, order="reg")
    wq_f, qs, qb = xattn_pack.fold_layernorm(mq.to(dev), ln[0], ln[1])
    wq_p, wo_p = xattn_pack.pack_w3(wq_f), xattn_pack.pack_w3(mo.half().to(dev).contiguous())
    kw = dict(wq_p=wq_p, q_rowsum=qs, q_bias=qb, wo_p=wo_p, bo=W["bo"].half().to(dev), kp=kp, vp=vp, kvrow=kvrow, B=B, N=N, C_=C,
              heads=heads, n_txt=n_txt, n_ip=n_ip, ip_scale=ip_scale, has_ln=True, add_residual=True)
    want = torch.empty(M, C, dtype=torch.float16, device=dev)
    ops.id_xattn3(x, want, **kw)
    buf = sentinel(M, 5 * C, dev)
    ops.id_xattn3(x, buf[:, 4 * C:], ldo=5 * C, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all()
    assert torch.equal(bits(buf[:, 4 * C:]), bits(want)), "pitched id_xattn3 differs from the contiguous launch"
    assert untouched(buf[:, :4 * C]), "columns outside the output block were written"


def test_geglu_pitched(dev, auto_rule):
    """the GEGLU projection writes columns 0 .. 4c of the shared buffer (ldo = 5c) and, with norm3 folded, reads h3 from
    columns 4c .. 5c (ld1 = 5c): for every mode-1 variant the folded levels reach, at the census's smallest descriptor"""
    from consistentid_amd import ops, weights
    fixture = gemm_census.load()
    _, folds = replay(fixture)
    levels = {(wl, M, c) for wl, M, c in folds}
    recs = [(r, p) for wl, rows in fixture.items() for r, p in rows if r["mode"] == 1 and (wl, r["M"], r["c1"]) in levels]
    table = gemm_census.keys_of(recs)
    assert table, "no GEGLU launch found at the folded levels"
    for key, (rec, _) in table.items():
        M, c = rec["M"], rec["c1"]
        assert rec["N"] == 8 * c
        now = dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(dict(rec, ld1=5 * c if rec["has_ln_s"] else c, ldo=5 * c))))
        assert gemm_census.variant_key(rec, now) == key, f"the pitches moved this launch: {gemm_census.variant_key(rec, now)} != {key}"
        print(f"[case] {key}: M={M} c={c}")
        ln = bool(rec["has_ln_s"])
        x = rnd(M, c, seed=1, scale=1.3).to(dev)
        w = weights._geglu_interleave(rnd(8 * c, c, seed=3, scale=c ** -0.5)).contiguous().to(dev)
        bias = weights._geglu_interleave(rnd(8 * c, seed=4, scale=0.3)).contiguous().to(dev)
        kw = dict(M=M, N=8 * c, c1=c, mode=1)
        if ln:
            gamma, beta = (1 + 0.2 * rnd(c, seed=7).float()).half().to(dev), rnd(c, seed=8, scale=0.2).to(dev)
            w, s_, b_ = weights.fold_ln(w.float(), gamma, beta, bias)
            kw["ln"] = (s_.view(torch.float32), b_.view(torch.float32), ops.LN_EPS)
        else:
            kw["bias"] = bias
        want = torch.empty(M, 4 * c, dtype=torch.float16, device=dev)
        ops.gemm(x, w, want, **kw)
        buf = sentinel(M, 5 * c, dev)
        buf[:, 4 * c:] = x
        if ln:
            ops.gemm(buf[:, 4 * c:], w, buf, ld1=5 * c, ldo=5 * c, **kw)
        else:
            ops.gemm(x, w, buf, ldo=5 * c, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all()
        assert torch.equal(bits(buf[:, :4 * c]), bits(want)), f"{key}: pitched GEGLU differs from the contiguous launch"
        assert torch.equal(bits(buf[:, 4 * c:]), bits(x)), f"{key}: the h3 columns were written"


# ----------------------------------------------------------------------------- the folded GEMM
GN_HW = {320: 4096, 640: 1024, 1280: 256}       # tokens per sample at the benchmark's three levels


def smallest_m(c, key, m_max):
    """smallest M (whole samples) at which the folded descriptor still plans to ``key``"""
    for M in range(GN_HW[c], m_max + 1, GN_HW[c]):
        rec = gemm_census.record_of(gn_hw=GN_HW[c], M=M, N=c, c1=5 * c, bias=True, res=True, ldr=c, ws=True, ws_bytes=64 << 20)
        if gemm_census.variant_key(rec, dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(rec)))) == key:
            return M
    raise AssertionError(f"no M <= {m_max} plans to {key}")


@pytest.mark.parametrize("m_bench,c", list(BENCH_FOLDS))
def test_folded_gemm(dev, m_bench, c):
    from consistentid_amd import ops, weights
    key = BENCH_FOLDS[(m_bench, c)]
    M = smallest_m(c, key, m_bench)
    # (c = 320: 128 x 160 unsplit tiles start at M = 16384, but with the three-stage ring -- another variant; the two-stage
    #  ring of the benchmark's launch starts at five samples of 4096 tokens, M = 20480)
    print(f"[case] {key}: M={M} c={c}")
    o = tail_operands(M, c, w_scale=(2 * c) ** -0.5, a_scale=1.0, seed=c)
    d = {k: v.to(dev) for k, v in o.items()}
    ref = tail_reference(d)                                    # fp64 on the GPU
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    # today's pair
    h = torch.empty(M, c, dtype=torch.float16, device=dev)
    ops.gemm(d["ff"], d["w2"], h, M=M, N=c, c1=4 * c, bias=d["b2"], res=d["h3"], ldr=c, ws=ws)
    two = torch.empty(M, c, dtype=torch.float16, device=dev)
    ops.gemm(h, d["wp"], two, M=M, N=c, c1=c, bias=d["bp"], res=d["x"], ldr=c, gn_hw=GN_HW[c])
    # the folded launch from the shared buffer
    w, b = weights.fold_ff2_proj_out(d["w2"], d["b2"], d["wp"], d["bp"])
    buf = torch.cat([d["ff"], d["h3"]], 1).contiguous()

    def run():
        out = sentinel(M + 16, c, dev)[8:8 + M]
        ops.gemm(buf, w, out, M=M, N=c, c1=5 * c, bias=b, res=d["x"], ldr=c, ws=ws, gn_hw=GN_HW[c])
        torch.cuda.synchronize()
        return out
    one, again = run(), run()
    assert torch.isfinite(one.float()).all()
    for name, err in (("max / max|ref|", max_rel), ("rel l2", rel_l2)):
        e1, e2 = err(one, ref), err(two, ref)
        print(f"[ff2 fold] {key} {name}: folded {e1:.3e}, two launches {e2:.3e}, ratio {e1 / e2:.2f}")
        assert e1 <= 1.5 * e2, f"{key}: folded {name} error {e1:.3e} > 1.5 x {e2:.3e}"
    assert torch.equal(bits(one), bits(again)), "the second launch differs"
    stats = getattr(one, "_gn_stats", None)
    assert (stats is not None) == key.endswith("-stats"), f"{key}: statistics attached = {stats is not None}"
    if stats is not None:
        st, rows = stats
        assert tuple(st.shape) == (M // rows, 32, 2)
        t = one.double().reshape(M // rows, rows, 32, c // 32)
        want = torch.stack([t.sum((1, 3)), (t * t).sum((1, 3))], -1)
        # (the bound of test_gemm_emits_groupnorm_statistics: fp32 sums of `rows * c / 32` fp16 values)
        e = float(((st.double() - want).abs() / (want.abs() + rows * (c // 32) * 1e-3)).max())
        print(f"[stats] {key}: {e:.2e}")
        assert e < 2e-5, f"{key}: statistics differ from the tensor they describe: {e:.2e}"
        assert torch.equal(st, again._gn_stats[0]), "the second launch's statistics differ"


# ----------------------------------------------------------------------------- one transformer tail in the engine
def _child(mode, out_path):
    """tiny UNet forward with CID_FF2_FOLD = ``mode`` (this process was started with it): parity against the oracle at the
    project's criterion, the output saved for the parent, the number of folded launches printed"""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from conftest import check_vs_fp16_arm, half_arm
    from consistentid_amd import ops, synth
    from consistentid_amd.unet import HipUNet
    from oracle_utils import build_oracle, make_weights
    assert ops._FF2_FOLD_MODE == mode
    dev = torch.device("cuda:0")
    cfg, sd, ad = make_weights("tiny", rank=8)
    hip = HipUNet(cfg, sd, ad, device=dev)
    oracle = build_oracle("tiny", sd, ad, rank=8)
    inp = synth.random_inputs(cfg, 1, cfg.sample_size * 8, cfg.sample_size * 8)
    ehs = torch.cat([inp["null"], inp["augmented"]])
    lat2 = torch.cat([inp["latents"]] * 2)
    with gemm_census.Recorder() as r:
        out = hip(lat2.to(dev), 981, encoder_hidden_states=ehs.to(dev)).sample
        torch.cuda.synchronize()
    recs = [dict(zip(gemm_census.DESC_FIELDS, d)) for d, _ in r.records]
    folded = sum(1 for rec in recs if rec["mode"] == 0 and rec["taps"] == 1 and rec["c1"] == 5 * rec["N"] and rec["has_res"])
    with torch.no_grad():
        ref = oracle(lat2.float(), 981, ehs.float()).sample
        arm = half_arm(oracle, dev)(lat2.to(dev), 981, ehs.to(dev)).sample
    check_vs_fp16_arm(out, ref, arm, f"tiny UNet, CID_FF2_FOLD={mode}")
    torch.save(out.cpu(), out_path)
    print(f"[ff2 fold] folded launch descriptors: {folded}")


def test_transformer_tail_in_the_engine(dev, tmp_path):
    """CID_FF2_FOLD is read once per process: one child with the fold forced wherever the library takes it, one without.
    The tiny widths run their cross-attention on the first-generation fused kernel, which writes contiguous rows only and
    keeps the tail on two launches; CID_XATTN_FUSED_MAX_C=0 with CID_QATTN=0 sends them down the wider levels' path
    (LayerNorm-folded q GEMM, attention core, out projection with a pitch) in both children."""
    outs = {}
    for mode in ("1", "0"):
        env = dict(os.environ, CID_FF2_FOLD=mode, CID_XATTN_FUSED_MAX_C="0", CID_QATTN="0")
        p = subprocess.run([sys.executable, __file__, mode, str(tmp_path / f"out{mode}.pt")], env=env, capture_output=True,
                           text=True, timeout=300)
        print(p.stdout[-2000:])
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        n = int(p.stdout.rsplit("folded launch descriptors:", 1)[1].split()[0])
        assert (n > 0) == (mode == "1"), f"CID_FF2_FOLD={mode}: {n} folded launches"
        outs[mode] = torch.load(tmp_path / f"out{mode}.pt")
    d = rel_l2(outs["1"], outs["0"])
    print(f"[ff2 fold] tiny UNet, folded vs two launches: rel_l2={d:.3e}")
    # (a figure, not a criterion: each child held the project's criterion against the oracle, and two fp16 paths that are
    #  each ~1.9e-3 from it may sit up to the sum apart)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
