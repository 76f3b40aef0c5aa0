"""The parity body of a cid_gemm_f16 launch given by a census record (test helper, not a conftest).

``run_case(dev, key, rec, plan)`` takes a record of tests/gemm_census.py (the descriptor's integers and operand presence) and
the plan it is expected on: the record must still plan to ``key``; operands are fp16-representable random tensors at the
recorded pitches; the launch goes into a sentinel-filled output with guard rows / columns and is checked against a plain
PyTorch CPU reference of the operation at the project's default tolerances; guards bit-untouched, second launch bit-identical,
statistics / second destination consistent.  tests/test_gpu_gemm_census.py runs it on every recorded variant,
tests/test_gpu_conv_rect.py on the fast 3x3 convolution variants at non-square geometry."""
import torch
import torch.nn.functional as F

import gemm_census
from conftest import check_close, check_vs_fp16_arm

SENTINEL = 0x7e5a       # an fp16 NaN with a payload: unwritten outputs are non-finite, guards compare bit for bit
GUARD = 8               # sentinel rows in front of row 0 and behind row M - 1
PAD_COLS = 32           # sentinel columns beyond the output width where the recorded pitch leaves none


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def _guarded(rows, ld, dev):
    """[GUARD + rows + GUARD, ld] fp16, every element the sentinel"""
    return torch.full(((rows + 2 * GUARD) * ld,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16).view(rows + 2 * GUARD, ld)


def _guards_intact(buf, rows, width, what):
    bits = buf.view(torch.int16).cpu()
    assert (bits[:GUARD] == SENTINEL).all(), f"{what}: rows in front of row 0 were written"
    assert (bits[GUARD + rows:] == SENTINEL).all(), f"{what}: rows behind row M - 1 were written"
    assert (bits[GUARD:GUARD + rows, width:] == SENTINEL).all(), f"{what}: columns beyond the output width were written"


def _conv_ref(x, w, rec, B):
    """x [B * Hi * Wi, C] tokens, w [N, 9 * C] (tap-major) -> [M, N] tokens of the 3x3 convolution the descriptor describes"""
    C = x.shape[1]
    img = x.reshape(B, rec["Hi"], rec["Wi"], C).permute(0, 3, 1, 2)
    if rec["up"]:
        img = F.interpolate(img, scale_factor=2.0, mode="nearest")
    w4 = w.reshape(rec["N"], 3, 3, C).permute(0, 3, 1, 2)
    if rec["pad_mode"] == 1:
        y = F.conv2d(F.pad(img, (0, 1, 0, 1)), w4, stride=2, padding=0)
    else:
        y = F.conv2d(img, w4, stride=rec["stride"], padding=1)
    assert tuple(y.shape[-2:]) == (rec["Ho"], rec["Wo"]), (tuple(y.shape), rec)
    return y.permute(0, 2, 3, 1).reshape(-1, rec["N"])


def _vt_image(vt, B, heads, d, dvp, ntok):
    """the transposed-V buffer -> [B, heads, ntok, d] (position formula of test_qkv_gemm_and_self_attention)"""
    t = torch.arange(ntok)
    pos = (t & ~15) | (8 * ((t >> 2) & 1) + 4 * ((t >> 3) & 1) + (t & 3))
    return vt.reshape(B, heads, dvp, ntok)[:, :, :d, :].cpu()[..., pos].transpose(-1, -2)


def run_case(dev, key, rec, plan):
    """-> (the [M, n_out] view of the first launch's output, its statistics ``(fp32 [M / rows, 32, 2], rows)`` or None)"""
    from consistentid_amd import ops, weights
    # 1. the planner still sends this shape to this variant
    now = dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(rec)))
    assert gemm_census.variant_key(rec, now) == key, f"the planner moved this shape: {gemm_census.variant_key(rec, now)}\n{rec}\n{now}"
    M, N, c1, c2, taps, mode = (rec[k] for k in ("M", "N", "c1", "c2", "taps", "mode"))
    K = taps * (c1 + c2)
    ln = bool(rec["has_ln_s"])
    dt = torch.float64 if ln else torch.float32          # (the LayerNorm-fold tests of this suite take fp64)
    B = M // (rec["Ho"] * rec["Wo"]) if taps == 9 else 1
    rows_in = B * rec["Hi"] * rec["Wi"] if taps == 9 else M
    print(f"[case] {key}: M={M} N={N} K={K} ({rows_in} input rows)")

    # 2. operands (fp16-representable), at the recorded pitches
    x1 = _rnd(rows_in, rec["ld1"], seed=1, scale=1.3 if ln else 1.0)
    x2 = _rnd(rows_in, rec["ld2"], seed=2) if c2 else None
    w = _rnd(N, K, seed=3, scale=K ** -0.5)
    with_bias = bool(rec["has_bias"]) or (ln and mode != 2)       # (folded forms carry their bias inside ln_b)
    bias = _rnd(N, seed=4, scale=0.3 if ln else 1.0) if with_bias else None
    rps = rec["rows_per_sample"] if rec["rows_per_sample"] > 0 else 1
    rowbias = _rnd((M + rps - 1) // rps, max(rec["ld_rowbias"], N), seed=5) if rec["has_rowbias"] else None
    res = _rnd(M, rec["ldr"], seed=6) if rec["has_res"] else None
    gamma = (1 + 0.2 * _rnd(c1, seed=7).float()).half() if ln else None
    beta = _rnd(c1, seed=8, scale=0.2) if ln else None

    # 3. the reference: the same operation in plain PyTorch on the CPU
    def reference(cast, device):
        c = lambda t: t.to(device).to(cast)
        x = c(x1)[:, :c1] if c2 == 0 else torch.cat([c(x1)[:, :c1], c(x2)[:, :c2]], 1)
        if ln:
            x = F.layer_norm(x, (c1,), c(gamma), c(beta), ops.LN_EPS)
        y = _conv_ref(x, c(w).reshape(N, 9, c1 + c2), rec, B) if taps == 9 else x @ c(w).T
        if bias is not None:
            y = y + c(bias)
        if rowbias is not None:
            y = y + c(rowbias)[:, :N].repeat_interleave(rps, 0)[:M]
        if res is not None:
            y = y + c(res)[:, :N]
        if rec["act"]:
            y = F.relu(y)
        if mode == 1:
            h, gate = y.chunk(2, dim=-1)
            y = h * F.gelu(gate)
        return y
    ref = reference(dt, "cpu")
    arm = reference(torch.float16, dev) if (ln or mode == 2) else None

    # 4. the launch: sentinel-filled output with guard rows and columns, twice
    n_out = N // 2 if mode == 1 else (rec["n_vt0"] if mode == 2 else N)
    ldo = rec["ldo"] if rec["ldo"] > n_out else n_out + PAD_COLS
    wk, bk = w, bias
    if mode == 1:
        wk, bk = weights._geglu_interleave(w).contiguous(), (weights._geglu_interleave(bias).contiguous() if bias is not None else None)
    kw = dict(M=M, N=N, c1=c1, ld1=rec["ld1"], c2=c2, ld2=rec["ld2"], ldo=ldo, taps=taps, Hi=rec["Hi"], Wi=rec["Wi"], Ho=rec["Ho"],
              Wo=rec["Wo"], stride=rec["stride"], up=rec["up"], mode=mode, pad_mode=rec["pad_mode"], act=rec["act"],
              gn_hw=rec["gn_hw"], rows_per_sample=rec["rows_per_sample"])
    if ln:
        wl, s_, b_ = weights.fold_ln(wk.float().to(dev), gamma.to(dev), beta.to(dev), bk.to(dev) if bk is not None else None)
        wk, bk = wl, None
        kw["ln"] = (s_.view(torch.float32), b_.view(torch.float32), ops.LN_EPS)
    wk = wk.to(dev)
    if c2:
        kw["x2"] = x2.to(dev)
    if bk is not None:
        kw["bias"] = bk.to(dev)
    if rowbias is not None:
        kw.update(rowbias=rowbias.to(dev), ld_rowbias=rowbias.shape[1])
    if res is not None:
        kw.update(res=res.to(dev), ldr=rec["ldr"])
    if rec["has_ws"]:
        kw["ws"] = torch.empty(rec["ws_bytes"], dtype=torch.uint8, device=dev)
    if rec["has_w_up4"]:
        kw["w_up4"] = ops.upconv_fold(wk)
    heads, d, dvp, ntok = rec["heads"], rec["dhead"], rec["dvp"], rec["ntok"]
    if mode == 2:
        kw.update(n_vt0=rec["n_vt0"], heads=heads, dhead=d, ntok=ntok)
        Bq, vt_elems = M // ntok, (M // ntok) * heads * dvp * ntok
    x1d = x1.to(dev)
    runs = []
    for _ in range(2):
        buf = _guarded(M, ldo, dev)
        buf2 = _guarded(M, ldo, dev) if rec["has_out2"] else None
        out = buf[GUARD:GUARD + M]
        if buf2 is not None:
            kw["out2"] = buf2[GUARD:GUARD + M]
        vtbuf = None
        if mode == 2:
            vtbuf = torch.full((vt_elems + 2 * GUARD * ntok,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
            kw["vt"] = vtbuf[GUARD * ntok:GUARD * ntok + vt_elems]
        ops.gemm(x1d, wk, out, **kw)
        torch.cuda.synchronize()
        runs.append((buf, buf2, vtbuf, getattr(out, "_gn_stats", None)))
    buf, buf2, vtbuf, stats = runs[0]
    got = buf[GUARD:GUARD + M, :n_out]

    # 5. parity at the project's tolerances
    if arm is not None:
        check_vs_fp16_arm(got, ref[:, :n_out], arm[:, :n_out], key)
    else:
        check_close(got, ref, key)
    if mode == 2:
        v_ref = ref[:, n_out:].reshape(Bq, ntok, heads, d).transpose(1, 2)
        v_arm = arm[:, n_out:].reshape(Bq, ntok, heads, d).transpose(1, 2)
        got_v = _vt_image(vtbuf[GUARD * ntok:GUARD * ntok + vt_elems], Bq, heads, d, dvp, ntok)
        check_vs_fp16_arm(got_v, v_ref, v_arm, key + " (v^T image)")

    # 6. guards untouched, second launch bit-identical, statistics / second destination consistent
    _guards_intact(buf, M, n_out, key)
    if mode == 2:
        vb = vtbuf.view(torch.int16).cpu()
        assert (vb[:GUARD * ntok] == SENTINEL).all() and (vb[GUARD * ntok + vt_elems:] == SENTINEL).all(), f"{key}: v^T guards were written"
    again = runs[1]
    assert torch.equal(buf.view(torch.int16), again[0].view(torch.int16)), f"{key}: the second launch differs"
    if mode == 2:
        assert torch.equal(vtbuf.view(torch.int16), again[2].view(torch.int16)), f"{key}: the second launch's v^T differs"
    if buf2 is not None:
        _guards_intact(buf2, M, n_out, key + " (out2)")
        assert torch.equal(buf2.view(torch.int16), buf.view(torch.int16)), f"{key}: out2 differs from out"
    assert (stats is not None) == bool(plan["stats"]), f"{key}: statistics attached = {stats is not None}, the plan says {plan['stats']}"
    if stats is not None:
        st, rows = stats
        assert rows == plan["stats_rows"] and tuple(st.shape) == (M // rows, 32, 2)
        o = got.double().cpu()
        if gemm_census.families()[plan["family"]] == "conv_h32_phase":
            # a statistics block is a tile: `rows` outputs of ONE parity of one image (image-major: image, parity, block)
            o = o.reshape(B, rec["Hi"], 2, rec["Wi"], 2, N).permute(0, 2, 4, 1, 3, 5)
        o = o.reshape(M // rows, rows, 32, N // 32)
        want = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
        # (the bound of test_gemm_emits_groupnorm_statistics: fp32 sums of `rows * N / 32` fp16 values)
        err = ((st.double().cpu() - want).abs() / (want.abs() + rows * (N // 32) * 1e-3)).max()
        print(f"[stats] {key}: {float(err):.2e}")
        assert err < 2e-5, f"{key}: statistics differ from the tensor they describe: {float(err):.2e}"
        assert torch.equal(st, again[3][0]), f"{key}: the second launch's statistics differ"
    return got, stats
