"""ff2 + proj_out of a transformer's tail as one GEMM (weights.fold_ff2_proj_out, ops.ff2_fold): the algebra in the
arithmetic of the kernels (fp16 operands, fp32 accumulation, one fp16 rounding per stored tensor) against fp64, and the rule
that decides where the engine folds, replayed over the census of the models' GEMM launches (tests/golden/gemm_calls.json)
without a GPU."""
import pytest
import torch

import gemm_census
from conftest import max_rel, rel_l2

# the three folded launches of the benchmark's shape (SD1.5, 512 x 512, CFG batch 8): (M, c) -> variant key
BENCH_FOLDS = {
    (32768, 320): "igemm-128x160-nb2-m0-t1-bias-res-stats",
    (8192, 640): "igemm-128x160-nb3-m0-t1-bias-res-stats",
    (2048, 1280): "igemm-256x160-nb3-m0-t1-sk-bias-res",
}


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def tail_operands(M, c, w_scale, a_scale, seed=0):
    """fp16 operands of a transformer tail: ff [M, 4c], h3 [M, c], x [M, c], W2 [c, 4c], b2, Wp [c, c], bp"""
    return dict(ff=_rnd(M, 4 * c, seed=seed + 1, scale=a_scale), h3=_rnd(M, c, seed=seed + 2, scale=a_scale),
                x=_rnd(M, c, seed=seed + 3, scale=a_scale), w2=_rnd(c, 4 * c, seed=seed + 4, scale=w_scale),
                b2=_rnd(c, seed=seed + 5, scale=0.1), wp=_rnd(c, c, seed=seed + 6, scale=w_scale), bp=_rnd(c, seed=seed + 7, scale=0.1))


def tail_reference(o):
    """out = Wp (W2 ff + b2 + h3) + bp + x in fp64 from the fp16 operands"""
    d = {k: v.double() for k, v in o.items()}
    h = d["ff"] @ d["w2"].T + d["b2"] + d["h3"]
    return h @ d["wp"].T + d["bp"] + d["x"]


@pytest.mark.parametrize("c", [320, 640, 1280])
@pytest.mark.parametrize("w_scale,a_scale", [(0.02, 1.0), (0.05, 4.0)])
def test_fold_algebra_in_kernel_arithmetic(c, w_scale, a_scale):
    from consistentid_amd import weights
    M = 256
    o = tail_operands(M, c, w_scale, a_scale, seed=c)
    ref = tail_reference(o)
    f = {k: v.float() for k, v in o.items()}
    # the two launches of the unfolded path: fp32 accumulation, h and out rounded to fp16
    h = (f["ff"] @ f["w2"].T + f["b2"] + f["h3"]).half()
    two = (h.float() @ f["wp"].T + f["bp"] + f["x"]).half()
    # the folded launch on the weights as shipped
    w, b = weights.fold_ff2_proj_out(o["w2"], o["b2"], o["wp"], o["bp"])
    assert w.dtype == torch.float16 and tuple(w.shape) == (c, 5 * c) and tuple(b.shape) == (c,)
    assert torch.equal(w[:, 4 * c:], o["wp"]), "the h3 columns of W' are proj_out's weights themselves"
    row = torch.cat([f["ff"], f["h3"]], 1)
    one = (row @ w.float().T + b.float() + f["x"]).half()
    sub = float(((w != 0) & (w.abs() < 2.0 ** -14)).float().mean())
    for name, err in (("max / max|ref|", max_rel), ("rel l2", rel_l2)):
        e1, e2 = err(one, ref), err(two, ref)
        print(f"[ff2 fold] c={c} w={w_scale} a={a_scale} {name}: folded {e1:.3e}, two launches {e2:.3e}, ratio {e1 / e2:.2f}")
        assert e1 <= 1.5 * e2, f"c={c}: folded {name} error {e1:.3e} > 1.5 x {e2:.3e}"
    print(f"[ff2 fold] c={c} w={w_scale}: {100 * sub:.2f} % of W' in the fp16 subnormal range")
    assert sub < 0.05


# ----------------------------------------------------------------------------- the rule, over the census
def _is_tail_linear(rec):
    return (rec["mode"] == 0 and rec["taps"] == 1 and rec["c2"] == 0 and rec["has_bias"] and rec["has_res"]
            and rec["N"] in (320, 640, 1280) and not rec["has_out2"] and not rec["has_rowbias"])


def _gen1_xattn(M, c):
    """does the first-generation fused kernel produce h3 at this level of the census workloads?  It has no pitched form and
    the engine does not fold there.  The engine's own predicates at the default switches: the third generation serves its
    geometry (eight heads at 320 channels in SD1.5, with the 77 + 4 and the 81 + 0 context alike), unet.fused_gen1 decides
    the rest."""
    from consistentid_amd import ops, unet
    return not ops.id_xattn3_supported(c, 8, 77, 4) and unet.fused_gen1(c, M)


def replay(fixture):
    """-> (keys the models reach with the fold on, {(workload, M, c): folded key}).  ff2 is the c x 4c linear with bias,
    residual and the split-K workspace; proj_out the c x c one that announces a GroupNorm consumer (gn_hw > 0).
    An approximation of the engine, by shape: at the padded-token sizes proj_out passes gn_hw = 0 and its record is the
    attention out projections' too, so there the ff2 record is folded (without statistics, as the engine does) and the
    c x c key stays, which the out projections reach anyway.  The check on the real launch sequence is
    tests/test_gpu_gemm_census.py::test_census_reproduces_fixture, which runs with the fold on."""
    from consistentid_amd import ops
    after, folds = set(), {}
    for wl, rows in fixture.items():
        unet = wl.startswith("sd")
        one_layer = wl.startswith("sd15")        # SDXL's transformers have 2 / 10 blocks: only the last ff2 goes
        po = {(r["M"], r["N"]): r["gn_hw"] for r, _ in rows
              if _is_tail_linear(r) and r["c1"] == r["N"] and r["gn_hw"] > 0 and not r["has_ws"]}
        for rec, plan in rows:
            key = gemm_census.variant_key(rec, plan)
            M, c = rec["M"], rec["N"]
            if unet and _is_tail_linear(rec) and rec["c1"] == 4 * c and rec["has_ws"]:
                gn_hw = po.get((M, c), 0)
                if ops.ff2_fold(M, c, gn_hw) and not _gen1_xattn(M, c):
                    frec = gemm_census.record_of(gn_hw=gn_hw, M=M, N=c, c1=5 * c, bias=True, res=True, ldr=c, ws=True,
                                                 ws_bytes=rec["ws_bytes"])
                    fplan = dict(zip(gemm_census.PLAN_FIELDS, gemm_census.plan_of(frec)))
                    folds[(wl, M, c)] = gemm_census.variant_key(frec, fplan)
                    after.add(folds[(wl, M, c)])
                    if one_layer:
                        continue
            elif (unet and _is_tail_linear(rec) and rec["c1"] == c and rec["gn_hw"] > 0 and not rec["has_ws"]
                  and ops.ff2_fold(M, c, rec["gn_hw"]) and not _gen1_xattn(M, c)):
                continue                        # proj_out of a folded tail
            after.add(key)
    return after, folds


@pytest.fixture
def auto_rule(lib):
    """the default rule, whatever CID_FF2_FOLD this process started with (the value is read once per process)"""
    from consistentid_amd import ops
    mode = ops._FF2_FOLD_MODE
    ops._FF2_FOLD_MODE = "auto"
    ops.ff2_fold.cache_clear()
    yield
    ops._FF2_FOLD_MODE = mode
    ops.ff2_fold.cache_clear()


def test_rule_keeps_the_census(auto_rule):
    fixture = gemm_census.load()
    keys = set(gemm_census.keys_of(gemm_census.all_records(fixture)))
    after, folds = replay(fixture)
    for (wl, M, c), k in sorted(folds.items()):
        print(f"[ff2 fold] {wl}: ({M}, {c}) -> {k}")
    new, gone = sorted(after - keys), sorted(keys - after)
    assert not new and not gone, f"the fold changes the launch variants the models reach: new {new}, gone {gone}"
    for (M, c), k in BENCH_FOLDS.items():
        assert folds.get(("sd15_512x512_cfg8", M, c)) == k, (M, c, folds.get(("sd15_512x512_cfg8", M, c)))
    # the mid block of the benchmark's shape stays on two launches: its tile would change
    assert ("sd15_512x512_cfg8", 512, 1280) not in folds


def test_switch_values(lib):
    """"1" folds wherever the library accepts the launch, "0" never (the values are read once per process: patched here)"""
    from consistentid_amd import ops
    mode = ops._FF2_FOLD_MODE
    try:
        for m, want in (("0", False), ("1", True), ("auto", False)):
            ops._FF2_FOLD_MODE = m
            ops.ff2_fold.cache_clear()
            assert ops.ff2_fold(512, 1280, 64) == want, m
    finally:
        ops._FF2_FOLD_MODE = mode
        ops.ff2_fold.cache_clear()
