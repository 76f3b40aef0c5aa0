"""Self-attention guidance on the GPU: cid_attn_colmass_f16 and cid_sag_degrade_f16 against the
float64 models of their contracts (tests/sag_ref.py), the three step entries against the float64 model of the row contract and
against their siblings at s == 0, and 3-step trajectories of the pipelines against ``oracle.loop.denoise`` through
``sag_ref.SagUNet``.

The threshold is the trap of the trajectories: a mass near 1.0 flips a mask cell between the fp32 oracle and any fp16 arm, and
one flipped cell moves the whole trajectory.  So every parity case first asserts, on the reference alone, that (a) SAG moves the
oracle by at least 20 x TOL_L2, (b) at every evaluation between 1/8 and 7/8 of the mask cells are set, (c) min |mass - 1| over
the reference trajectory is at least four times the largest deviation of the stock fp16 arm's masses from the fp32 oracle's.
The models are built from a state dict whose ``mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight`` is scaled by
``PEAK`` (1 as measured: see there); the shapes and seeds of ``CASES`` were chosen on the CPU so that (a) - (c) hold with room."""
import functools

import numpy as np
import pytest
import torch

import engine_cases as E
import sag_ref as R
from conftest import TOL_L2, check_close, check_vs_fp16_arm, dev_half, half_arm, rel_l2
from multistep_ref import RowEmulator
from oracle_utils import build_oracle, make_weights, product_cfg
from test_gpu_lcm import BIG, KERNEL_ROWS, NAN, _device_row, _same_bits

pytestmark = pytest.mark.gpu

G = 7.5


# ----------------------------------------------------------------------------------------------------------- the mass kernel
def _tiny_mid(name):
    """(heads, d) of the mid block's self-attention of a tiny model, from the product's config"""
    cfg = product_cfg(name)
    c, heads = cfg.block_out_channels[-1], cfg.num_attention_heads[-1]
    return heads, c // heads


# (B, heads, N, n_keys, d, standard deviation of the base-2 logits[, layout]): the geometry list of DESIGN.md 4.29; 250: a softmax
# without the row maximum subtracted overflows fp32 (2^128) there.  ``layout`` "split": q and k in two buffers of differing
# pitch (see the test).  The generator seed of every case is N + heads + d; the reference conditions were checked on the CPU for
# each of them at the deviation 3.0, which none of the geometries below needed raised.
MASS_CASES = {
    "sd15-512": (1, 8, 64, 64, 160, 3.0),
    "sd15-512x768-padded": (3, 8, 128, 96, 160, 3.0),
    "sd15-1024": (1, 8, 256, 256, 160, 3.0),
    "sdxl-1024": (1, 20, 1024, 1024, 64, 3.0),
    "tiny-6x4-of-64": (2, _tiny_mid("tiny")[0], 64, 24, _tiny_mid("tiny")[1], 3.0),
    "tinyxl-8x8": (2, _tiny_mid("tinyxl")[0], 64, 64, _tiny_mid("tinyxl")[1], 3.0),
    "large-logits": (1, 8, 64, 64, 160, 60.0),
    # the head widths the entry advertises and no model of the suite has; 40 is no multiple of 16: the upper half of the third
    # MFMA K-step is zero-filled by cm_load_frags
    "d32": (2, 2, 64, 64, 32, 3.0),
    "d40": (2, 2, 64, 64, 40, 3.0),
    "d80": (2, 2, 64, 64, 80, 3.0),
    "d40-partial-tile": (2, 2, 64, 40, 40, 3.0),             # ... together with 8 real columns / rows in the last tile
    # SD1.5 at 576 x 576: a 9 x 9 mid block; tiles 0 - 1 full, tile 2 with 17 real columns, tile 3 skipped
    "81-of-128": (2, 8, 128, 81, 160, 3.0),
    "33-of-64": (2, 2, 64, 33, 64, 3.0),                     # one real column and one real row in the last tile
    "257-of-288-nine-tiles": (2, 2, 288, 257, 32, 3.0),      # nine tiles on eight waves: wave 0 takes two, the ninth holds one token
    "4096-top-of-lds": (1, 1, 4096, 4000, 32, 3.0),          # N = CM_MAXN: the last slots of rmax / rinv / macc
    "split-buffers": (2, 2, 64, 64, 64, 3.0, "split"),       # ldq = 3c, ldk = 2c + 8
    "split-buffers-partial": (2, 2, 128, 81, 40, 3.0, "split"),
    "one-head": (2, 1, 64, 64, 64, 3.0),                     # 1 / heads = 1
    "three-heads": (2, 3, 96, 81, 64, 3.0),                  # 1 / 3 is not exact; an odd trip count of the head loop's barrier pairs
}


def mass_inputs(case):
    """(fp16 [q | k] of ``MASS_CASES[case]`` as one [B * N, 2c] tensor, c, the float64 reference, its fp32 arm); needs no GPU"""
    B, heads, N, n_keys, d, sd = MASS_CASES[case][:6]
    c = heads * d
    g = torch.Generator().manual_seed(N + heads + d)
    qk = torch.randn(B * N, 2 * c, generator=g)
    qk[:, :c] *= sd / d ** 0.5
    qk = qk.half()
    if n_keys < N:
        pad = (torch.arange(B * N) % N) >= n_keys
        qk[pad] = (torch.randn(int(pad.sum()), 2 * c, generator=g) * 50.0).half()
    ref = R.colmass64(qk[:, :c], qk[:, c:], B, N, n_keys, heads, d)
    arm = R.colmass64(qk[:, :c], qk[:, c:], B, N, n_keys, heads, d, dtype=torch.float32)
    return qk, c, ref, arm


@pytest.mark.parametrize("case", list(MASS_CASES))
def test_colmass_matches_float64(dev, case):
    """q and k inside ONE [B * N, 2c] buffer at ldq = ldk = 2c, as the fused QKV GEMM leaves them (the ``split`` cases: in two
    buffers, ldq != ldk).  Reference: the same formula
    in float64; the fp16 arm of the tolerance is the formula on the same fp16 q / k evaluated in fp32 torch
    (check_vs_fp16_arm's defaults: max(TOL_L2, 1.5 x the arm's error)).  On the reference: the masses span both sides of 1.
    Pad rows of q and k hold large finite values and must not enter; pad columns are exactly 0; a second launch gives the
    same bits."""
    from consistentid_amd import ops
    B, heads, N, n_keys, d, sd, *layout = MASS_CASES[case]
    qk, c, ref, arm = mass_inputs(case)
    real = ref[:, :n_keys]
    print(f"[sag] {case}: reference masses {float(real.min()):.3f} .. {float(real.max()):.3f}, "
          f"{float((real > 1).double().mean()):.2f} above 1; largest base-2 logit {float((qk[:, :c].double().abs().max())):.1f} x |k|")
    assert real.min() < 0.9 and real.max() > 1.1, "the masses do not span both sides of 1"
    assert abs(float(real.sum(1).mean()) - n_keys) < 1e-6 * n_keys          # every real row of the map sums to 1
    if case == "large-logits":
        s = (qk[:N, :d].double() @ qk[:N, c:c + d].double().T)
        assert s.max() > 128.0, "2^logit would not overflow fp32"
    if layout:
        # q at columns [c, 2c) of a [B * N, 3c] buffer, k at columns [c, 2c) of a [B * N, 2c + 8] buffer; whatever else the two
        # buffers hold is large, finite and must not enter.  A kernel that strode sample 1 by the other operand's pitch, or by
        # none, would give masses of the wrong rows: the two samples' masses differ by far more than the tolerance
        assert layout == ["split"] and B == 2
        dev_arm = float((arm.double() - ref).abs().max())
        apart = float((ref[0] - ref[1]).abs().max())
        print(f"[sag] {case}: the two samples' masses are {apart:.3e} apart (needs >= 10 x the fp32 arm's {dev_arm:.3e})")
        assert apart >= 10 * dev_arm
        g = torch.Generator().manual_seed(N + heads + d + 1)
        q_buf = (torch.randn(B * N, 3 * c, generator=g) * 50.0).half()
        k_buf = (torch.randn(B * N, 2 * c + 8, generator=g) * 50.0).half()
        q_buf[:, c:2 * c], k_buf[:, c:2 * c] = qk[:, :c], qk[:, c:]
        q_buf, k_buf = q_buf.to(dev), k_buf.to(dev)
        q_d, k_d, ldq, ldk = q_buf[:, c:], k_buf[:, c:], 3 * c, 2 * c + 8
    else:
        qk_d = qk.to(dev)
        q_d, k_d, ldq, ldk = qk_d, qk_d[:, c:], 2 * c, 2 * c
    got = torch.full((B, N), NAN, dtype=torch.float32, device=dev)
    ops.attn_colmass(q_d, k_d, got, B=B, N=N, heads=heads, d=d, ldq=ldq, ldk=ldk, n_keys=n_keys)
    again = torch.full((B, N), NAN, dtype=torch.float32, device=dev)
    ops.attn_colmass(q_d, k_d, again, B=B, N=N, heads=heads, d=d, ldq=ldq, ldk=ldk, n_keys=n_keys)
    torch.cuda.synchronize()
    assert _same_bits(got, again), "two launches on the same input differ"
    assert torch.equal(got[:, n_keys:].cpu(), torch.zeros(B, N - n_keys)), "pad columns are not 0"
    check_vs_fp16_arm(got, ref, arm, f"column mass {case}")
    near = (real - 1.0).abs() > 1e-4
    assert torch.equal((got[:, :n_keys].cpu() > 1.0)[near], (real > 1.0)[near]), "a mask cell away from the threshold differs"


# ----------------------------------------------------------------------------------------------------------- the degrade kernel
def _coef_sets():
    from consistentid_amd import scheduler as S
    sets = {}
    for name, cls, pt in (("vp-eps", S.DDIMScheduler, "epsilon"), ("vp-v", S.DDIMScheduler, "v_prediction"),
                          ("euler-eps", S.EulerDiscreteScheduler, "epsilon")):
        sch = cls(prediction_type=pt)
        sch.set_timesteps(4)
        sets[name] = S.sag_coefficient_table(sch)[1]
    return sets


DEGRADE_SHAPES = {"8x8": (2, 4, 8, 8, 2, 2), "64x64": (1, 4, 64, 64, 8, 8), "96x64": (2, 4, 96, 64, 12, 8), "5x7-odd": (1, 3, 5, 7, 2, 3)}
MASKS = ("random", "all-clear", "all-set", "checkerboard-at-1")


@pytest.mark.parametrize("coefs", ["vp-eps", "vp-v", "euler-eps"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", list(DEGRADE_SHAPES))
def test_degrade_matches_float64(dev, shape, mask, coefs):
    """cid_sag_degrade_f16 against sag_ref.degrade64 (F.pad(mode="reflect") + grouped conv2d in float64) at check_close's
    defaults.  8 x 8: the reflection reaches across half the image; 96 x 64 with a 12 x 8 mask: more than one tile each way,
    ragged against the 16-pixel tile.  ``all-clear`` equals n_d x0 + n_e ehat; ``checkerboard-at-1`` alternates exactly 1.0
    (strict >: clear) with the next fp32 above it (set)."""
    from consistentid_amd import ops
    B, C, h, w, hm, wm = DEGRADE_SHAPES[shape]
    g = torch.Generator().manual_seed(h * w + MASKS.index(mask))
    x, e = torch.randn(B, C, h, w, generator=g).half(), torch.randn(B, C, h, w, generator=g).half()
    if mask == "random":
        mass = 1.0 + 0.5 * torch.randn(B, hm * wm, generator=g)
    elif mask == "checkerboard-at-1":
        board = (torch.arange(hm)[:, None] + torch.arange(wm)[None]) % 2 == 1
        mass = torch.where(board, torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)), torch.tensor(1.0)).reshape(1, -1).repeat(B, 1)
    else:
        mass = torch.full((B, hm * wm), 2.0 if mask == "all-set" else 0.5)
    mass = mass.float().contiguous()
    coef = torch.from_numpy(_coef_sets()[coefs]).float()
    want = R.degrade64(x, e, mass, coef, hm, wm)
    if mask == "all-clear":
        p_x, p_e, q_x, q_e, n_d, n_e = [float(v) for v in coef[:6]]
        plain = n_d * (p_x * x.double() + p_e * e.double()) + n_e * (q_x * x.double() + q_e * e.double())
        assert torch.allclose(want, plain, rtol=0, atol=1e-12)
    if mask == "checkerboard-at-1":
        set_ = R.upsample_mask(mass.reshape(B, hm, wm) > 1.0, h, w)
        assert 0 < int(set_.sum()) < set_.numel()
    out = torch.full((B, C, h, w), NAN, dtype=torch.float16, device=dev)
    ops.sag_degrade(x.to(dev), e.to(dev), mass.to(dev), out, coef.to(dev), hm=hm, wm=wm)
    torch.cuda.synchronize()
    check_close(out, want, f"degrade {shape} {mask} {coefs}")


def test_degrade_refusals(dev, lib):
    """-22 before any launch: h < 5 or w < 5, a null pointer, a misaligned buffer"""
    t = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    p, q = t.data_ptr(), f.data_ptr()
    ok = lambda *a: lib.cid_sag_degrade_f16(*a, None)
    assert ok(p, p, q, p, q, 1, 4, 8, 8, 2, 2) == 0
    assert ok(p, p, q, p, q, 1, 4, 4, 8, 2, 2) == -22 and ok(p, p, q, p, q, 1, 4, 8, 4, 2, 2) == -22
    for k in range(5):
        args = [p, p, q, p, q]
        args[k] = None
        assert ok(*args, 1, 4, 8, 8, 2, 2) == -22, f"null pointer {k}"
        args[k] = (p, p, q, p, q)[k] + 2 * (1 + (k in (2, 4)))
        assert ok(*args, 1, 4, 8, 8, 2, 2) == -22, f"misaligned pointer {k}"
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- the step entries
SHAPES = pytest.mark.parametrize("B,per", [(1, 8), (3, 320), (1, BIG)], ids=["one-item", "3x320", "past-the-grid-cap"])
BLEND = pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
ROW_SCALES = (0.75, 0.0, 1.5, 1.0, 0.0, 2.0)        # the SAG scale of each launch over KERNEL_ROWS; at 0 eps_d is NaN


def _blend(n, g, dev, inpaint):
    if not inpaint:
        return {}, ()
    rnd = lambda: torch.randn(n, generator=g).half()
    mask, init, noise = (torch.rand(n, generator=g) > 0.5).half(), rnd(), rnd()
    return dict(mask=mask.to(dev), init=init.to(dev), noise=noise.to(dev)), tuple(t.double().numpy() for t in (mask, init, noise))


def _eps_d(n, g, s):
    return torch.full((n,), NAN, dtype=torch.float16) if s == 0.0 else torch.randn(n, generator=g).half()


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "single-pass"])
@BLEND
@SHAPES
def test_multistep_entries_match_the_row_contract(dev, B, per, inpaint, cfg):
    """cid_cfg_sag_multistep_step_f16 (eps [u | c]) and cid_sag_multistep_step_f16 (eps [c]) over the six rows of
    test_gpu_lcm.KERNEL_ROWS, one SAG scale each: latents against the float64 emulator fed e as both halves at check_close's
    defaults after every launch, the ring at 1e-6, ``saved`` a bit copy.  Two launches have s == 0 and NaN in eps_d: the
    sibling entry on copies of the state leaves the same bits in latents, ring and ``saved``."""
    from consistentid_amd import ops
    n, parts = B * per, 2 if cfg else 1
    g = torch.Generator().manual_seed(n % 1000 + 2 * inpaint + cfg + 50)
    lat0 = torch.randn(n, generator=g).half()
    z = torch.full((3, n), NAN, dtype=torch.float16)
    z[2] = torch.randn(n, generator=g).half()
    blend_h, blend_e = _blend(n, g, dev, inpaint)
    lat, hist = lat0.to(dev), torch.full((4, n), NAN, device=dev)
    saved, zd = torch.full((n,), NAN, dtype=torch.float16, device=dev), z.to(dev)
    emu = RowEmulator(n, z=z.double().numpy())
    for k, (row, s) in enumerate(zip(KERNEL_ROWS, ROW_SCALES)):
        eps, ed = torch.randn(parts, n, generator=g).half(), _eps_d(n, g, s)
        x_in = lat.cpu().double().numpy()
        e = R.combine64(eps, ed, G, s, single=not cfg)
        want = emu.step(row, x_in, e, e, 1.0, *blend_e)
        eps_dev, ed_dev, drow = eps.to(dev), ed.to(dev), _device_row(row, dev)
        kw = dict(B=B, per_sample=per, z=zd, **blend_h)
        if s == 0.0:
            twin = [t.clone() for t in (lat, hist, saved)]
            if cfg:
                ops.cfg_multistep_step(eps_dev, twin[0], twin[1], twin[2], drow, G, **kw)
            else:
                ops.multistep_step(eps_dev, twin[0], twin[1], twin[2], drow, **kw)
        if cfg:
            ops.cfg_sag_multistep_step(eps_dev, lat, hist, saved, drow, G, ed_dev, s, **kw)
        else:
            ops.sag_multistep_step(eps_dev, lat, hist, saved, drow, ed_dev, s, **kw)
        torch.cuda.synchronize()
        if s == 0.0:
            for a, b, what in zip((lat, hist, saved), twin, ("latents", "ring", "saved")):
                assert _same_bits(a, b), f"row {k}, s == 0: {what} differ from the sibling entry"
        check_close(lat, torch.from_numpy(want), f"SAG multistep cfg={cfg} B={B} per_sample={per} inpaint={inpaint} row {k} s={s}")
        if k == 0:
            assert torch.equal(saved.cpu().double(), torch.from_numpy(x_in)), "saved is not a copy of the incoming sample"
    assert torch.isfinite(hist).all()
    check_close(hist, torch.from_numpy(emu.hist), f"SAG multistep ring n={n}", tol_l2=1e-6, tol_max=1e-6)   # fp32 vs float64
    assert torch.equal(saved.cpu().double(), torch.from_numpy(emu.saved))


DDIM_COEFS = [(0.98, -0.12, 0.7, 0.71), (1.05, 0.3, 0.9, 0.43), (0.9, -0.5, 1.0, 0.0), (1.0, 0.2, 0.6, 0.8)]   # c_x, c_eps, c_init, c_noise
DDIM_SCALES = (0.75, 0.0, 1.5, 0.0)


@BLEND
@SHAPES
def test_ddim_entry_matches_the_update(dev, B, per, inpaint):
    """cid_cfg_sag_ddim_step_f16 over four coefficient sets: x' = c_x x + c_eps e (then the inpaint blend) in float64 at
    check_close's defaults; at s == 0, NaN in eps_d and the bits of cid_cfg_ddim_step_f16"""
    from consistentid_amd import ops
    n = B * per
    g = torch.Generator().manual_seed(n % 1000 + 57 + inpaint)
    lat = torch.randn(n, generator=g).half().to(dev)
    blend_h, blend_e = _blend(n, g, dev, inpaint)
    for k, (coefs, s) in enumerate(zip(DDIM_COEFS, DDIM_SCALES)):
        eps, ed = torch.randn(2, n, generator=g).half(), _eps_d(n, g, s)
        x = lat.cpu().double().numpy()
        want = coefs[0] * x + coefs[1] * R.combine64(eps, ed, G, s)
        if inpaint:
            m, init, noise = blend_e
            want = (1.0 - m) * (coefs[2] * init + coefs[3] * noise) + m * want
        coef = torch.tensor([*coefs, 1.0], dtype=torch.float32, device=dev)
        eps_dev = eps.to(dev)
        twin = lat.clone()
        if s == 0.0:
            ops.cfg_ddim_step(eps_dev, twin, coef, G, B=B, per_sample=per, **blend_h)
        ops.cfg_sag_ddim_step(eps_dev, lat, coef, G, ed.to(dev), s, B=B, per_sample=per, **blend_h)
        torch.cuda.synchronize()
        if s == 0.0:
            assert _same_bits(lat, twin), f"set {k}, s == 0: latents differ from cid_cfg_ddim_step_f16"
        check_close(lat, torch.from_numpy(want), f"SAG DDIM B={B} per_sample={per} inpaint={inpaint} set {k} s={s}")


# ----------------------------------------------------------------------------------------------------------- trajectories
Q_KEY = f"{R.LAYER}.to_q.weight"
# Factor on that layer's to_q.weight.  Measured on the CPU: the synthetic tiny weights do NOT give near-uniform attention -- at
# factor 1 the masses of one evaluation run from 0.13 to 4.8 with 45 % above 1 -- and a larger factor only raises the fp16 arm's
# mass deviation (1.4e-2 at factor 1, 2.7e-2 at 4, 4.3e-2 at 12) while the cells nearest to 1 stay where they are.  So the factor
# is 1 and condition (c) is met by the shapes and seeds: one sample on small latents (4 to 16 mid-block tokens of
# the 64 the token axis is padded to, i.e. 12 - 48 mask cells per trajectory) and an input seed per case.
PEAK = {"tiny": 1.0, "tinyxl": 1.0}
SAG = 1.0                                  # sag_scale of the parity cases
# three schedule steps each (PNDM: four evaluations), the embed switch after the first.  ``seed``: of every input value, chosen
# with tools/sag_seed_search.py (fp16 arm on the CPU as a stand-in, whose deviation is 2 - 4 times smaller than the GPU arm's)
# so that min |mass - 1| is well above ten times the arm's largest mass deviation there; the test asserts the factor 4 against
# the GPU arm.
SMALL = dict(steps=3, merge=0, B=1, hw=(16, 16))
CASES = {
    "ddim": E.Spec(scheduler="ddim", seed=625, **{**SMALL, "hw": (12, 12)}),     # mid block 3 x 3
    "euler": E.Spec(scheduler="euler", seed=247, **SMALL),
    "dpm": E.Spec(scheduler="dpm", seed=222, **{**SMALL, "hw": (16, 8)}),
    "pndm": E.Spec(scheduler="pndm", seed=557, **{**SMALL, "hw": (8, 8)}),
    "lcm-single-pass": E.Spec(scheduler="lcm", guidance=1.0, seed=306, **{**SMALL, "hw": (16, 8)}),
    "sdxl-null-post": E.Spec(pipe="sdxl", scheduler="ddim", null_post=True, seed=324, **{**SMALL, "hw": (6, 6)}),     # mid block 3 x 3
    "inpaint-blend": E.Spec(pipe="inpaint", scheduler="ddim", seed=342, **SMALL),
    "v-prediction": E.Spec(scheduler="ddim", prediction="v_prediction", seed=974, **{**SMALL, "hw": (8, 8)}),     # the arm deviates 2.5 x more here: 2 x 2 mid tokens
    "non-square": E.Spec(scheduler="ddim", seed=331, **{**SMALL, "hw": (16, 8)}),      # mid block 4 x 2 = 8 tokens, padded to 64
}


@functools.lru_cache(maxsize=None)
def sag_models(dev_str, name, nine=False):
    """(cfg, state dict, adapter dict, fp32 oracle, fp16 arm or None without a GPU) with the peaky ``to_q`` of ``PEAK``"""
    over = {"in_channels": 9} if nine else {}
    cfg, sd, ad = make_weights(name, rank=8, **over)
    sd = dict(sd)
    sd[Q_KEY] = (sd[Q_KEY].float() * PEAK[name]).to(sd[Q_KEY].dtype)
    oracle = build_oracle(name, sd, ad, rank=8, **over)
    dev = torch.device(dev_str)
    return cfg, sd, ad, oracle, (half_arm(oracle, dev) if dev.type == "cuda" else None)


def _loop_kw(spec, inp, f):
    kw = dict(num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge)
    if spec.pipe == "inpaint":
        kw.update(inpaint_mask=f(inp["mask"]), inpaint_init=f(inp["init"]), inpaint_noise=f(inp["noise"]), strength=spec.strength)
    if spec.pipe == "sdxl":
        kw.update(add_text_embeds_null=f(inp["pooled_null"]), add_text_embeds_text=f(inp["pooled_text"]),
                  add_text_embeds_aug=f(inp["pooled_augmented"]), add_time_ids=f(inp["time_ids"]))
        if spec.null_post:
            kw["null_embeds_post"] = f(inp["null_post"])
    return kw


def arm_unet(dev_str, name, nine=False):
    """(the stock fp16 arm of the peaky oracle on the GPU, the cast of its inputs); tools/sag_seed_search.py puts a CPU
    stand-in here to choose seeds without a GPU"""
    dev = torch.device(dev_str)
    return sag_models(dev_str, name, nine)[4], (lambda t: dev_half(t, dev))


@functools.lru_cache(maxsize=None)
def sag_oracle(case, dev_str, arm, s):
    """``CASES[case]`` (or ``TWO_SAMPLES[case]``) through ``oracle.loop.denoise`` with sag_ref.SagUNet in front of the peaky oracle UNet (fp32 on the
    CPU, or its fp16 arm on the GPU) -> (latents, masses per evaluation, masks per evaluation); s == 0: the plain loop"""
    from lcm_ref import CondOnly
    from oracle import loop
    spec = {**CASES, **TWO_SAMPLES}[case]
    unet, f = arm_unet(dev_str, spec.name) if arm else (sag_models(dev_str, spec.name)[3], (lambda t: t.float()))
    inp = E.inputs(spec, dev_str)
    sch = E.reference_scheduler(spec, list(inp["variance_noise"].float()))
    single = E.single_pass(spec)
    if s > 0.0:
        model = R.SagUNet(unet, sch, spec.guidance, s, single=single, prediction=spec.prediction)
    else:
        model = CondOnly(unet) if single else unet
    out = loop.denoise(model, sch, f(inp["latents"]) * float(sch.init_noise_sigma), f(inp["null"]), f(inp["augmented"]),
                       f(inp["text"]), **_loop_kw(spec, inp, f))
    return out, tuple(getattr(model, "masses", ())), tuple(getattr(model, "masks", ()))


def reference_says_something(case, dev_str):
    """(a), (b), (c) of the module docstring on the reference alone -> (fp32 latents, arm latents, fp32 masses, arm masses)"""
    ref, masses, masks = sag_oracle(case, dev_str, False, SAG)
    arm, arm_masses, _ = sag_oracle(case, dev_str, True, SAG)
    base, _, _ = sag_oracle(case, dev_str, False, 0.0)
    moved = rel_l2(ref, base)
    fractions = [float(m.mean()) for m in masks]
    margin = min(float(np.abs(m - 1.0).min()) for m in masses)
    dev_arm = max(float(np.abs(a - m).max()) for a, m in zip(arm_masses, masses))
    print(f"[sag] {case}: (a) SAG moves the fp32 oracle by rel_l2={moved:.3e} (needs >= {20 * TOL_L2:.1e}); (b) mask cells set per "
          f"evaluation {[round(x, 3) for x in fractions]} (needs 1/8 .. 7/8); (c) min |mass - 1| = {margin:.3e}, largest mass "
          f"deviation of the fp16 arm {dev_arm:.3e} (needs a factor 4, has {margin / max(dev_arm, 1e-30):.1f})")
    assert len(masses) == E.executed_steps(CASES[case])
    assert moved >= 20 * TOL_L2, f"{case}: SAG moves the reference by {moved:.3e} only"
    assert all(1 / 8 <= x <= 7 / 8 for x in fractions), f"{case}: mask fractions {fractions}"
    assert margin >= 4.0 * dev_arm, f"{case}: min |mass - 1| = {margin:.3e} < 4 x {dev_arm:.3e}"
    return ref, arm, masses, arm_masses


class _With:
    """``pipe(**kw)`` of engine_cases.call_pipeline with further keywords added to the call"""

    def __init__(self, pipe, **extra):
        self.pipe, self.extra = pipe, extra

    def __call__(self, **kw):
        return self.pipe(**kw, **self.extra)


def _pipeline(dev, spec, use_graph):
    from consistentid_amd.unet import HipUNet
    cfg, sd, ad, _, _ = sag_models(str(dev), spec.name)
    return E.pipeline_class(spec)(HipUNet(cfg, sd, ad, device=dev), scheduler=E.product_scheduler(spec), use_graph=use_graph)


def _check_masses(eng, masses, arm_masses, what):
    """engine_cases.check_last_masses with the arm's largest deviation over the trajectory"""
    E.check_last_masses(eng, masses, max(float(np.abs(a - m).max()) for a, m in zip(arm_masses, masses)), what)


@pytest.mark.parametrize("case", list(CASES))
def test_sag_trajectory(dev, case):
    """graphs on (evaluation 0 eager, 1 captured, the rest replayed) against the oracle loop through SagUNet at
    check_vs_fp16_arm's defaults; the step launch is the sibling's ``+sag``, one capture; the engine's mass buffer of the last
    evaluation against the reference's"""
    spec = CASES[case]
    ref, arm, masses, arm_masses = reference_says_something(case, str(dev))
    pipe = _pipeline(dev, spec, True)
    out, _ = E.call_pipeline(_With(pipe, sag_scale=SAG), spec, dev)
    eng = pipe._engine
    assert eng.step_path == E.expected_step_path(spec) + "+sag"
    assert tuple(eng._static["kvrow"].shape) == ((1 if E.single_pass(spec) else 2) * spec.B,)
    assert len(eng.captures) == 1
    check_vs_fp16_arm(out, ref, arm, f"{case} SAG trajectory")
    _check_masses(eng, masses, arm_masses, case)


# B = 2, ONE evaluation, masses only: the guide rows' slices of the engine (the mass rows, the kept prediction, the context
# rows, SDXL's conditions) and the per-sample stride of the mass buffer, which the B = 1 trajectories cannot tell from [:1].  With
# 32 cells per evaluation condition (c) is out of reach, so no trajectory is compared: the masses of the first evaluation are.
TWO_SAMPLES = {
    "two-samples": E.Spec(scheduler="ddim", steps=1, merge=0, B=2, hw=(16, 16)),
    "two-samples-sdxl": E.Spec(pipe="sdxl", scheduler="ddim", steps=1, merge=0, B=2, hw=(8, 8), time_ids=(8, 16)),
    "two-samples-single-pass": E.Spec(scheduler="lcm", steps=1, merge=0, guidance=1.0, B=2, hw=(16, 16)),
}


@pytest.mark.parametrize("case", list(TWO_SAMPLES))
def test_two_samples_masses(dev, case):
    """the engine's masses of a one-step run with two samples against the reference's: every mass within 1.5 x the fp16 arm's
    largest deviation (``_check_masses``' bound), every mask cell further than 4 x that deviation from the threshold equal; on
    the reference, the two samples' masses are at least 10 x that deviation apart, so a wrong row or stride cannot pass"""
    spec = TWO_SAMPLES[case]
    _, masses, _ = sag_oracle(case, str(dev), False, SAG)
    _, arm_masses, _ = sag_oracle(case, str(dev), True, SAG)
    assert len(masses) == 1 and masses[0].shape[0] == 2
    want = torch.from_numpy(masses[0])
    dev_arm = float(np.abs(arm_masses[0] - masses[0]).max())
    apart = float((want[0] - want[1]).abs().max())
    pipe = _pipeline(dev, spec, False)
    E.call_pipeline(_With(pipe, sag_scale=SAG), spec, dev)
    got = pipe.sag_mass.cpu().double()
    off = float((got - want).abs().max())
    print(f"[parity] {case}: largest mass deviation {off:.3e} | fp16 arm {dev_arm:.3e} -> tol {1.5 * dev_arm:.3e}; the samples' "
          f"masses are {apart:.3e} apart (needs >= {10 * dev_arm:.3e})")
    assert apart >= 10 * dev_arm
    assert tuple(got.shape) == tuple(want.shape) and torch.isfinite(got).all() and off <= 1.5 * dev_arm
    clear = (want - 1.0).abs() > 4.0 * dev_arm
    assert torch.equal((got > 1.0)[clear], (want > 1.0)[clear]) and int(clear.sum()) >= want.numel() // 2


NINE_SEED = 8       # of the latents and embeds of the 9-channel case, chosen like the seeds of CASES


def nine_channel_runs(dev_str):
    """the 9-channel inpainting UNet through the oracle loop: {"ref", "base", "arm"} -> (latents, masses, masks), and the inputs"""
    from consistentid_amd import synth
    from oracle import ddim, loop
    seed = NINE_SEED
    oracle = sag_models(dev_str, "tiny", True)[3]
    arm_m, fa = arm_unet(dev_str, "tiny", True)
    B, steps, g, h = 1, 3, 5.0, 8
    inp = synth.random_inputs(make_weights("tiny")[0], B, 8 * h, 8 * h, seed_latents=3000 + seed, seed_embeds=7 + seed)
    gen = torch.Generator().manual_seed(41 + seed)
    init = torch.randn(B, 4, h, h, generator=gen).half()
    mask = (torch.rand(B, 1, h, h, generator=gen) > 0.5).half()
    masked = (init.float() * (1 - mask.float())).half()
    extra = torch.cat([mask, masked], dim=1)
    runs = {}
    for key, unet, f, s in (("ref", oracle, lambda t: t.float(), SAG), ("base", oracle, lambda t: t.float(), 0.0), ("arm", arm_m, fa, SAG)):
        sch = ddim.DDIMScheduler()
        sch.set_timesteps(steps)
        model = R.SagUNet(unet, sch, g, s) if s > 0.0 else unet
        out = loop.denoise(model, sch, f(inp["latents"]), f(inp["null"]), f(inp["augmented"]), f(inp["text"]),
                           num_inference_steps=steps, guidance_scale=g, start_merge_step=0, unet_extra=f(extra))
        runs[key] = (out, getattr(model, "masses", ()), getattr(model, "masks", ()))
    return runs, inp, mask, masked, (steps, g)


def nine_channel_figures(runs):
    ref, masses, masks = runs["ref"]
    moved = rel_l2(ref, runs["base"][0])
    margin = min(float(np.abs(m - 1.0).min()) for m in masses)
    dev_arm = max(float(np.abs(a - m).max()) for a, m in zip(runs["arm"][1], masses))
    return moved, [float(m.mean()) for m in masks], margin, dev_arm


def test_nine_channel_inpainting_unet(dev):
    """the inpaint pipeline on a 9-channel UNet: cat([mask, masked_image_latents]) reaches the second evaluation too (beside
    the degraded latents, unscaled) and nothing is blended.  Reference conditions (a) - (c) as in the other cases."""
    from consistentid_amd import pipeline, scheduler
    from consistentid_amd.unet import HipUNet
    runs, inp, mask, masked, (steps, g) = nine_channel_runs(str(dev))
    moved, fractions, margin, dev_arm = nine_channel_figures(runs)
    print(f"[sag] 9-channel: (a) {moved:.3e} (b) {fractions} (c) {margin:.3e} against {dev_arm:.3e}")
    assert moved >= 20 * TOL_L2 and all(1 / 8 <= x <= 7 / 8 for x in fractions) and margin >= 4.0 * dev_arm
    (ref, masses, _), (arm, arm_masses, _) = runs["ref"], runs["arm"]
    cfg, sd, ad, _, _ = sag_models(str(dev), "tiny", True)
    pipe = pipeline.StableDiffusionInpaintConsistentIDPipeline(HipUNet(cfg, sd, ad, device=dev), scheduler=scheduler.DDIMScheduler())
    out = pipe(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]).to(dev), latents=inp["latents"].to(dev),
               num_inference_steps=steps, guidance_scale=g, start_merge_step=0, output_type="latent", mask_latents=mask.to(dev),
               masked_image_latents=masked.to(dev), sag_scale=SAG).images
    torch.cuda.synchronize()
    assert pipe._engine.step_path == "cfg_ddim+sag"
    check_vs_fp16_arm(out, ref, arm, "9-channel inpaint SAG trajectory")
    _check_masses(pipe._engine, masses, arm_masses, "9-channel inpaint")


def test_graph_equals_eager_and_a_second_scale(dev):
    """one graph pipeline: sag_scale 1.0, then 0.5 (the scale is part of the graph key: a new capture), then 1.0 again -- each
    generation the bits of a fresh eager pipeline; the second scale against its own reference"""
    spec = CASES["ddim"]
    eager = {s: E.call_pipeline(_With(_pipeline(dev, spec, False), sag_scale=s), spec, dev)[0].clone() for s in (SAG, 0.5)}
    assert rel_l2(eager[0.5], eager[SAG]) >= 10 * TOL_L2
    pipe = _pipeline(dev, spec, True)
    for gen, s in enumerate((SAG, 0.5, SAG)):
        out, _ = E.call_pipeline(_With(pipe, sag_scale=s), spec, dev)
        assert pipe._engine.step_path == "cfg_ddim+sag"
        assert torch.equal(out, eager[s]), f"generation {gen} (sag_scale {s}): differs from the fresh eager run"
    assert len(pipe._engine.captures) == 3, pipe._engine.captures
    ref, arm = sag_oracle("ddim", str(dev), False, 0.5)[0], sag_oracle("ddim", str(dev), True, 0.5)[0]
    check_vs_fp16_arm(eager[0.5], ref, arm, "ddim SAG trajectory at sag_scale 0.5")


@pytest.mark.parametrize("case", ["ddim", "lcm-single-pass"])
def test_scale_zero_is_the_call_without_the_keyword(dev, case):
    """sag_scale = 0.0 spelled out: the bits, the step launch, the static buffers and the capture count of the call without it"""
    spec = CASES[case]
    runs = []
    for extra in ({}, dict(sag_scale=0.0)):
        pipe = _pipeline(dev, spec, True)
        out, _ = E.call_pipeline(_With(pipe, **extra), spec, dev)
        runs.append((out.clone(), pipe._engine.step_path, len(pipe._engine.captures), sorted(pipe._engine._static)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    assert runs[1][1] == E.expected_step_path(spec) and not any(k.startswith("sag") for k in runs[1][3])
