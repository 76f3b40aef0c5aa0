"""Perturbed-attention guidance on the GPU: the three step entries against the float64 model of the
row contract fed e = u + g (c - u) + s (c - p), against their siblings at s == 0 and replayed from a hipGraph behind
cid_step_select; the UNet forward with perturbed rows against the oracle UNet with tests/pag_ref.py's processor; 4-step
trajectories of three pipelines against ``oracle.loop.denoise`` through ``pag_ref.PagUNet``; one engine switched on, off and on
again; community LoRAs under the folded weights.  Every comparison also asserts, on the oracle, that PAG moves what is compared
by at least ten times the tolerance applied."""
import functools

import numpy as np
import pytest
import torch

import engine_cases as E
import lora_cases as L
import pag_ref as R
from conftest import TOL_L2, check_close, check_vs_fp16_arm, dev_half, rel_l2
from multistep_ref import RowEmulator
from test_gpu_lcm import BIG, KERNEL_ROWS, NAN, _device_row, _same_bits

pytestmark = pytest.mark.gpu

G = 7.5
SHAPES = pytest.mark.parametrize("B,per", [(1, 8), (3, 320), (1, BIG)], ids=["one-item", "3x320", "past-the-grid-cap"])
BLEND = pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
ROW_SCALES = (3.0, 0.0, 1.5, 0.75, 0.0, 2.0)        # the PAG scale of each launch over KERNEL_ROWS; at 0 the perturbed rows are NaN


def _blend(n, g, dev, inpaint):
    if not inpaint:
        return {}, ()
    rnd = lambda: torch.randn(n, generator=g).half()
    mask, init, noise = (torch.rand(n, generator=g) > 0.5).half(), rnd(), rnd()
    return dict(mask=mask.to(dev), init=init.to(dev), noise=noise.to(dev)), tuple(t.double().numpy() for t in (mask, init, noise))


def _eps(parts, n, g, s):
    eps = torch.randn(parts, n, generator=g).half()
    if s == 0.0:
        eps[-1] = NAN
    return eps


# ----------------------------------------------------------------------------------------------------------- the step entries
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "single-pass"])
@BLEND
@SHAPES
def test_multistep_entries_match_the_row_contract(dev, B, per, inpaint, cfg):
    """cid_cfg_pag_multistep_step_f16 ([u | c | p]) and cid_pag_multistep_step_f16 ([c | p]) over the six rows of
    test_gpu_lcm.KERNEL_ROWS, one PAG scale each: latents against the float64 emulator fed e as both halves at check_close's
    defaults after every launch, the ring at 1e-6, ``saved`` a bit copy.  Two launches have s == 0 and NaN in the perturbed
    rows: the sibling entry, launched on copies of the state with the rows in front alone, leaves the same bits in latents,
    ring and ``saved``.  Ring, ``saved`` and noise rows 0 and 1 start as NaN."""
    from consistentid_amd import ops
    n, parts = B * per, 3 if cfg else 2
    g = torch.Generator().manual_seed(n % 1000 + 2 * inpaint + cfg)
    lat0 = torch.randn(n, generator=g).half()
    z = torch.full((3, n), NAN, dtype=torch.float16)
    z[2] = torch.randn(n, generator=g).half()
    blend_h, blend_e = _blend(n, g, dev, inpaint)
    lat, hist = lat0.to(dev), torch.full((4, n), NAN, device=dev)
    saved, zd, pag = torch.full((n,), NAN, dtype=torch.float16, device=dev), z.to(dev), torch.zeros(1, device=dev)
    emu = RowEmulator(n, z=z.double().numpy())
    for k, (row, s) in enumerate(zip(KERNEL_ROWS, ROW_SCALES)):
        eps = _eps(parts, n, g, s)
        x_in = lat.cpu().double().numpy()
        e = R.combine64(eps, G, s, single=not cfg)
        want = emu.step(row, x_in, e, e, 1.0, *blend_e)
        eps_d, drow = eps.to(dev), _device_row(row, dev)
        pag.fill_(s)
        kw = dict(B=B, per_sample=per, z=zd, **blend_h)
        if s == 0.0:
            twin = [t.clone() for t in (lat, hist, saved)]
            if cfg:
                ops.cfg_multistep_step(eps_d[:2], twin[0], twin[1], twin[2], drow, G, **kw)
            else:
                ops.multistep_step(eps_d[:1], twin[0], twin[1], twin[2], drow, **kw)
        if cfg:
            ops.cfg_pag_multistep_step(eps_d, lat, hist, saved, drow, G, pag, **kw)
        else:
            ops.pag_multistep_step(eps_d, lat, hist, saved, drow, pag, **kw)
        torch.cuda.synchronize()
        if s == 0.0:
            for a, b, what in zip((lat, hist, saved), twin, ("latents", "ring", "saved")):
                assert _same_bits(a, b), f"row {k}, pag == 0: {what} differ from the sibling entry"
        check_close(lat, torch.from_numpy(want), f"PAG multistep cfg={cfg} B={B} per_sample={per} inpaint={inpaint} row {k} s={s}")
        if k == 0:
            assert torch.equal(saved.cpu().double(), torch.from_numpy(x_in)), "saved is not a copy of the incoming sample"
    assert torch.isfinite(hist).all()
    check_close(hist, torch.from_numpy(emu.hist), f"PAG multistep ring n={n}", tol_l2=1e-6, tol_max=1e-6)   # fp32 vs float64
    assert torch.equal(saved.cpu().double(), torch.from_numpy(emu.saved))


DDIM_COEFS = [(0.98, -0.12, 0.7, 0.71), (1.05, 0.3, 0.9, 0.43), (0.9, -0.5, 1.0, 0.0), (1.0, 0.2, 0.6, 0.8)]   # c_x, c_eps, c_init, c_noise
DDIM_SCALES = (2.5, 0.0, 0.5, 0.0)


@BLEND
@SHAPES
def test_ddim_entry_matches_the_update(dev, B, per, inpaint):
    """cid_cfg_pag_ddim_step_f16 over four coefficient sets: x' = c_x x + c_eps e (then the inpaint blend) in float64 at
    check_close's defaults; at s == 0, NaN in the perturbed rows and the bits of cid_cfg_ddim_step_f16 on the first 2B rows"""
    from consistentid_amd import ops
    n = B * per
    g = torch.Generator().manual_seed(n % 1000 + 7 + inpaint)
    lat = torch.randn(n, generator=g).half().to(dev)
    blend_h, blend_e = _blend(n, g, dev, inpaint)
    pag = torch.zeros(1, device=dev)
    for k, (coefs, s) in enumerate(zip(DDIM_COEFS, DDIM_SCALES)):
        eps = _eps(3, n, g, s)
        x = lat.cpu().double().numpy()
        want = coefs[0] * x + coefs[1] * R.combine64(eps, G, s)
        if inpaint:
            m, init, noise = blend_e
            want = (1.0 - m) * (coefs[2] * init + coefs[3] * noise) + m * want
        coef = torch.tensor([*coefs, 1.0], dtype=torch.float32, device=dev)
        eps_d = eps.to(dev)
        pag.fill_(s)
        twin = lat.clone()
        if s == 0.0:
            ops.cfg_ddim_step(eps_d[:2], twin, coef, G, B=B, per_sample=per, **blend_h)
        ops.cfg_pag_ddim_step(eps_d, lat, coef, G, pag, B=B, per_sample=per, **blend_h)
        torch.cuda.synchronize()
        if s == 0.0:
            assert _same_bits(lat, twin), f"set {k}, pag == 0: latents differ from cid_cfg_ddim_step_f16"
        check_close(lat, torch.from_numpy(want), f"PAG DDIM B={B} per_sample={per} inpaint={inpaint} set {k} s={s}")


@pytest.mark.parametrize("entry", ["cfg_ddim", "cfg_multistep", "multistep"])
def test_captured_launch_follows_the_pag_column(dev, entry):
    """One captured launch behind cid_step_select over a 4-row table whose PAG column is 2.0, 0.0, 0.5, 1.25 (the model output
    and the coefficient row are columns too; the row at 0 has NaN perturbed rows): four replays equal four eager launches bit
    for bit, and the float64 model of the four steps"""
    from consistentid_amd import ops
    from consistentid_amd.scheduler import pack_step_rows
    from test_gpu_lcm import _row
    n, B = 3 * 1024, 3
    parts, single = (2 if entry == "multistep" else 3), entry == "multistep"
    scales = (2.0, 0.0, 0.5, 1.25)
    g = torch.Generator().manual_seed(31)
    rows = [KERNEL_ROWS[0], KERNEL_ROWS[1], _row(a=0.5, b=0.5, c_x=0.95, c_m=0.4, c_hist=(0.3, -0.35, 0, 0), c_z=0.6, flags=2, z_row=1),
            _row(a=0.1, b=1.0, c_x=1.0, c_m=-0.5, c_hist=(0.45, -0.2, 0, 0), c_z=-0.3, w=0, z_row=2)]
    eps_all = torch.stack([_eps(parts, n, g, s) for s in scales])
    lat0, z = torch.randn(n, generator=g).half(), torch.randn(3, n, generator=g).half()
    emu, x = RowEmulator(n, z=z.double().numpy()), lat0.double().numpy()
    for k, s in enumerate(scales):
        e = R.combine64(eps_all[k], G, s, single=single)
        x = DDIM_COEFS[k][0] * x + DDIM_COEFS[k][1] * e if entry == "cfg_ddim" else emu.step(rows[k], x, e, e, 1.0)
        x = x.astype(np.float16).astype(np.float64)            # the kernel's one rounding, at the store of the latents
    eps_buf = torch.zeros(parts * n, dtype=torch.float16, device=dev)
    pag_buf = torch.zeros(1, dtype=torch.float32, device=dev)
    if entry == "cfg_ddim":
        row_buf = torch.zeros(5, dtype=torch.float32, device=dev)
        row_col = torch.tensor([[*c, 1.0] for c in DDIM_COEFS], dtype=torch.float32)
    else:
        row_buf = torch.zeros(16, dtype=torch.int32, device=dev)
        row_col = torch.from_numpy(pack_step_rows(np.asarray(rows)))
    tab = ops.StepTable([(row_buf, row_col), (eps_buf, eps_all.reshape(4, -1)), (pag_buf, torch.tensor(scales).view(4, 1))], dev)
    lat, hist = lat0.to(dev), torch.full((4, n), NAN, device=dev)
    saved, zd = torch.full((n,), NAN, dtype=torch.float16, device=dev), z.to(dev)

    def launch():
        tab.select()
        if entry == "cfg_ddim":
            ops.cfg_pag_ddim_step(eps_buf, lat, row_buf, G, pag_buf, B=B, per_sample=n // B)
        elif entry == "cfg_multistep":
            ops.cfg_pag_multistep_step(eps_buf, lat, hist, saved, row_buf.view(torch.float32), G, pag_buf, B=B, per_sample=n // B, z=zd)
        else:
            ops.pag_multistep_step(eps_buf, lat, hist, saved, row_buf.view(torch.float32), pag_buf, B=B, per_sample=n // B, z=zd)

    def start():
        lat.copy_(lat0)
        hist.fill_(NAN)
        saved.fill_(NAN)
        tab.reset(0)
    for _ in range(4):
        launch()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (lat, hist, saved)]
    check_close(lat, torch.from_numpy(x), f"four eager {entry}+pag launches")
    start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    start()
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    for got, want, what in zip((lat, hist, saved), eager, ("latents", "ring", "saved")):
        assert _same_bits(got, want), f"graph replay differs from eager launches: {what}"
    check_close(lat, torch.from_numpy(x), f"four replayed {entry}+pag launches")


# ----------------------------------------------------------------------------------------------------------- the UNet forward
T_FWD, B_FWD = 501, 2
SELECTIONS = E.PAG_SELECTIONS       # per model: selection -> (the ids enable_pag is given, the oracle's module paths)
ODD = {"tiny": (24, 20), "tinyxl": (12, 10)}        # token counts 480 / 120 / 30 and 120 / 30: no multiple of 64 at any level
FORWARD_CASES = [(name, sel, hw) for name in ("tiny", "tinyxl") for sel in ("mid", "first-down", "all") for hw in (None, ODD[name])]


@functools.lru_cache(maxsize=None)
def _forward_inputs(dev_str, name, hw, B=B_FWD):
    """(latents [B], embeds [null | text] (2B rows), added conditions of the 3B rows or None), on the CPU in fp16"""
    from consistentid_amd import synth
    cfg = E.unet_models(dev_str, name)[0]
    h, w = hw or (cfg.sample_size, cfg.sample_size)
    inp = synth.random_inputs(cfg, B, 8 * h, 8 * w, seed_latents=2031, seed_embeds=5)
    added = None
    if name == "tinyxl":
        added = {"text_embeds": torch.cat([inp["pooled_null"], inp["pooled_text"], inp["pooled_text"]]),
                 "time_ids": torch.cat([inp["time_ids"], inp["time_ids"][-B:]])}
    return inp["latents"], torch.cat([inp["null"], inp["text"]]), added


def _oracle_forward(unet, paths, dev_str, name, hw, f, B=B_FWD):
    lat, ehs, added = _forward_inputs(dev_str, name, hw, B)
    with torch.no_grad():
        return R.forward_rows(unet, paths, f(torch.cat([lat] * 3)), T_FWD, f(torch.cat([ehs, ehs[B:]])), 3,
                              None if added is None else {k: f(v) for k, v in added.items()})


@functools.lru_cache(maxsize=None)
def _forward_refs(dev_str, name, sel, hw, loras=(), B=B_FWD):
    """(fp32 oracle output, fp16 arm output) of the 3B-row forward whose last B rows are perturbed in ``sel``; computed once"""
    oracle, arm = E.oracle_models(dev_str, name, 0, loras)
    dev, paths = torch.device(dev_str), SELECTIONS[name][sel][1]
    return (_oracle_forward(oracle, paths, dev_str, name, hw, lambda t: t.float(), B),
            _oracle_forward(arm, paths, dev_str, name, hw, lambda t: dev_half(t, dev), B))


@functools.lru_cache(maxsize=None)
def _hip(dev_str, name):
    return E.new_unet(dev_str, name, keep_base=True)


def _hip_forward(hip, dev, name, hw, B=B_FWD):
    """the engine's way: K/V of [null | text], and a row selector that gives the perturbed rows the conditional rows' context"""
    lat, ehs, added = _forward_inputs(str(dev), name, hw, B)
    hip.set_context(ehs.to(dev))
    kvrow = torch.tensor(list(range(2 * B)) + list(range(B, 2 * B)), dtype=torch.int32, device=dev)
    t = torch.full((1,), float(T_FWD), dtype=torch.float32, device=dev)
    kw = None if added is None else {k: v.to(dev) for k, v in added.items()}
    out = hip.forward_tokens(lat.to(dev), t, kvrow, 3 * B, kw, pag_rows=B)
    torch.cuda.synchronize()
    return out


def _check_forward(out, ref, arm, what, B=B_FWD):
    """all 3B rows, then the perturbed rows alone (an error in them must not hide behind the 2B others), each at
    check_vs_fp16_arm's defaults; and the condition that keeps the comparison able to fail: the reference's perturbed rows are
    at least 10 x the tolerance applied away from its conditional rows"""
    check_vs_fp16_arm(out, ref, arm, what)
    _, e_arm = check_vs_fp16_arm(out[2 * B:], ref[2 * B:], arm[2 * B:], f"{what}, perturbed rows")
    tol = max(TOL_L2, 1.5 * e_arm)
    moved = rel_l2(ref[2 * B:], ref[B:2 * B])
    print(f"[pag] {what}: the oracle's perturbed rows are rel_l2={moved:.3e} from its conditional rows (needs >= {10 * tol:.3e})")
    assert moved >= 10 * tol, f"{what}: perturbed and conditional rows of the reference are {moved:.3e} apart, tolerance {tol:.3e}"


@pytest.mark.parametrize("name,sel,hw", FORWARD_CASES, ids=[f"{n}-{s}-{'odd' if hw else 'square'}" for n, s, hw in FORWARD_CASES])
def test_unet_forward_with_perturbed_rows(dev, name, sel, hw):
    """B = 2 latents as 3B batch rows [uncond | cond | perturbed].  ``mid`` keeps the de-duplication of the first transformer
    (tiny: three copies, the generic path), ``first-down`` switches it off, ``all`` perturbs every self-attention; the odd
    latent size runs every transformer on a zero-padded token axis.  The layer count is the oracle's."""
    hip = _hip(str(dev), name)
    ids, paths = SELECTIONS[name][sel]
    hip.enable_pag(ids)
    assert len(hip.pag_layers) == len(R.attn1_modules(E.oracle_models(str(dev), name)[0], paths))
    assert set(hip.packed.pag) == {f"{b}.attn1.vo.{x}" for b in hip.pag_layers for x in ("w", "wl", "lns", "lnb")}
    ref, arm = _forward_refs(str(dev), name, sel, hw)
    out = _hip_forward(hip, dev, name, hw)
    assert tuple(out.shape) == tuple(ref.shape) and out.shape[0] == 3 * B_FWD
    _check_forward(out, ref, arm, f"{name} forward, PAG on {sel}, latents {hw or 'square'}")


UNFOLDED_CASES = [("tiny", "all", 3, False), ("tiny", "first-down", 3, False), ("tiny", "all", 2, True), ("tinyxl", "all", 2, True)]


@pytest.mark.parametrize("name,sel,B,never_fold", UNFOLDED_CASES,
                         ids=[f"{n}-{s}-B{b}{'-nofold' if nf else ''}" for n, s, b, nf in UNFOLDED_CASES])
def test_unet_forward_on_the_unfolded_branch(dev, monkeypatch, name, sel, B, never_fold):
    """The perturbed rows of a launch of more than 2048 rows -- every selection of the two upper levels at the real sizes --
    do not fold norm1: a LayerNorm launch, then the GEMM on the unfolded ``attn1.vo.w`` with to_out's bias and the residual.
    B = 3 on the tiny SD1.5 model reaches it by itself at level 0 (3 x 1024 rows; the deeper levels stay folded); with the
    fold switched off (the CID_LN_FOLD=0 setting of ops.py) every selected layer of both models takes it.  Same check as the
    folded cases; which weight each selected layer's GEMM read is recorded from the launches."""
    from consistentid_amd import ops
    if never_fold:
        monkeypatch.setattr(ops, "_LN_FOLD_MODE", "0")
    hip = _hip(str(dev), name)
    ids, paths = SELECTIONS[name][sel]
    hip.enable_pag(ids)
    read, gemm = set(), ops.gemm

    def spy(x1, w, out, **kw):
        read.add(w.data_ptr())
        return gemm(x1, w, out, **kw)
    monkeypatch.setattr(ops, "gemm", spy)
    out = _hip_forward(hip, dev, name, None, B)
    monkeypatch.setattr(ops, "gemm", gemm)
    P = hip.packed.pag
    unfolded = [b for b in hip.pag_layers if P[f"{b}.attn1.vo.w"].data_ptr() in read]
    folded = [b for b in hip.pag_layers if P[f"{b}.attn1.vo.wl"].data_ptr() in read]
    assert sorted(unfolded + folded) == sorted(hip.pag_layers) and not set(unfolded) & set(folded)
    if never_fold:
        assert not folded
    else:       # level 0 alone: 3 x 1024 perturbed rows there, 3 x 256 and 3 x 64 below
        assert not ops.ln_fold(B * 1024) and ops.ln_fold(B * 256)
        assert unfolded == [b for b in hip.pag_layers if b.startswith(("down_blocks.0.", "up_blocks.2."))] and unfolded
    ref, arm = _forward_refs(str(dev), name, sel, None, (), B)
    assert tuple(out.shape) == tuple(ref.shape) and out.shape[0] == 3 * B
    _check_forward(out, ref, arm, f"{name} forward, PAG on {sel}, B = {B}, unfolded {len(unfolded)} of {len(hip.pag_layers)} layers", B)


def test_unperturbed_forward_is_untouched_by_a_selection(dev):
    """pag_rows = 0 with layers selected: the bits of a UNet that never heard of PAG, and the same packed set"""
    lat, ehs, _ = _forward_inputs(str(dev), "tiny", None)
    plain, hip = E.new_unet(str(dev), "tiny"), _hip(str(dev), "tiny")
    hip.enable_pag(SELECTIONS["tiny"]["all"][0])
    assert set(plain.W) == set(hip.W) and plain.packed.nbytes() == hip.packed.nbytes()
    outs = [u(torch.cat([lat] * 2).to(dev), T_FWD, encoder_hidden_states=ehs.to(dev)).sample.clone() for u in (plain, hip)]
    assert torch.equal(*outs)


# ----------------------------------------------------------------------------------------------------------- trajectories
# (pag_scale, pag_adaptive_scale) per sampler: s_i = 1.755, 0.505, 0, 0 at DDIM's timesteps 751, 501, 251, 1; 2.99, 1.37, 0, 0 at
# DPM-Solver++'s 999, 749, 500, 250; 2.00, 0.92, 0, 0 at LCM's 999, 759, 519, 279
PAG = {"ddim": (3.0, 0.005), "dpm": (3.0, 0.0065), "lcm": (2.0, 0.0045)}
TRAJ_SEL = "all"
TRAJECTORIES = [(pipe, sch) for pipe in ("txt2img", "sdxl", "inpaint") for sch in ("ddim", "dpm", "lcm")]


def _traj_spec(pipe, sch):
    """four steps, the embed switch after the first one (inside the window); LCM at guidance_scale 1: the single pass"""
    return E.Spec(pipe=pipe, scheduler=sch, steps=4, merge=0, guidance=1.0 if sch == "lcm" else 5.0)


@functools.lru_cache(maxsize=None)
def _pag_oracle(spec, dev_str, arm, sel, pag_scale, adaptive):
    """``spec`` through ``oracle.loop.denoise`` with pag_ref.PagUNet in front of the oracle UNet (fp32 on the CPU, or its fp16
    arm on the GPU) -> (latents, [(s_i, |c - p| / |c|) per step])"""
    from oracle import loop
    dev = torch.device(dev_str)
    unet = E.oracle_models(dev_str, spec.name, spec.adapter, spec.loras)[int(arm)]
    f = (lambda t: dev_half(t, dev)) if arm else (lambda t: t.float())
    inp = E.inputs(spec, dev_str)
    sch = E.reference_scheduler(spec, list(inp["variance_noise"].float()))
    kw = dict(num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge)
    if spec.pipe == "inpaint":
        kw.update(inpaint_mask=f(inp["mask"]), inpaint_init=f(inp["init"]), inpaint_noise=f(inp["noise"]), strength=spec.strength)
    if spec.pipe == "sdxl":
        kw.update(add_text_embeds_null=f(inp["pooled_null"]), add_text_embeds_text=f(inp["pooled_text"]),
                  add_text_embeds_aug=f(inp["pooled_augmented"]), add_time_ids=f(inp["time_ids"]))
    model = R.PagUNet(unet, SELECTIONS[spec.name][sel][1], spec.guidance, pag_scale, adaptive, single=E.single_pass(spec))
    out = loop.denoise(model, sch, f(inp["latents"]) * float(sch.init_noise_sigma), f(inp["null"]), f(inp["augmented"]),
                       f(inp["text"]), **kw)
    return out, tuple(model.seen)


class _With:
    """``pipe(**kw)`` of engine_cases.call_pipeline with further keywords added to the call"""

    def __init__(self, pipe, **extra):
        self.pipe, self.extra = pipe, extra

    def __call__(self, **kw):
        return self.pipe(**kw, **self.extra)


def _pag_pipeline(dev, spec, use_graph, sel=TRAJ_SEL):
    pipe = E.pipeline_class(spec)(E.new_unet(str(dev), spec.name, keep_base=True), scheduler=E.product_scheduler(spec), use_graph=use_graph)
    pipe.enable_pag(SELECTIONS[spec.name][sel][0])
    return pipe


def _pag_rows(spec):
    return (2 if E.single_pass(spec) else 3) * spec.B


@pytest.mark.parametrize("pipe,sch", TRAJECTORIES, ids=[f"{p}-{s}" for p, s in TRAJECTORIES])
def test_pag_trajectory(dev, pipe, sch):
    """4 steps with graphs (step 0 eager, step 1 captured, steps 2 and 3 replayed) against the oracle loop through PagUNet at
    check_vs_fp16_arm's defaults, the tolerance of test_gpu_lcm's trajectories.  The adaptive scale makes s_i positive in the
    first two steps -- one before and one after the embed switch -- and 0 in the last two, where the perturbed rows are
    computed and not read.  On the oracle: the trajectory is at least 10 x the tolerance applied away from the same trajectory
    without PAG, and in the steps that read it the perturbed prediction is at least 10 x TOL_L2 (the floor of a single
    forward's tolerance) away from the conditional one.  Measured on the MI355X: rel_l2 1.7e-3 - 3.0e-3 against the arm's
    3.2e-3 - 5.7e-3 over the nine cases; PAG moves the oracle by 0.16 - 0.42, the perturbed prediction is 0.084 - 0.71 away."""
    _check_trajectory(dev, pipe, sch, TRAJ_SEL)


def _check_trajectory(dev, pipe, sch, sel):
    spec = _traj_spec(pipe, sch)
    scale, adaptive = PAG[sch]
    ref, seen = _pag_oracle(spec, str(dev), False, sel, scale, adaptive)
    arm, _ = _pag_oracle(spec, str(dev), True, sel, scale, adaptive)
    assert len(seen) == 4 and seen[0][0] > 0.0 and seen[1][0] > 0.0 and seen[2][0] == 0.0 == seen[3][0], seen
    p = _pag_pipeline(dev, spec, True, sel)
    out, _ = E.call_pipeline(_With(p, pag_scale=scale, pag_adaptive_scale=adaptive), spec, dev)
    eng = p._engine
    assert eng.step_path == E.expected_step_path(spec) + "+pag" and tuple(eng._static["kvrow"].shape) == (_pag_rows(spec),)
    assert len(eng.captures) == 1 and float(eng._static["pag"]) == 0.0
    if pipe == "sdxl":
        assert eng._static["pooled"].shape[0] == _pag_rows(spec) == eng._static["time_ids"].shape[0]
    what = f"{pipe} {sch} 4-step PAG trajectory on {sel}"
    _, e_arm = check_vs_fp16_arm(out, ref, arm, what)
    tol = max(TOL_L2, 1.5 * e_arm)
    moved, apart = rel_l2(ref, E.oracle_run(spec, str(dev))), min(d for s, d in seen if s > 0.0)
    print(f"[pag] {what}: PAG moves the fp32 oracle by rel_l2={moved:.3e} (needs >= {10 * tol:.3e}), |c - p| / |c| >= {apart:.3e} "
          f"in the steps with s_i > 0 (needs >= {10 * TOL_L2:.1e})")
    assert moved >= 10 * tol, f"{what}: PAG moves the reference by {moved:.3e} only, tolerance {tol:.3e}"
    assert apart >= 10 * TOL_L2, f"{what}: perturbed and conditional predictions of the reference are {apart:.3e} apart"


def test_single_pass_trajectory_through_the_deduplication(dev):
    """LCM at guidance_scale 1 with ``mid`` alone selected: the batch [cond | perturbed] goes through the two-copy
    de-duplication of the first transformer (both copies agree until the first cross-attention), which the trajectories on
    ``all`` switch off.  Same checks as there; on the oracle PAG on ``mid`` moves this trajectory by 8.9e-2."""
    _check_trajectory(dev, "txt2img", "lcm", "mid")


def test_trajectory_on_the_unfolded_branch(dev, monkeypatch):
    """the DDIM trajectory on ``all`` with the LayerNorm fold switched off: every perturbed launch of every step, eager, captured
    and replayed, is LayerNorm + GEMM on ``attn1.vo.w`` with bias and residual; same reference, same tolerance"""
    from consistentid_amd import ops
    monkeypatch.setattr(ops, "_LN_FOLD_MODE", "0")
    _check_trajectory(dev, "txt2img", "ddim", "all")


# ----------------------------------------------------------------------------------------------------------- engine reuse
def test_one_engine_on_off_on(dev):
    """One graph pipeline: PAG, no PAG, PAG again, then pag_scale = 0.0 spelled out -- each generation the bits of a fresh eager
    pipeline on a fresh UNet, the step launch and the UNet's batch rows following the switch, and the explicit 0.0 the bits,
    the launch and the rows of the call without the keyword"""
    spec = _traj_spec("txt2img", "ddim")
    scale, adaptive = PAG["ddim"]
    kw = dict(pag_scale=scale, pag_adaptive_scale=adaptive)
    fresh_on = E.call_pipeline(_With(_pag_pipeline(dev, spec, False), **kw), spec, dev)[0].clone()
    fresh_off = E.fresh_eager(spec, str(dev))[0]
    assert rel_l2(fresh_on, fresh_off) >= 10 * TOL_L2
    pipe, eng = _pag_pipeline(dev, spec, True), None
    for gen, (extra, want, path, rows) in enumerate([(kw, fresh_on, "cfg_ddim+pag", 3), ({}, fresh_off, "cfg_ddim", 2),
                                                     (kw, fresh_on, "cfg_ddim+pag", 3), (dict(pag_scale=0.0), fresh_off, "cfg_ddim", 2)]):
        out, _ = E.call_pipeline(_With(pipe, **extra), spec, dev)
        eng = pipe._engine
        assert eng.step_path == path and tuple(eng._static["kvrow"].shape) == (rows * spec.B,), f"generation {gen}"
        assert torch.equal(out, want), f"generation {gen} ({extra or 'no keyword'}): differs from the fresh eager run"
    assert len(eng.captures) == 4, eng.captures       # every switch re-captures: the key holds PAG on / off and the batch rows


def test_default_layers_and_base_weights(dev):
    """pag_scale > 0 without enable_pag selects ``mid``; a UNet built without keep_base refuses, naming it"""
    spec = _traj_spec("txt2img", "ddim")
    pipe = E.pipeline_class(spec)(E.new_unet(str(dev), keep_base=True), use_graph=False)
    assert pipe.unet.pag_layers == ()
    out, _ = E.call_pipeline(_With(pipe, pag_scale=3.0), spec, dev)
    assert pipe.unet.pag_layers == ("mid_block.attentions.0.transformer_blocks.0",) and torch.isfinite(out.float()).all()
    assert pipe._engine.step_path == "cfg_ddim+pag"
    bare = E.pipeline_class(spec)(E.new_unet(str(dev)), use_graph=False)
    with pytest.raises(RuntimeError, match="keep_base=True"):
        E.call_pipeline(_With(bare, pag_scale=3.0), spec, dev)


# ----------------------------------------------------------------------------------------------------------- LoRA
LORA = ((11, 1.0),)


def _bits(t):
    return t.contiguous().view(torch.int16).clone()


@pytest.mark.parametrize("name", ["tiny", "tinyxl"])
def test_lora_reaches_the_folded_weights(dev, name):
    """load_lora_weights repacks ``attn1.vo.*`` in place from base + adapter + LoRA: the 3B-row forward matches the oracle built
    from the merged state dict (and the LoRA moves the oracle's perturbed rows, lora_cases.assert_matters);
    unload_lora_weights restores every folded tensor bit for bit, at its address"""
    spec = E.Spec(pipe="sdxl" if name == "tinyxl" else "txt2img")
    pipe = E.pipeline_class(spec)(E.new_unet(str(dev), name, keep_base=True), use_graph=False)
    ids, _ = SELECTIONS[name]["all"]
    pipe.enable_pag(ids)
    held = {k: (v, v.data_ptr(), _bits(v)) for k, v in pipe.unet.packed.pag.items()}
    pipe.load_lora_weights(E.lora_file(name, LORA[0][0]), adapter_name="a")
    folded = [k for k, (v, _, old) in held.items() if k.endswith(".wl") and not torch.equal(_bits(v), old)]
    assert len(folded) == len(pipe.unet.pag_layers), "a LoRA on to_v / to_out left a folded weight untouched"
    ref, arm = _forward_refs(str(dev), name, "all", None, LORA)
    base = _forward_refs(str(dev), name, "all", None)[0]
    L.assert_matters(ref[2 * B_FWD:], base[2 * B_FWD:], f"{name}: the LoRA in the perturbed rows")
    out = _hip_forward(pipe.unet, dev, name, None)
    _check_forward(out, ref, arm, f"{name} forward with a LoRA, PAG on all")
    pipe.unload_lora_weights()
    for k, (v, ptr, old) in held.items():
        now = pipe.unet.packed.pag[k]
        assert now is v and now.data_ptr() == ptr and torch.equal(_bits(now), old), f"{k} after unload_lora_weights"
    out = _hip_forward(pipe.unet, dev, name, None)
    _check_forward(out, *_forward_refs(str(dev), name, "all", None), f"{name} forward after unload_lora_weights, PAG on all")
