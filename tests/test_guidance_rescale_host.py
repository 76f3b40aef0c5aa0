"""Host side of guidance_rescale, v-prediction and zero-SNR DDIM (no GPU): the schedulers' fp32 coefficient tables, run
through the float64 model of the step kernels' contracts, against the stateful restatements of the diffusers 0.23 ``step``
functions in tests/vpred_ref.py; configs, loader, refusals; the ABI refusals of the three new entry points."""
import json
import math
import zlib

import numpy as np
import pytest
import torch

from conftest import check_close
from multistep_ref import RowEmulator
from vpred_ref import DDIMRef, DPMSolverVRef, EulerRef, PNDMVRef

from consistentid_amd import loader, scheduler as S

A = 64        # a 16-byte-aligned stand-in address
N = 24        # elements of the toy sample
G = 5.0
ZERO_SNR = dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")


class TableEmulator:
    """float64 model of cid_cfg_ddim_step_f16 on a ``coefficient_table`` row: c_x, c_eps, c_init, c_noise (, c_in)"""

    def step(self, row, x, eps_u, eps_c, g, mask=None, init=None, noise=None):
        row = np.asarray(row, dtype=np.float64)
        out = row[0] * x + row[1] * (eps_u + g * (eps_c - eps_u))
        if mask is not None:
            out = (1.0 - mask) * (row[2] * init + row[3] * noise) + mask * out
        return out


# name -> (product class, reference class, takes coefficient_rows)
SAMPLERS = {"ddim": (S.DDIMScheduler, DDIMRef), "euler": (S.EulerDiscreteScheduler, EulerRef),
            "pndm": (S.PNDMScheduler, PNDMVRef), "dpm": (S.DPMSolverMultistepScheduler, DPMSolverVRef)}
# DDIM additionally with eta = 1, the inpaint blend and first_step > 0 (every scheduler gets the blend and the window too)
VARIANTS = [(name, eta, inpaint, first) for name in SAMPLERS for eta in ((0.0, 1.0) if name == "ddim" else (0.0,))
            for inpaint, first in ((False, 0), (True, 0), (False, 3), (True, 2))]


def _run_both(name, prediction_type, eta, inpaint, first, steps=8, **sched_kw):
    """(per-step samples of the emulated tables, per-step samples of the stateful reference) on shared random inputs"""
    product_cls, ref_cls = SAMPLERS[name]
    rng = np.random.default_rng(zlib.crc32(repr((name, prediction_type, eta, inpaint, first)).encode()))
    product = product_cls(prediction_type=prediction_type, **sched_kw)
    product.set_timesteps(steps)
    n_ts = len(product.timesteps)
    x0 = rng.standard_normal(N) * float(product.init_noise_sigma)
    outs = rng.standard_normal((n_ts, 2, N))
    z = rng.standard_normal((n_ts - first, N))
    mask, init, noise = (rng.random(N) > 0.5).astype(np.float64), rng.standard_normal(N), rng.standard_normal(N)
    blend = (mask, init, noise) if inpaint else ()

    rows_path = bool(product.multistep) or eta > 0.0
    if rows_path:
        table = product.coefficient_rows(inpaint, first, np.float32, **({"eta": eta} if eta > 0.0 else {}))
        emu = RowEmulator(N, z=z if eta > 0.0 else None)
    else:
        table = product.coefficient_table(inpaint)
        emu = TableEmulator()
    assert table.dtype == np.float32 and np.isfinite(table).all()
    x, got = x0.copy(), []
    for i in range(first, n_ts):
        x = emu.step(table[i], x, outs[i, 0], outs[i, 1], G, *blend)
        got.append(x)

    kw = dict(sched_kw)
    if name == "ddim":
        kw.update(eta=eta, noises=[torch.from_numpy(r) for r in z])
    ref = ref_cls(prediction_type=prediction_type, **kw)
    ref.set_timesteps(steps)
    ts = ref.timesteps[first:]
    assert [float(t) for t in ref.timesteps] == [float(t) for t in product.timesteps]
    xr, want = torch.from_numpy(x0.copy()), []
    for k, t in enumerate(ts):
        e = torch.from_numpy(outs[first + k, 0] + G * (outs[first + k, 1] - outs[first + k, 0]))
        xr = ref.step(e, t, xr)
        if inpaint:
            ini = torch.from_numpy(init)
            if k < len(ts) - 1:
                ini = ref.add_noise(ini, torch.from_numpy(noise), ts[k + 1])
            xr = (1 - torch.from_numpy(mask)) * ini + torch.from_numpy(mask) * xr
        want.append(xr.numpy())
    return got, want


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("name,eta,inpaint,first", VARIANTS,
                         ids=[f"{n}-eta{int(e)}-{'inpaint' if i else 'plain'}-first{f}" for n, e, i, f in VARIANTS])
def test_tables_match_the_stateful_step_functions(name, eta, inpaint, first, prediction_type):
    """every step's sample, fp32 tables in the float64 kernel model against the float64 step functions: 1e-6 relative, the
    fp32-table-against-fp64 tolerance of test_gpu_multistep.py's ring check"""
    got, want = _run_both(name, prediction_type, eta, inpaint, first)
    assert len(got) == len(want) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        check_close(torch.from_numpy(g), torch.from_numpy(w), f"{name} {prediction_type} eta={eta} inpaint={inpaint} "
                    f"first={first} step {k}", tol_l2=1e-6, tol_max=1e-6)


@pytest.mark.parametrize("eta,inpaint", [(0.0, False), (1.0, False), (0.0, True)])
def test_zero_snr_ddim_trajectory(eta, inpaint):
    """v-prediction + zero-SNR betas + trailing spacing, 4 steps from the terminal timestep, against the step function"""
    got, want = _run_both("ddim", "v_prediction", eta, inpaint, 0, steps=4, rescale_betas_zero_snr=True,
                          timestep_spacing="trailing")
    for k, (g, w) in enumerate(zip(got, want)):
        check_close(torch.from_numpy(g), torch.from_numpy(w), f"zero-SNR DDIM eta={eta} inpaint={inpaint} step {k}",
                    tol_l2=1e-6, tol_max=1e-6)


def test_zero_snr_schedule_starts_at_the_terminal_timestep():
    sch = S.DDIMScheduler(**ZERO_SNR)
    sch.set_timesteps(4)
    assert int(sch.timesteps[0]) == 999 and sch.alphas_cumprod[999] == 0.0
    # the first entry is kept up to the float32 roundings of the shift and the scale
    assert (sch.alphas_cumprod[:999] > 0).all() and sch.alphas_cumprod[0] == pytest.approx(S.DDIMScheduler().alphas_cumprod[0], rel=1e-6)
    for tab in (sch.coefficient_table(False), sch.coefficient_table(True), sch.coefficient_rows(eta=1.0),
                sch.coefficient_rows(inpaint=True, eta=0.5)):
        assert np.isfinite(tab).all()
    # the terminal step: x0 = -v, eps = x -- the sample only contributes as the noise it is
    c_x, c_v = sch.step_coefficients(999)
    a_p = float(sch.alphas_cumprod[999 - 250])
    assert c_x == pytest.approx(math.sqrt(1 - a_p), rel=1e-12) and c_v == pytest.approx(-math.sqrt(a_p), rel=1e-12)


def test_epsilon_prediction_on_a_zero_snr_schedule_is_refused():
    sch = S.DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    sch.set_timesteps(4)
    with pytest.raises(ValueError, match="alphas_cumprod is 0"):
        sch.coefficient_table(False)
    with pytest.raises(ValueError, match="alphas_cumprod is 0"):
        sch.coefficient_rows(eta=1.0)
    # ... but not where the schedule never reaches the terminal timestep
    lead = S.DDIMScheduler(rescale_betas_zero_snr=True)
    lead.set_timesteps(4)
    assert np.isfinite(lead.coefficient_table(False)).all()


ALL = (S.DDIMScheduler, S.EulerDiscreteScheduler, S.PNDMScheduler, S.DPMSolverMultistepScheduler)


@pytest.mark.parametrize("cls", ALL)
def test_config_round_trips_and_refusals(cls):
    """``.config`` reports the prediction type and ``Other.from_config(scheduler.config)`` -- the reference scripts' idiom --
    carries it to any of the four classes; so does the keyword override ``from_config(config, prediction_type=...)``.  A RAW
    dict that names v-prediction or zero-SNR betas stays refused without the keyword (tests/test_host_logic.py,
    tests/test_multistep_host.py and tests/test_loader.py pin that answer)."""
    assert cls().config["prediction_type"] == "epsilon" and cls().prediction_type == "epsilon"
    v = cls(prediction_type="v_prediction", timestep_spacing="trailing")
    assert v.config["prediction_type"] == "v_prediction"
    for other in ALL:
        again = other.from_config(v.config)
        assert (again.prediction_type, again.timestep_spacing) == ("v_prediction", "trailing")
        assert again.config["prediction_type"] == "v_prediction"
        assert other.from_config(again.config).prediction_type == "v_prediction"           # and on, through a second class
        assert other.from_config(cls().config, prediction_type="v_prediction").prediction_type == "v_prediction"
        assert other.from_config(v.config, prediction_type="epsilon").prediction_type == "epsilon"
        assert other.from_config(dict(v.config), prediction_type="v_prediction").prediction_type == "v_prediction"
        with pytest.raises(NotImplementedError, match="prediction_type=..."):
            other.from_config(dict(v.config))
    for bad in (lambda: cls(prediction_type="sample"), lambda: cls.from_config(dict(cls().config, prediction_type="sample")),
                lambda: cls.from_config(cls().config, prediction_type="sample")):
        with pytest.raises(NotImplementedError, match="prediction_type"):
            bad()
    with pytest.raises(TypeError):
        cls.from_config(cls().config, use_karras_sigmas=True)
    z = S.DDIMScheduler(**ZERO_SNR)
    if cls is S.DDIMScheduler:
        for again in (cls.from_config(z.config), cls.from_config(cls().config, **ZERO_SNR),
                      cls.from_config(dict(z.config), prediction_type="v_prediction", rescale_betas_zero_snr=True)):
            assert again.config["rescale_betas_zero_snr"] is True and again.prediction_type == "v_prediction"
            assert again.alphas_cumprod.tobytes() == z.alphas_cumprod.tobytes() and again.timestep_spacing == "trailing"
        assert cls().config["rescale_betas_zero_snr"] is False and cls.from_config(cls().config).alphas_cumprod[-1] > 0.0
        with pytest.raises(NotImplementedError, match="zero-SNR"):
            cls.from_config(dict(z.config), prediction_type="v_prediction")
    else:
        # the other three have no such flag in diffusers 0.23: a zero-SNR DDIM's config does not move to them
        for cfg in (z.config, dict(cls().config, rescale_betas_zero_snr=True)):
            with pytest.raises(NotImplementedError, match="DDIMScheduler only"):
                cls.from_config(cfg)
        for make in (lambda: cls(rescale_betas_zero_snr=True), lambda: cls.from_config(cls().config, rescale_betas_zero_snr=True)):
            with pytest.raises(TypeError):
                make()


def _parent_ddim_pair(sch, t):
    """the epsilon coefficients as the code computed them before prediction_type existed"""
    a_t, a_p = sch.alphas(t)
    return (a_p / a_t) ** 0.5, (1.0 - a_p) ** 0.5 - (a_p ** 0.5) * ((1.0 - a_t) ** 0.5) / (a_t ** 0.5)


# The two multistep classes' ``coefficient_rows`` as they stood before prediction_type existed, restated with ``self`` = the scheduler
def _parent_pndm_rows(self, inpaint: bool = False, first_step: int = 0, dtype=np.float32) -> np.ndarray:
    ts, T = self.timesteps, self.num_train_timesteps
    ratio = T // self.num_inference_steps
    rows = [S._idle_row() for _ in range(min(first_step, len(ts)))]
    counter = appended = 0
    for i in range(first_step, len(ts)):
        t = int(ts[i])
        w, flags, c_hist = -1, 0, [0.0] * 4
        if counter != 1:
            w = appended % 4
            appended += 1
            prev = t - ratio
        else:
            prev, t = t, t + ratio
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)
        c_x = (a_p / a_t) ** 0.5
        c_mo = -(a_p - a_t) / (a_t * (1.0 - a_p) ** 0.5 + (a_t * (1.0 - a_t) * a_p) ** 0.5)
        held = min(appended, 4)
        slot = lambda back: (appended - back) % 4          # ring slot of ets[-back]
        if counter == 1:                                    # (e + ets[-1]) / 2 from the remembered sample
            c_m, flags = 0.5 * c_mo, S.FLAG_RESTORE
            c_hist[slot(1)] = 0.5 * c_mo
        else:                                               # ets[-1] is this step's e, written after the reads
            weights = {1: (1.0,), 2: (1.5, -0.5), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[held]
            c_m = weights[0] * c_mo
            for back, wt in enumerate(weights[1:], start=2):
                c_hist[slot(back)] = wt * c_mo
            if counter == 0:
                flags = S.FLAG_SAVE
        ci, cn = S._next_blend(self, inpaint, i)
        rows.append(S._row(a=0.0, b=1.0, c_x=c_x, c_m=c_m, c_hist=c_hist, c_init=ci, c_noise=cn, w=w, flags=flags))
        counter += 1
    return np.asarray(rows, dtype=np.float64).reshape(-1, S.ROW_WORDS).astype(dtype)


def _parent_dpm_rows(self, inpaint: bool = False, first_step: int = 0, dtype=np.float32) -> np.ndarray:
    n = len(self.timesteps)
    alpha = 1.0 / (self.sigmas ** 2 + 1.0) ** 0.5
    s = self.sigmas * alpha
    lam = np.log(alpha) - np.log(s)
    rows = [S._idle_row() for _ in range(min(first_step, n))]
    for i in range(first_step, n):
        k = i - first_step
        h = lam[i + 1] - lam[i]
        D = -alpha[i + 1] * (np.exp(-h) - 1.0)
        c_m, c_hist = D, [0.0] * 4
        if k > 0 and not (i == n - 1 and n < 15):
            r = (lam[i] - lam[i - 1]) / h
            c_m = D + D / (2.0 * r)
            c_hist[(k - 1) % 4] = -D / (2.0 * r)
        ci, cn = S._next_blend(self, inpaint, i)
        rows.append(S._row(a=1.0 / alpha[i], b=-s[i] / alpha[i], c_x=s[i + 1] / s[i], c_m=float(c_m), c_hist=c_hist,
                         c_init=ci, c_noise=cn, w=k % 4))
    return np.asarray(rows, dtype=np.float64).reshape(-1, S.ROW_WORDS).astype(dtype)


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_epsilon_tables_are_bit_identical(name):
    """``prediction_type`` omitted and "epsilon" give the same bits, and those are the bits of the formulas this file
    restates from the code as it stood before prediction_type existed (all four classes), and of a from_config round trip
    of a config that never had the key"""
    cls = SAMPLERS[name][0]
    legacy_cfg = {k: v for k, v in cls().config.items() if k not in ("prediction_type", "rescale_betas_zero_snr")}
    for steps in (4, 50):
        tabs = []
        for sch in (cls(), cls(prediction_type="epsilon"), cls.from_config(legacy_cfg)):
            sch.set_timesteps(steps)
            for inpaint in (False, True):
                if hasattr(sch, "coefficient_table"):
                    tabs.append(sch.coefficient_table(inpaint))
                if hasattr(sch, "coefficient_rows"):
                    tabs.append(sch.coefficient_rows(inpaint, 1))
                    if name == "ddim":
                        tabs.append(sch.coefficient_rows(inpaint, 0, eta=0.5))
        k = len(tabs) // 3
        for a, b, c in zip(tabs[:k], tabs[k:2 * k], tabs[2 * k:]):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        sch = cls()
        sch.set_timesteps(steps)
        if name == "ddim":
            want = np.asarray([[*_parent_ddim_pair(sch, int(t)), 1.0, 0.0, 1.0] for t in sch.timesteps], dtype=np.float32)
            assert sch.coefficient_table(False).tobytes() == want.tobytes()
        if name in ("pndm", "dpm"):
            parent_rows = _parent_pndm_rows if name == "pndm" else _parent_dpm_rows
            for inpaint, first in ((False, 0), (True, 0), (True, 2)):
                assert sch.coefficient_rows(inpaint, first).tobytes() == parent_rows(sch, inpaint, first).tobytes()
        if name == "euler":
            sg = [float(s) for s in sch.sigmas]
            want = np.asarray([[1.0, sg[i + 1] - sg[i], 1.0, 0.0, 1.0 / (sg[i] * sg[i] + 1.0) ** 0.5] for i in range(steps)],
                              dtype=np.float32)
            assert sch.coefficient_table(False).tobytes() == want.tobytes()


def test_loader_reads_a_v_prediction_model(tmp_path):
    """loader acceptance on a temporary scheduler_config.json: ``prediction_type: v_prediction`` of every class name reaches
    the engine scheduler, and the hand-over ``Other.from_config(pipe.scheduler.config)`` keeps it.  A saved
    ``rescale_betas_zero_snr`` is still the loader's error that names ``scheduler=`` (tests/test_loader.py pins it): the
    route there is ``from_pretrained(..., scheduler=DDIMScheduler(...))`` or the keywords on the saved JSON."""
    import warnings
    d = tmp_path / "m" / "scheduler"
    d.mkdir(parents=True)
    base = {"beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear", "num_train_timesteps": 1000,
            "steps_offset": 1, "clip_sample": False, "prediction_type": "v_prediction"}

    def read(**cfg):
        (d / "scheduler_config.json").write_text(json.dumps(dict(base, **cfg)))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            return loader.read_scheduler(tmp_path / "m"), [str(x.message) for x in w]

    sch, w = read(_class_name="DDIMScheduler", timestep_spacing="trailing")
    assert isinstance(sch, S.DDIMScheduler) and sch.prediction_type == "v_prediction" and sch.timestep_spacing == "trailing"
    assert len(w) == 1 and "v-prediction model" in w[0]
    sch, _ = read(_class_name="EulerDiscreteScheduler", timestep_spacing="leading")
    assert isinstance(sch, S.EulerDiscreteScheduler) and sch.prediction_type == "v_prediction"
    # a modifier the engine drops does not take the prediction type with it
    sch, w = read(_class_name="DDIMScheduler", clip_sample=True)
    assert sch.prediction_type == "v_prediction" and any("IGNORES" in m for m in w)
    # classes the loader samples with DDIM on their config until pipe.scheduler is replaced
    for name, cls in (("PNDMScheduler", S.PNDMScheduler), ("DPMSolverMultistepScheduler", S.DPMSolverMultistepScheduler)):
        sch, _ = read(_class_name=name, skip_prk_steps=True)
        assert isinstance(sch, S.DDIMScheduler) and sch.prediction_type == "v_prediction"
        assert cls.from_config(sch.config).prediction_type == "v_prediction"
    sch, _ = read(_class_name="DDIMScheduler", prediction_type="epsilon")
    assert sch.prediction_type == "epsilon"
    for flag in (dict(use_karras_sigmas=True), dict(interpolation_type="log_linear"), dict(rescale_betas_zero_snr=True)):
        with pytest.raises(NotImplementedError, match="noise schedule"):
            read(_class_name="DDIMScheduler", **flag)
    # the zero-SNR route on the saved JSON
    with open(d / "scheduler_config.json") as f:
        cfg = json.load(f)
    z = S.DDIMScheduler.from_config(cfg, prediction_type=cfg["prediction_type"], rescale_betas_zero_snr=True,
                                    timestep_spacing="trailing")
    assert z.prediction_type == "v_prediction" and z.alphas_cumprod[-1] == 0.0


def test_guidance_rescale_argument_is_checked():
    from consistentid_amd import denoise, pipeline
    import inspect
    assert denoise.check_guidance_rescale(0) == 0.0 and denoise.check_guidance_rescale(0.7) == 0.7
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            denoise.check_guidance_rescale(bad)
    for cls in (pipeline.ConsistentIDStableDiffusionPipeline, pipeline.ConsistentIDStableDiffusionXLPipeline,
                pipeline.StableDiffusionInpaintConsistentIDPipeline, pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline):
        p = inspect.signature(cls.__call__).parameters["guidance_rescale"]
        assert p.default == 0.0
        with pytest.raises(ValueError, match="guidance_rescale"):      # refused before anything else is looked at
            cls.__new__(cls)(guidance_rescale=-1.0)
    assert inspect.signature(denoise.DenoiseEngine.run).parameters["guidance_rescale"].default == 0.0
    for cls in (pipeline.ConsistentIDStableDiffusionPipeline, pipeline.StableDiffusionInpaintConsistentIDPipeline,
                pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline):
        assert list(inspect.signature(cls.__call__).parameters)[-1] == "guidance_rescale"      # trailing: positional calls keep


def _refused(lib, rc, fragment):
    msg = lib.cid_last_error()
    assert rc == -22 and fragment in msg, (rc, msg)


def test_new_entry_points_check_their_arguments_without_gpu(lib):
    """-22 with a message before anything is launched; dummy non-null addresses (tests/test_abi.py)"""
    assert lib.cid_version() >= 108

    def factor(eps=A, g=7.5, phi=0.7, escale=A, B=2, per=64):
        return lib.cid_cfg_rescale_f16(eps, g, phi, escale, B, per, None)

    for kw in (dict(eps=None), dict(escale=None)):
        _refused(lib, factor(**kw), b"cid_cfg_rescale_f16: null pointer")
    for B in (0, -1):
        _refused(lib, factor(B=B), b"cid_cfg_rescale_f16: B must be positive")
    for per in (0, -8, 4, 12, 65):
        _refused(lib, factor(per=per), b"cid_cfg_rescale_f16: per_sample must be a positive multiple of 8")
    for per in (2 ** 24 + 8, 2 ** 31 - 8):
        _refused(lib, factor(per=per), b"cid_cfg_rescale_f16: per_sample must be at most 2^24")
    for eps in (A + 2, A + 8):
        _refused(lib, factor(eps=eps), b"cid_cfg_rescale_f16: eps must be 16-byte aligned")
    for phi in (-0.5, float("nan"), float("inf"), -float("inf")):
        _refused(lib, factor(phi=phi), b"cid_cfg_rescale_f16: rescale must be finite and not negative")

    def ddim(eps=A, lat=A, coef=A, mask=None, init=None, noise=None, B=2, per=64, escale=A):
        return lib.cid_cfg_ddim_step_scaled_f16(eps, lat, coef, 7.5, mask, init, noise, B, per, escale, None)

    for kw in (dict(eps=None), dict(lat=None), dict(coef=None), dict(escale=None)):
        _refused(lib, ddim(**kw), b"cid_cfg_ddim_step_scaled_f16: null pointer")
    for kw in (dict(mask=A), dict(mask=A, init=A), dict(init=A, noise=A)):
        _refused(lib, ddim(**kw), b"cid_cfg_ddim_step_scaled_f16: mask/init/noise must come together")
    # B * per_sample = 8 passes the unscaled entry; here an item may not straddle two samples
    for kw in (dict(B=0), dict(per=0), dict(B=2, per=4), dict(B=8, per=9)):
        _refused(lib, ddim(**kw), b"cid_cfg_ddim_step_scaled_f16: per_sample must be a multiple of 8")
    _refused(lib, ddim(B=2 ** 10, per=2 ** 24), b"cid_cfg_ddim_step_scaled_f16: B * per_sample must be below 2^34")

    def multi(eps=A, lat=A, hist=A, saved=A, z=None, z_rows=0, row=A, mask=None, init=None, noise=None, B=2, per=64, escale=A):
        return lib.cid_cfg_multistep_step_scaled_f16(eps, lat, hist, saved, z, z_rows, row, 7.5, mask, init, noise, B, per,
                                                     escale, None)

    for kw in (dict(eps=None), dict(lat=None), dict(hist=None), dict(saved=None), dict(row=None), dict(escale=None)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_scaled_f16: null pointer")
    for kw in (dict(z=A), dict(z_rows=2), dict(z=A, z_rows=-1)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_scaled_f16: z and z_rows must come together")
    for kw in (dict(mask=A), dict(mask=A, init=A), dict(init=A, noise=A)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_scaled_f16: mask/init/noise must come together")
    for kw in (dict(B=0), dict(per=0), dict(B=2, per=4), dict(B=8, per=9)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_scaled_f16: per_sample must be a multiple of 8")
    _refused(lib, multi(B=2 ** 10, per=2 ** 24), b"cid_cfg_multistep_step_scaled_f16: B * per_sample must be below 2^34")
