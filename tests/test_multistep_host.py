"""Host side of the multistep step (PNDM, DPM-Solver++ 2M, DDIM with eta): the product's per-step rows, fed through a float64
model of the kernel's row contract, against the stateful restatements of tests/multistep_ref.py; properties that need no
restatement; the config surface; the argument checks of the C entry point.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from multistep_ref import DDIMEtaRef, DPMSolverPP2MRef, PNDMRef, RowEmulator

from consistentid_amd import scheduler as S

SPACINGS = ("leading", "linspace", "trailing")
SAMPLERS = ("pndm", "dpm", "ddim_eta")
N_ELEM, G, ETA = 24, 3.0, 0.7

SD15_PNDM_JSON = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012,
                  "beta_schedule": "scaled_linear", "beta_start": 0.00085, "num_train_timesteps": 1000,
                  "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None,
                  "clip_sample": False}
SDXL_EULER_JSON = {"_class_name": "EulerDiscreteScheduler", "_diffusers_version": "0.19.0.dev0", "beta_end": 0.012,
                   "beta_schedule": "scaled_linear", "beta_start": 0.00085, "clip_sample": False,
                   "interpolation_type": "linear", "num_train_timesteps": 1000, "prediction_type": "epsilon",
                   "sample_max_value": 1.0, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1,
                   "timestep_spacing": "leading", "trained_betas": None, "use_karras_sigmas": False}
CLASSES = (S.DDIMScheduler, S.EulerDiscreteScheduler, S.PNDMScheduler, S.DPMSolverMultistepScheduler)


def toy_eps(x, t):
    """a fixed non-linear model with an unconditional and a conditional head (any array library with tanh / cos)"""
    t = float(t)
    lib = torch if isinstance(x, torch.Tensor) else np
    u = lib.tanh(0.7 * x + 0.3 * np.sin(t / 100.0)) + 0.1 * x * np.cos(t / 37.0)
    c = 0.5 * lib.cos(x - t / 200.0) + 0.2 * x
    return u, c


def _pair(sampler, spacing, noises=None):
    """(product scheduler, stateful restatement, extra arguments of coefficient_rows)"""
    if sampler == "pndm":
        return S.PNDMScheduler(timestep_spacing=spacing), PNDMRef(timestep_spacing=spacing), {}
    if sampler == "dpm":
        return (S.DPMSolverMultistepScheduler(timestep_spacing=spacing, steps_offset=1),
                DPMSolverPP2MRef(timestep_spacing=spacing, steps_offset=1), {})
    return S.DDIMScheduler(timestep_spacing=spacing), DDIMEtaRef(ETA, noises, timestep_spacing=spacing), {"eta": ETA}


def _run_rows(sch, rows, first, x0, z=None, blend=None, eps=toy_eps):
    emu = RowEmulator(x0.size, z=z)
    x = x0.copy()
    for i in range(first, len(sch.timesteps)):
        u, c = eps(x, sch.timesteps[i])
        x = emu.step(rows[i], x, u, c, G, *(blend or ()))
    return x


def _run_stateful(ref, n, first, x0, blend=None):
    ref.set_timesteps(n)
    ts = ref.timesteps[first:]
    x = torch.from_numpy(x0.copy())
    for i, t in enumerate(ts):
        u, c = toy_eps(x, t)
        x = ref.step(u + G * (c - u), t, x)
        if blend is not None:
            mask, init, noise = (torch.from_numpy(b) for b in blend)
            ini = ref.add_noise(init, noise, ts[i + 1]) if i < len(ts) - 1 else init
            x = (1 - mask) * ini + mask * x
    return x.numpy()


CASES = [(s, sp, n, f, inp) for s, sp, n, f, inp in itertools.product(SAMPLERS, SPACINGS, (1, 2, 3, 4, 5, 12, 20), (0, 3),
                                                                      (False, True)) if f < n]


@pytest.mark.parametrize("sampler,spacing,n,first,inpaint", CASES)
def test_rows_reproduce_the_stateful_sampler(sampler, spacing, n, first, inpaint):
    """The two forms are algebraically equal (a float64 prototype of both recurrences agrees to 1e-14): relative L2 <= 1e-9.
    The fp32 rows the device gets are the float64 rows rounded once."""
    rng = np.random.default_rng(1000 * n + first)
    x0 = rng.standard_normal(N_ELEM)
    noises = rng.standard_normal((n + 1, N_ELEM))
    blend = None
    if inpaint:
        blend = ((rng.random(N_ELEM) > 0.5).astype(np.float64), rng.standard_normal(N_ELEM), rng.standard_normal(N_ELEM))
    sch, ref, kw = _pair(sampler, spacing, [torch.from_numpy(z) for z in noises])
    sch.set_timesteps(n)
    rows = sch.coefficient_rows(inpaint, first, np.float64, **kw)
    assert rows.shape == (len(sch.timesteps), 16) and rows.dtype == np.float64
    got = _run_rows(sch, rows, first, x0, z=noises if sampler == "ddim_eta" else None, blend=blend)
    want = _run_stateful(ref, n, first, x0, blend)
    assert np.array_equal(np.asarray(ref.timesteps), sch.timesteps)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert np.isfinite(got).all() and err <= 1e-9, f"{sampler} {spacing} n={n} first={first} inpaint={inpaint}: rel_l2 {err:.3e}"
    rows32 = sch.coefficient_rows(inpaint, first, np.float32, **kw)
    assert rows32.dtype == np.float32 and np.array_equal(rows32, rows.astype(np.float32))
    packed = S.pack_step_rows(rows32)
    assert packed.dtype == np.int32 and np.array_equal(packed[:, :12].view(np.float32), rows32[:, :12])
    assert np.array_equal(packed[:, 12:], rows[:, 12:].astype(np.int32)) and np.all(rows[:, S.C_IN] == 1.0)


@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("n", [2, 5, 20])
def test_pndm_with_a_constant_model_output_is_ddim(spacing, n):
    """Every PNDM combination of model outputs has weights summing to 1, and its transfer formula is DDIM's (eta 0) written
    differently: with eps constant in time the trajectory ends where the product's DDIM ends.  Both are at most 21 float64
    updates with coefficients of order 1, a few ulp each: bound 1e-12 (measured <= 2e-14).
    Holds where neighbouring timesteps are T // n apart -- "leading" always, "trailing" for n | T.  With "linspace" they
    are not, and the published PNDM redoes its first step from ``t + T // n``, which is then not the timestep the
    remembered sample belongs to: there the two samplers differ by construction (0.76 relative at n = 2), so that
    spacing has no such property to test."""
    rng = np.random.default_rng(n)
    x0, e = rng.standard_normal(N_ELEM), rng.standard_normal(N_ELEM)
    const = lambda x, t: (e, e)
    pndm = S.PNDMScheduler(timestep_spacing=spacing)
    pndm.set_timesteps(n)
    got = _run_rows(pndm, pndm.coefficient_rows(False, 0, np.float64), 0, x0, eps=const)
    ddim = S.DDIMScheduler(timestep_spacing=spacing)
    ddim.set_timesteps(n)
    want = x0.copy()
    for t in ddim.timesteps:
        c_x, c_e = ddim.step_coefficients(int(t))
        want = c_x * want + c_e * e
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err <= 1e-12, f"PNDM vs DDIM, {spacing} n={n}: rel_l2 {err:.3e}"


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", [5, 20])
def test_dpm_solver_is_exact_for_a_point_mass(spacing, n):
    """eps(x, t) = (x - alpha_t x*) / sigma_t is the exact noise prediction when the data are the single point x*: the data
    prediction is x* at every step, the second-order difference vanishes, and DPM-Solver++ lands on alpha_last x* +
    sigma_last e_0 with e_0 the initial noise direction.  Float64, <= 20 updates: bound 1e-12 (measured <= 2e-14)."""
    rng = np.random.default_rng(n)
    star, e0 = rng.standard_normal(N_ELEM), rng.standard_normal(N_ELEM)
    sch = S.DPMSolverMultistepScheduler(timestep_spacing=spacing, steps_offset=1)
    sch.set_timesteps(n)
    alpha = 1.0 / np.sqrt(sch.sigmas.astype(np.float64) ** 2 + 1.0)
    sig = sch.sigmas * alpha
    index = {int(t): i for i, t in enumerate(sch.timesteps)}

    def eps(x, t):
        i = index[int(t)]
        e = (x - alpha[i] * star) / sig[i]
        return e, e
    got = _run_rows(sch, sch.coefficient_rows(False, 0, np.float64), 0, alpha[0] * star + sig[0] * e0, eps=eps)
    want = alpha[-1] * star + sig[-1] * e0
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err <= 1e-12, f"DPM-Solver++ on a point mass, {spacing} n={n}: rel_l2 {err:.3e}"


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_no_row_weighs_what_was_not_written(sampler, spacing):
    """for every schedule length and strength window: a ring slot, ``saved`` or a noise row with a non-zero coefficient was
    written by an earlier row of the same generation (the ring and ``saved`` keep the previous generation's values)"""
    for n in range(1, 26):
        sch, _, kw = _pair(sampler, spacing, [])
        sch.set_timesteps(n)
        for first in range(len(sch.timesteps)):
            rows = sch.coefficient_rows(True, first, np.float64, **kw)
            assert rows.shape == (len(sch.timesteps), 16)
            slots, saved, n_run = set(), False, len(sch.timesteps) - first
            for k, row in enumerate(rows[first:]):
                where = f"{sampler} {spacing} n={n} first={first} step {k}"
                assert np.isfinite(row).all(), where
                w, flags, z_row = int(row[12]), int(row[13]), int(row[14])
                assert all(s in slots for s in range(4) if row[4 + s] != 0.0), f"{where}: unwritten ring slot"
                assert saved or not flags & 2, f"{where}: unwritten saved sample"
                assert -1 <= w < 4 and 0 <= flags < 4 and row[15] == 0.0, where
                if row[S.C_Z] != 0.0:
                    assert sampler == "ddim_eta" and z_row == k < n_run, f"{where}: noise row {z_row}"
                if w >= 0:
                    slots.add(w)
                saved = saved or bool(flags & 1)


@pytest.mark.parametrize("json_cfg", [SD15_PNDM_JSON, SDXL_EULER_JSON], ids=["sd15_pndm", "sdxl_euler"])
def test_from_config_round_trips_between_the_four_classes(json_cfg):
    for first, second in itertools.product(CLASSES, CLASSES):
        a = first.from_config(json_cfg)
        b = second.from_config(a.config)
        for sch in (a, b):
            assert sch.steps_offset == 1 and sch.timestep_spacing == "leading" and sch.num_train_timesteps == 1000
            assert sch.config["beta_start"] == 0.00085 and sch.config["beta_end"] == 0.012
            sch.set_timesteps(7)
            assert len(sch.timesteps) == (8 if isinstance(sch, S.PNDMScheduler) else 7) and sch.order == 1
            assert float(sch.init_noise_sigma) >= 1.0
            if not isinstance(sch, S.EulerDiscreteScheduler):      # Euler's input scale is a table column (conv_in applies it)
                assert sch.scale_model_input(3.0, sch.timesteps[0]) == 3.0
            ca, cn = sch.add_noise_coefficients(sch.timesteps[1])
            assert ca > 0 and cn > 0
    assert S.PNDMScheduler.from_config(SD15_PNDM_JSON).timesteps.dtype == np.int64
    # the SD1.5 schedule of diffusers' PNDM documentation: 50 steps -> 51 evaluations, the second timestep twice
    p = S.PNDMScheduler.from_config(SD15_PNDM_JSON)
    p.set_timesteps(50)
    assert list(p.timesteps[:4]) == [981, 961, 961, 941] and p.timesteps[-1] == 1 and len(p.timesteps) == 51
    d = S.DPMSolverMultistepScheduler()
    d.set_timesteps(20)
    assert d.timestep_spacing == "linspace" and d.timesteps[0] == 999 and len(d.sigmas) == 21 and d.timesteps.dtype == np.int64


@pytest.mark.parametrize("key,value", [("use_karras_sigmas", True), ("thresholding", True), ("solver_order", 3),
                                       ("solver_type", "heun"), ("algorithm_type", "sde-dpmsolver++"),
                                       ("algorithm_type", "dpmsolver"), ("lambda_min_clipped", -5.1),
                                       ("variance_type", "learned_range"), ("lower_order_final", False)])
def test_dpm_solver_refuses_what_is_not_built(key, value):
    with pytest.raises(NotImplementedError, match=key):
        S.DPMSolverMultistepScheduler.from_config({**SD15_PNDM_JSON, key: value})


def test_other_refusals():
    with pytest.raises(NotImplementedError, match="skip_prk_steps"):
        S.PNDMScheduler.from_config({**SD15_PNDM_JSON, "skip_prk_steps": False})
    for cls in (S.PNDMScheduler, S.DPMSolverMultistepScheduler):
        with pytest.raises(NotImplementedError, match="prediction_type"):
            cls.from_config({**SD15_PNDM_JSON, "prediction_type": "v_prediction"})
        with pytest.raises(NotImplementedError):
            cls.from_config({**SD15_PNDM_JSON, "beta_schedule": "linear"})
        with pytest.raises(ValueError):
            cls(timestep_spacing="karras")
    # -inf, as json writes it, is the built value
    S.DPMSolverMultistepScheduler.from_config({**SD15_PNDM_JSON, "lambda_min_clipped": float("-inf"), "variance_type": None})


def test_pipeline_takes_the_new_schedulers():
    """``pipe.scheduler = PNDMScheduler.from_config(pipe.scheduler.config)`` reaches the engine; eta stays DDIM's"""
    from types import SimpleNamespace
    from consistentid_amd import pipeline
    base = S.DDIMScheduler.from_config(SD15_PNDM_JSON)
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(SimpleNamespace(device="cpu"), scheduler=base, use_graph=False)
    for cls in (S.PNDMScheduler, S.DPMSolverMultistepScheduler):
        pipe.scheduler = cls.from_config(pipe.scheduler.config)
        assert isinstance(pipe._engine.scheduler, cls) and pipe._engine.scheduler is pipe.scheduler
        assert pipe.scheduler.steps_offset == 1 and pipe.scheduler.multistep
        with pytest.raises(ValueError, match="DDIM"):
            pipe._variance_noise(1.0, None, None, torch.zeros(1, 4, 8, 8), 4)
    with pytest.raises(TypeError, match="PNDMScheduler"):
        pipe.scheduler = object()
    pipe.scheduler = S.DDIMScheduler.from_config(pipe.scheduler.config)
    assert not pipe.scheduler.multistep and pipe._variance_noise(0.0, None, None, torch.zeros(1, 4, 8, 8), 4) is None
    given = torch.zeros(4, 1, 4, 8, 8)
    assert pipe._variance_noise(1.0, None, given, torch.zeros(1, 4, 8, 8), 4) is given


def test_multistep_entry_refuses_bad_arguments(lib):
    """cid_cfg_multistep_step_f16 checks its arguments before it launches anything (no GPU needed): dummy non-null addresses"""
    f = lib.cid_cfg_multistep_step_f16
    p = 64
    ok = dict(eps=p, lat=p, hist=p, saved=p, z=None, z_rows=0, row=p, mask=None, init=None, noise=None, B=1, per=16)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["eps"], a["lat"], a["hist"], a["saved"], a["z"], a["z_rows"], a["row"], C.c_float(1.0), a["mask"], a["init"],
                 a["noise"], a["B"], a["per"], None)
    for name in ("eps", "lat", "hist", "saved", "row"):
        assert call(**{name: None}) == -22 and b"null pointer" in lib.cid_last_error(), name
    assert call(mask=p) == -22 and b"mask/init/noise" in lib.cid_last_error()
    assert call(mask=p, init=p) == -22 and call(init=p, noise=p) == -22
    assert call(B=1, per=12) == -22 and b"multiple of 8" in lib.cid_last_error()
    assert call(B=3, per=4) == -22
    assert call(z=p, z_rows=0) == -22 and call(z=None, z_rows=2) == -22
    assert lib.cid_version() >= 105
