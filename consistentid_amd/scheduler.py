"""Host side of the DDIM update used by the reference demos (demo/controlnet_demo.py:67;
loop call sites pipline_StableDiffusion_ConsistentID.py:510,540,569).  Stable Diffusion
scheduler config: scaled_linear betas 0.00085..0.012, 1000 train steps, epsilon prediction,
steps_offset 1, set_alpha_to_one False, eta 0; timestep spacing "leading" (the base models' configs) by default,
"linspace" / "trailing" on request; ``from_config`` takes a diffusers scheduler config.

Only tiny tables are computed here (float64 on the host, once); the per-element update runs
in cid_cfg_ddim_step_f16 which reads the coefficients from device memory.

``PNDMScheduler`` (the sampler the Stable Diffusion 1.5 model directory names), ``DPMSolverMultistepScheduler``
(DPM-Solver++ 2M) and DDIM with eta > 0 are linear multistep updates: a combination of the sample, the current model
output, earlier model outputs and a noise tensor.  They run in cid_cfg_multistep_step_f16, and each class writes its
per-step rows (include/cid.h, "multistep row") by simulating its own state machine over the schedule entries the loop
will run: ``coefficient_rows(inpaint, first_step, dtype)``.  The three algorithms are restated from the published
diffusers 0.23 schedulers, UNPINNED like oracle/ddim.py.

``prediction_type="v_prediction"`` (all four classes) and ``DDIMScheduler(rescale_betas_zero_snr=True)`` -- constructor
arguments, or keywords of ``from_config(config, **kwargs)`` -- are other coefficients in the same tables: the update stays linear in the sample and the model output.  A
schedule entry whose coefficients are not finite -- epsilon prediction at a timestep whose alphas_cumprod is 0, the terminal
step of a zero-SNR schedule -- raises ValueError when the table is built.

``LCMScheduler`` (multistep latent consistency sampling, 1 to 8 steps) is one more writer of such
rows: its update is linear in the sample, the model output and one fresh noise tensor per step.  At ``guidance_scale <= 1``
the engine steps it with cid_multistep_step_f16, the same row contract on ONE model output per sample (denoise.py)."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

SPACINGS = ("leading", "linspace", "trailing")
PREDICTION_TYPES = ("epsilon", "v_prediction")

ROW_WORDS = 16          # cid_cfg_multistep_step_f16's device row: words 0..11 fp32, 12..15 int32
C_IN, C_Z = 8, 11       # word of the model-input scale (16-byte aligned: conv_in reads it in place) / of z's coefficient
_W, _FLAGS, _ZROW = 12, 13, 14
FLAG_SAVE, FLAG_RESTORE = 1, 2


def _row(a=0.0, b=1.0, c_x=0.0, c_m=0.0, c_hist=(0.0, 0.0, 0.0, 0.0), c_z=0.0, c_init=1.0, c_noise=0.0, c_in=1.0,
         w=-1, flags=0, z_row=0) -> List[float]:
    return [a, b, c_x, c_m, *c_hist, c_in, c_init, c_noise, c_z, float(w), float(flags), float(z_row), 0.0]


def _idle_row() -> List[float]:
    """a schedule entry before ``first_step``: never selected; it writes nothing and weighs nothing"""
    return _row(c_x=1.0)


def pack_step_rows(rows: np.ndarray) -> np.ndarray:
    """rows [n, 16] as ``coefficient_rows`` returns them (every word a float, the integer words holding integer values)
    -> int32 [n, 16], the bit pattern the kernel reads: words 0..11 fp32, words 12..15 int32"""
    rows = np.asarray(rows)
    out = np.ascontiguousarray(rows.astype(np.float32)).view(np.int32).copy()
    out[:, _W:] = np.rint(rows[:, _W:]).astype(np.int32)
    return out


def _train_alphas_cumprod(beta_start: float, beta_end: float, T: int) -> np.ndarray:
    betas = np.linspace(np.float32(beta_start) ** 0.5, np.float32(beta_end) ** 0.5, T, dtype=np.float32) ** 2
    return np.cumprod((1.0 - betas).astype(np.float32), dtype=np.float32)


def rescale_zero_terminal_snr(betas: np.ndarray) -> np.ndarray:
    """diffusers 0.23 ``rescale_zero_terminal_snr`` (Algorithm 1 of "Common Diffusion Noise Schedules and Sample Steps Are
    Flawed") in float32 like the original: sqrt(alphas_cumprod) is shifted so that its last value is 0 and scaled so that its
    first one is kept; the betas are read back from the ratios.  The last beta is exactly 1, so alphas_cumprod[-1] == 0."""
    betas = np.asarray(betas, dtype=np.float32)
    bar_sqrt = np.sqrt(np.cumprod(np.float32(1.0) - betas, dtype=np.float32))
    first, last = bar_sqrt[0].copy(), bar_sqrt[-1].copy()
    bar_sqrt = (bar_sqrt - last) * (first / (first - last))
    bar = bar_sqrt ** 2
    alphas = np.concatenate([bar[0:1], bar[1:] / bar[:-1]]).astype(np.float32)
    return np.float32(1.0) - alphas


def _check_prediction_type(prediction_type: str) -> str:
    if prediction_type not in PREDICTION_TYPES:
        raise NotImplementedError(f"prediction_type {prediction_type!r}: the coefficient tables implement {PREDICTION_TYPES}")
    return prediction_type


def _check_finite(rows: np.ndarray, sch, what: str) -> np.ndarray:
    """the table-build-time refusal of a schedule the prediction type cannot step from"""
    flat = np.asarray(rows, dtype=np.float64)
    bad = np.flatnonzero(~np.isfinite(flat.reshape(len(flat), -1)).all(axis=1))
    if len(bad):
        ts = [float(sch.timesteps[i]) for i in bad]
        raise ValueError(f"{type(sch).__name__}.{what}: the coefficients of schedule entries {bad.tolist()} (timesteps {ts}) are "
                         f"not finite: with prediction_type {sch.prediction_type!r} the sample cannot be predicted from the "
                         "model output where alphas_cumprod is 0 (rescale_betas_zero_snr with a schedule that starts at the "
                         "last training timestep needs prediction_type='v_prediction')")
    return rows


class SchedulerConfig(dict):
    """``scheduler.config`` of an engine scheduler: the dict the reference scripts hand to ``Other.from_config(...)``.  Being
    this type is what tells ``from_config`` that the values describe a scheduler these tables already implement -- a
    v-prediction or zero-SNR scheduler's own config is taken over as it is -- where a raw diffusers config dict that names
    v-prediction or zero-SNR betas needs them confirmed as keywords (``_config_args``)."""


def _config_args(config, accepted, overrides=None) -> dict:
    """the arguments of a diffusers scheduler config (dict or FrozenDict-like) that this engine scheduler takes; refuses
    what the coefficient tables do not implement instead of silently computing something else.  ``overrides``: the keyword
    arguments of ``from_config(config, **kwargs)``, which replace the config's values as in diffusers.
    ``prediction_type="v_prediction"`` and ``rescale_betas_zero_snr`` are taken from an engine scheduler's own ``.config``
    (``Other.from_config(pipe.scheduler.config)`` keeps the pipeline's prediction type) and from keywords; a RAW config dict
    that names one of them is refused as it was before they were built -- callers that probe a config for support rely on
    that answer -- and ``loader.read_scheduler`` passes the saved prediction type on as a keyword."""
    cfg, overrides = dict(config), dict(overrides or {})
    own = isinstance(config, SchedulerConfig)
    unknown = sorted(set(overrides) - {"prediction_type", *accepted})
    if unknown:
        raise TypeError(f"from_config: unexpected keyword arguments {unknown}")
    if cfg.get("beta_schedule", "scaled_linear") != "scaled_linear" or cfg.get("trained_betas") is not None:
        raise NotImplementedError(f"beta_schedule {cfg.get('beta_schedule')!r} / trained_betas: only scaled_linear is built")
    if not own and "prediction_type" not in overrides and cfg.get("prediction_type", "epsilon") != "epsilon":
        raise NotImplementedError(f"prediction_type {cfg.get('prediction_type')!r} in a raw scheduler config is not taken over: "
                                  f"pass it explicitly, from_config(config, prediction_type=...) with one of {PREDICTION_TYPES}")
    zero_snr = bool(cfg.get("rescale_betas_zero_snr")) and "rescale_betas_zero_snr" not in overrides
    if zero_snr and "rescale_betas_zero_snr" not in accepted:
        raise NotImplementedError("rescale_betas_zero_snr: zero-SNR betas are built for DDIMScheduler only (the one of these "
                                  "classes that has the flag in diffusers 0.23)")
    if cfg.get("use_karras_sigmas") or cfg.get("interpolation_type", "linear") != "linear" or cfg.get("clip_sample") \
            or cfg.get("thresholding") or (zero_snr and not own):
        raise NotImplementedError("karras sigmas / log-linear interpolation / clip_sample / thresholding are not built; zero-SNR "
                                  "betas in a raw scheduler config are not taken over (DDIMScheduler takes rescale_betas_zero_snr "
                                  "as a keyword)")
    cfg.update(overrides)
    return {k: cfg[k] for k in ("prediction_type", *accepted) if k in cfg and cfg[k] is not None}


def _spaced_timesteps(T: int, n: int, spacing: str, offset: int) -> np.ndarray:
    """diffusers 0.23 ``set_timesteps`` (float64, descending): "leading" = multiples of T // n plus steps_offset,
    "linspace" = T - 1 ... 0 evenly, "trailing" = T - 1 downwards in steps of T / n"""
    if spacing == "leading":
        return (np.arange(0, n) * (T // n)).round()[::-1].astype(np.float64) + offset
    if spacing == "linspace":
        return np.linspace(0, T - 1, n)[::-1].astype(np.float64)
    if spacing == "trailing":
        return np.round(np.arange(T, 0, -T / n)).astype(np.float64) - 1
    raise ValueError(f"timestep_spacing {spacing!r}: one of {SPACINGS}")


def _next_blend(sch, inpaint: bool, i: int) -> Tuple[float, float]:
    """(c_init, c_noise) of the inpaint blend after schedule entry i: add_noise at the NEXT entry, identity after the last"""
    if inpaint and i < len(sch.timesteps) - 1:
        return sch.add_noise_coefficients(sch.timesteps[i + 1])
    return 1.0, 0.0


def _vp_sag_coefficients(a_t: float, prediction_type: str) -> Tuple[float, ...]:
    """(p_x, p_e, q_x, q_e, n_d, n_e) of self-attention guidance under a variance-preserving noise
    model at alphas_cumprod ``a_t``: x0 = p_x x + p_e out, ehat = q_x x + q_e out, and add_noise(D, ehat) = n_d D + n_e ehat"""
    sa, sb = a_t ** 0.5, (1.0 - a_t) ** 0.5
    if prediction_type == "v_prediction":
        return sa, -sb, sb, sa, sa, sb
    if a_t == 0.0:
        raise ValueError("sag_coefficients: the coefficients are not finite where alphas_cumprod is 0 -- with prediction_type "
                         "'epsilon' the sample cannot be predicted from the model output there (the terminal step of a zero-SNR "
                         "schedule needs prediction_type='v_prediction')")
    return 1.0 / sa, -sb / sa, 0.0, 1.0, sa, sb


def sag_coefficient_table(sch) -> np.ndarray:
    """[len(timesteps), 8] fp32: ``sch.sag_coefficients`` of every schedule entry (one row per UNet evaluation: PNDM's
    repeated timestep has a row of its own) and two zero words -- the step-table column cid_sag_degrade_f16 reads"""
    rows = [[*sch.sag_coefficients(t), 0.0, 0.0] for t in sch.timesteps]
    return _check_finite(np.asarray(rows, dtype=np.float64).reshape(-1, 8), sch, "sag_coefficients").astype(np.float32)


class DDIMScheduler:
    order = 1
    init_noise_sigma = 1.0
    multistep = False        # eta = 0 is cid_cfg_ddim_step_f16's two-coefficient update; eta > 0 takes coefficient_rows

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1, set_alpha_to_one: bool = False, timestep_spacing: str = "leading",
                 prediction_type: str = "epsilon", rescale_betas_zero_snr: bool = False):
        if timestep_spacing not in SPACINGS:
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: one of {SPACINGS}")
        self.prediction_type = _check_prediction_type(prediction_type)
        betas = np.linspace(np.float32(beta_start) ** 0.5, np.float32(beta_end) ** 0.5, num_train_timesteps,
                            dtype=np.float32) ** 2
        if rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        self.alphas_cumprod = np.cumprod((1.0 - betas).astype(np.float32), dtype=np.float32)
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset, self.timestep_spacing = steps_offset, timestep_spacing
        self.timesteps: np.ndarray = np.zeros(0, dtype=np.int64)
        self.num_inference_steps = 0
        # what ``OtherScheduler.from_config(pipe.scheduler.config)`` of the reference scripts reads
        self.config = SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", trained_betas=None, steps_offset=steps_offset,
                           set_alpha_to_one=set_alpha_to_one, timestep_spacing=timestep_spacing,
                           prediction_type=prediction_type, clip_sample=False,
                           rescale_betas_zero_snr=bool(rescale_betas_zero_snr))

    @classmethod
    def from_config(cls, config, **kwargs) -> "DDIMScheduler":
        """``DDIMScheduler.from_config(pipe.scheduler.config)`` (demo/controlnet_demo.py:67): a diffusers scheduler config
        (the dict of ``scheduler/scheduler_config.json``, or ``scheduler.config``) -> the engine's coefficient tables"""
        return cls(**_config_args(config, ("num_train_timesteps", "beta_start", "beta_end", "steps_offset", "set_alpha_to_one",
                                           "timestep_spacing", "rescale_betas_zero_snr"), kwargs))

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts = _spaced_timesteps(self.num_train_timesteps, num_inference_steps, self.timestep_spacing, self.steps_offset)
        self.timesteps = ts.round().astype(np.int64)

    def _step_pair(self, t: int, sigma: float = 0.0) -> Tuple[float, float]:
        """(c_x, c_out) of x' = c_x x + c_out model_output [+ sigma z].  v-prediction: x0 = sqrt(a_t) x - sqrt(1 - a_t) v and
        eps = sqrt(a_t) v + sqrt(1 - a_t) x go into x' = sqrt(a_p) x0 + sqrt(1 - a_p - sigma^2) eps as they are -- nothing is
        divided by sqrt(a_t), so the pair is finite at a_t = 0 (the terminal step of a zero-SNR schedule).  Epsilon
        prediction divides there: inf / nan, which the table builders refuse."""
        a_t, a_p = self.alphas(t)
        d = (1.0 - a_p - sigma * sigma) ** 0.5
        if self.prediction_type == "v_prediction":
            return (a_p ** 0.5) * (a_t ** 0.5) + d * ((1.0 - a_t) ** 0.5), d * (a_t ** 0.5) - (a_p ** 0.5) * ((1.0 - a_t) ** 0.5)
        if a_t == 0.0:
            return float("inf"), float("nan")
        return (a_p / a_t) ** 0.5, d - (a_p ** 0.5) * ((1.0 - a_t) ** 0.5) / (a_t ** 0.5)

    def scale_model_input(self, sample, t=None):
        return sample

    def alphas(self, t: int) -> Tuple[float, float]:
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_p

    def step_coefficients(self, t: int) -> Tuple[float, float]:
        """x_prev = c_x * x + c_out * model_output  (eta = 0; the model output is eps or v, by ``prediction_type``)."""
        return self._step_pair(t)

    def add_noise_coefficients(self, t) -> Tuple[float, float]:
        a = float(self.alphas_cumprod[int(t)])
        return a ** 0.5, (1.0 - a) ** 0.5

    def sag_coefficients(self, t) -> Tuple[float, ...]:
        """(p_x, p_e, q_x, q_e, n_d, n_e) at timestep ``t``: the predicted sample, the predicted noise and add_noise at ``t``"""
        return _vp_sag_coefficients(float(self.alphas_cumprod[int(t)]), self.prediction_type)

    def coefficient_table(self, inpaint: bool = False) -> np.ndarray:
        """[steps, 4] fp32: c_x, c_eps, c_init, c_noise (last two for the inpaint blend of the
        NEXT timestep, CN :437-449; identity on the final step)."""
        rows: List[List[float]] = []
        ts = self.timesteps
        for i, t in enumerate(ts):
            c_x, c_e = self.step_coefficients(int(t))
            ci, cn = 1.0, 0.0
            if inpaint and i < len(ts) - 1:
                ci, cn = self.add_noise_coefficients(int(ts[i + 1]))
            rows.append([c_x, c_e, ci, cn, 1.0])          # last column: model-input scale (identity for DDIM)
        return _check_finite(np.asarray(rows, dtype=np.float32), self, "coefficient_table")

    def coefficient_rows(self, inpaint: bool = False, first_step: int = 0, dtype=np.float32, eta: float = 0.0) -> np.ndarray:
        """[len(timesteps), 16] multistep rows of DDIM with ``eta`` (diffusers' ``step(..., eta=, variance_noise=)``):
        sigma_t = eta sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)),
        x' = sqrt(a_prev) (x - sqrt(1 - a_t) e) / sqrt(a_t) + sqrt(1 - a_prev - sigma_t^2) e + sigma_t z[k],
        k counting the executed steps from ``first_step``; v-prediction as in ``_step_pair``.  The engine takes this path for
        eta > 0 only."""
        ts = self.timesteps
        rows = [_idle_row() for _ in range(min(first_step, len(ts)))]
        for i in range(first_step, len(ts)):
            a_t, a_p = self.alphas(int(ts[i]))
            sigma = float(eta) * ((1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p)) ** 0.5
            c_x, c_e = self._step_pair(int(ts[i]), sigma)
            ci, cn = _next_blend(self, inpaint, i)
            rows.append(_row(c_x=c_x, c_m=c_e, c_z=sigma, c_init=ci, c_noise=cn, z_row=i - first_step))
        return _check_finite(np.asarray(rows, dtype=np.float64).reshape(-1, ROW_WORDS), self, "coefficient_rows").astype(dtype)


class EulerDiscreteScheduler:
    """The scheduler of the reference's canonical scripts (infer.py:33, infer_SDXL.py:37:
    ``EulerDiscreteScheduler.from_config(pipe.scheduler.config)``; SD config: scaled_linear betas, steps_offset 1, "leading"
    spacing; epsilon prediction, linear sigma interpolation, s_churn 0).  In the engine's terms it is the same per-element
    update as DDIM with other coefficients -- x_prev = x + (sigma_next - sigma) * eps -- plus a model-input scale
    1 / sqrt(sigma^2 + 1) (applied inside conv_in) and an initial latent scale ``init_noise_sigma``."""
    order = 1
    multistep = False

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1, timestep_spacing: str = "leading", prediction_type: str = "epsilon"):
        # "leading" is what ``EulerDiscreteScheduler.from_config(pipe.scheduler.config)`` inherits from the base models'
        # PNDM / DDIM / Euler scheduler configs (a loaded scheduler's config carries every init argument, defaults included);
        # diffusers' own class default would be "linspace" -- pass the base model's config to from_config to be sure
        if timestep_spacing not in SPACINGS:
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: one of {SPACINGS}")
        self.prediction_type = _check_prediction_type(prediction_type)
        betas = np.linspace(np.float32(beta_start) ** 0.5, np.float32(beta_end) ** 0.5, num_train_timesteps,
                            dtype=np.float32) ** 2
        ac = np.cumprod((1.0 - betas).astype(np.float32), dtype=np.float32)
        self._train_sigmas = np.array(((1 - ac) / ac) ** 0.5)
        self.num_train_timesteps, self.steps_offset, self.timestep_spacing = num_train_timesteps, steps_offset, timestep_spacing
        self.sigmas = np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32)
        self.timesteps: np.ndarray = np.zeros(0, dtype=np.float32)
        self.num_inference_steps = 0
        self.config = SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", trained_betas=None, steps_offset=steps_offset,
                           timestep_spacing=timestep_spacing, prediction_type=prediction_type, interpolation_type="linear",
                           use_karras_sigmas=False)

    @classmethod
    def from_config(cls, config, **kwargs) -> "EulerDiscreteScheduler":
        """``EulerDiscreteScheduler.from_config(pipe.scheduler.config)`` (infer.py:33, infer_SDXL.py:37).  A raw
        ``scheduler_config.json`` without a ``timestep_spacing`` key belongs to a scheduler class whose default is
        "leading" (PNDM, DDIM): that is what the loaded scheduler's config would hand over, so it is the fallback here."""
        return cls(**_config_args(config, ("num_train_timesteps", "beta_start", "beta_end", "steps_offset", "timestep_spacing"),
                                  kwargs))

    @property
    def init_noise_sigma(self) -> float:
        """diffusers 0.23: max sigma of the CURRENT table for "linspace" / "trailing" spacing, sqrt(max sigma^2 + 1) for
        "leading".  The pipelines call set_timesteps before prepare_latents (ref :510 then :517), so this is the first
        inference sigma, not the training maximum"""
        m = float(self.sigmas.max())
        return m if self.timestep_spacing in ("linspace", "trailing") else float((m ** 2 + 1) ** 0.5)

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts = _spaced_timesteps(self.num_train_timesteps, num_inference_steps, self.timestep_spacing,
                               self.steps_offset).astype(np.float32)
        sig = np.interp(ts, np.arange(0, len(self._train_sigmas)), self._train_sigmas)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = ts

    def add_noise_coefficients(self, t: float):
        """add_noise(original, noise, t) = original + sigma(t) * noise (t: one of the current inference timesteps)"""
        i = int(np.argmin(np.abs(self.timesteps - float(t))))
        return 1.0, float(self.sigmas[i])

    def sag_coefficients(self, t) -> Tuple[float, ...]:
        """(p_x, p_e, q_x, q_e, n_d, n_e) at inference timestep ``t``, in this sampler's own variables (x = x0 + sigma eps; the
        model input is scaled by c_in like every other): epsilon prediction x0 = x - sigma e, ehat = e; v-prediction
        x0 = x / (sigma^2 + 1) - sigma v / sqrt(sigma^2 + 1), ehat = (x - x0) / sigma; add_noise(D, ehat) = D + sigma ehat"""
        sg = self.add_noise_coefficients(t)[1]
        if self.prediction_type == "v_prediction":
            r = (sg * sg + 1.0) ** 0.5
            return 1.0 / (r * r), -sg / r, sg / (r * r), 1.0 / r, 1.0, sg
        return 1.0, -sg, 0.0, 1.0, 1.0, sg

    def coefficient_table(self, inpaint: bool = False) -> np.ndarray:
        """[steps, 5] fp32: c_x, c_eps, c_init, c_noise, c_in (see DDIMScheduler.coefficient_table).  v-prediction (diffusers:
        pred_original = -sigma v / sqrt(sigma^2 + 1) + x / (sigma^2 + 1), derivative = (x - pred_original) / sigma):
        x' = x (1 + dt sigma / (sigma^2 + 1)) + v dt / sqrt(sigma^2 + 1), dt = sigma_next - sigma; c_in is the same."""
        rows: List[List[float]] = []
        for i in range(len(self.timesteps)):
            s, nxt = float(self.sigmas[i]), float(self.sigmas[i + 1])
            ci, cn = 1.0, 0.0
            if inpaint and i < len(self.timesteps) - 1:
                ci, cn = 1.0, nxt                           # add_noise at the NEXT timestep: init + sigma_next * noise
            c_x, c_e = 1.0, nxt - s
            if self.prediction_type == "v_prediction":
                c_x, c_e = 1.0 + (nxt - s) * s / (s * s + 1.0), (nxt - s) / (s * s + 1.0) ** 0.5
            rows.append([c_x, c_e, ci, cn, 1.0 / (s * s + 1.0) ** 0.5])
        return _check_finite(np.asarray(rows, dtype=np.float32), self, "coefficient_table")


class PNDMScheduler:
    """The scheduler Stable Diffusion 1.5's model directory names (``scheduler/scheduler_config.json``: PNDMScheduler,
    skip_prk_steps true, steps_offset 1): ``pipe.scheduler = PNDMScheduler.from_config(pipe.scheduler.config)`` samples
    with the model's own sampler.  Built: ``skip_prk_steps=True`` (the linear multistep part, no Runge-Kutta warm-up) and
    epsilon prediction.  The timestep list has num_inference_steps + 1 entries -- the second timestep comes twice: the
    first step is taken once with its own model output and redone from the remembered sample with the mean of two -- so
    a generation is num_inference_steps + 1 UNet evaluations (one for a single step)."""
    order = 1
    init_noise_sigma = 1.0
    multistep = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1, set_alpha_to_one: bool = False, timestep_spacing: str = "leading",
                 skip_prk_steps: bool = True, prediction_type: str = "epsilon"):
        self.prediction_type = _check_prediction_type(prediction_type)
        if not skip_prk_steps:
            raise NotImplementedError("skip_prk_steps=False: the Runge-Kutta warm-up steps are not built")
        if timestep_spacing not in SPACINGS:
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: one of {SPACINGS}")
        self.alphas_cumprod = _train_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset, self.timestep_spacing = steps_offset, timestep_spacing
        self.timesteps: np.ndarray = np.zeros(0, dtype=np.int64)
        self.num_inference_steps = 0
        self.config = SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", trained_betas=None, steps_offset=steps_offset,
                           set_alpha_to_one=set_alpha_to_one, timestep_spacing=timestep_spacing,
                           prediction_type=prediction_type, skip_prk_steps=True)

    @classmethod
    def from_config(cls, config, **kwargs) -> "PNDMScheduler":
        """a config without ``skip_prk_steps`` (another scheduler class's) gets the built variant; an explicit false raises"""
        return cls(**_config_args(config, ("num_train_timesteps", "beta_start", "beta_end", "steps_offset", "set_alpha_to_one",
                                           "timestep_spacing", "skip_prk_steps"), kwargs))

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.num_train_timesteps, num_inference_steps
        self.num_inference_steps = n
        if self.timestep_spacing == "leading":
            t = np.arange(0, n) * (T // n) + self.steps_offset
        elif self.timestep_spacing == "linspace":
            t = np.linspace(0, T - 1, n).round()
        else:
            t = np.round(np.arange(T, 0, -T / n))[::-1] - 1
        t = t.astype(np.int64)
        self.timesteps = np.concatenate([t[:-1], t[-2:-1], t[-1:]])[::-1].copy()

    def scale_model_input(self, sample, t=None):
        return sample

    def add_noise_coefficients(self, t) -> Tuple[float, float]:
        a = float(self.alphas_cumprod[int(t)])
        return a ** 0.5, (1.0 - a) ** 0.5

    def sag_coefficients(self, t) -> Tuple[float, ...]:
        """(p_x, p_e, q_x, q_e, n_d, n_e) at timestep ``t``: the predicted sample, the predicted noise and add_noise at ``t``"""
        return _vp_sag_coefficients(float(self.alphas_cumprod[int(t)]), self.prediction_type)

    def coefficient_rows(self, inpaint: bool = False, first_step: int = 0, dtype=np.float32) -> np.ndarray:
        """[len(timesteps), 16] multistep rows: ``step_plms`` over entries [first_step, len) with a counter and a history
        that start empty at ``first_step``, as a fresh scheduler stepping over the truncated list does.  The kernel's m is
        the model output itself (a = 0, b = 1); ring slot k mod 4 takes the k-th appended one.  v-prediction: ``_get_prev_sample``
        converts the COMBINED output with the step's source sample, eps = sqrt(a_t) v + sqrt(1 - a_t) src; the combination's
        weights sum to 1, so every model-output coefficient is multiplied by sqrt(a_t) and c_x gains c_mo sqrt(1 - a_t)."""
        ts, T = self.timesteps, self.num_train_timesteps
        ratio = T // self.num_inference_steps
        rows = [_idle_row() for _ in range(min(first_step, len(ts)))]
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
            if self.prediction_type == "v_prediction":
                c_x, c_mo = c_x + c_mo * (1.0 - a_t) ** 0.5, c_mo * a_t ** 0.5
            held = min(appended, 4)
            slot = lambda back: (appended - back) % 4          # ring slot of ets[-back]
            if counter == 1:                                    # (e + ets[-1]) / 2 from the remembered sample
                c_m, flags = 0.5 * c_mo, FLAG_RESTORE
                c_hist[slot(1)] = 0.5 * c_mo
            else:                                               # ets[-1] is this step's e, written after the reads
                weights = {1: (1.0,), 2: (1.5, -0.5), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[held]
                c_m = weights[0] * c_mo
                for back, wt in enumerate(weights[1:], start=2):
                    c_hist[slot(back)] = wt * c_mo
                if counter == 0:
                    flags = FLAG_SAVE
            ci, cn = _next_blend(self, inpaint, i)
            rows.append(_row(a=0.0, b=1.0, c_x=c_x, c_m=c_m, c_hist=c_hist, c_init=ci, c_noise=cn, w=w, flags=flags))
            counter += 1
        return _check_finite(np.asarray(rows, dtype=np.float64).reshape(-1, ROW_WORDS), self, "coefficient_rows").astype(dtype)


class DPMSolverMultistepScheduler:
    """DPM-Solver++ (2M): ``algorithm_type="dpmsolver++"``, ``solver_order=2``, ``solver_type="midpoint"``,
    ``lower_order_final=True``, epsilon prediction -- what ``DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)``
    gives on the Stable Diffusion configs.  The kernel's m is the data prediction (x - sigma_i e) / alpha_i, kept in the
    fp32 ring; the second-order step weighs m_i and m_(i-1).  The first executed step is first order, and so is the last
    one of a schedule shorter than 15 (``lower_order_final``)."""
    order = 1
    init_noise_sigma = 1.0
    multistep = True

    _BUILT = dict(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", lower_order_final=True,
                  use_karras_sigmas=False, thresholding=False, lambda_min_clipped=-float("inf"), variance_type=None,
                  euler_at_final=False, use_lu_lambdas=False)

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 0, timestep_spacing: str = "linspace", prediction_type: str = "epsilon"):
        if timestep_spacing not in SPACINGS:
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: one of {SPACINGS}")
        self.prediction_type = _check_prediction_type(prediction_type)
        self.alphas_cumprod = _train_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        ac = self.alphas_cumprod.astype(np.float64)
        self._train_sigmas = ((1.0 - ac) / ac) ** 0.5
        self.num_train_timesteps, self.steps_offset, self.timestep_spacing = num_train_timesteps, steps_offset, timestep_spacing
        self.timesteps: np.ndarray = np.zeros(0, dtype=np.int64)
        self.sigmas: np.ndarray = np.zeros(0, dtype=np.float64)
        self.num_inference_steps = 0
        self.config = SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", trained_betas=None, steps_offset=steps_offset,
                           timestep_spacing=timestep_spacing, prediction_type=prediction_type, **self._BUILT)

    @classmethod
    def from_config(cls, config, **kwargs) -> "DPMSolverMultistepScheduler":
        """a config without ``timestep_spacing`` belongs to a class whose default is "leading" (PNDM, DDIM; see
        EulerDiscreteScheduler.from_config); diffusers' own default for this class, "linspace", is the constructor's"""
        cfg = dict(config)
        for key, built in cls._BUILT.items():
            got = cfg.get(key, built)
            if key == "lambda_min_clipped":
                ok = got is None or float(got) == built
            elif key == "variance_type":
                ok = got is None or not str(got).startswith("learned")      # a learned variance doubles the UNet's channels
            else:
                ok = got == built
            if not ok:
                raise NotImplementedError(f"{key}={got!r}: DPMSolverMultistepScheduler is built for {key}={built!r} only")
        args = _config_args(config, ("num_train_timesteps", "beta_start", "beta_end", "steps_offset", "timestep_spacing"), kwargs)
        args.setdefault("timestep_spacing", "leading")
        return cls(**args)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.num_train_timesteps, num_inference_steps
        self.num_inference_steps = n
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1]
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1] + self.steps_offset
        else:
            ts = np.arange(T, 0, -T / n).round() - 1
        self.timesteps = ts.astype(np.int64)
        sig = np.interp(self.timesteps, np.arange(0, T), self._train_sigmas)
        self.sigmas = np.concatenate([sig, self._train_sigmas[:1]])

    def scale_model_input(self, sample, t=None):
        return sample

    def add_noise_coefficients(self, t) -> Tuple[float, float]:
        a = float(self.alphas_cumprod[int(t)])
        return a ** 0.5, (1.0 - a) ** 0.5

    def sag_coefficients(self, t) -> Tuple[float, ...]:
        """(p_x, p_e, q_x, q_e, n_d, n_e) at timestep ``t``: the predicted sample, the predicted noise and add_noise at ``t``"""
        return _vp_sag_coefficients(float(self.alphas_cumprod[int(t)]), self.prediction_type)

    def coefficient_rows(self, inpaint: bool = False, first_step: int = 0, dtype=np.float32) -> np.ndarray:
        """[len(timesteps), 16] multistep rows over entries [first_step, len); the history starts empty at ``first_step``.
        With alpha = 1 / sqrt(sigma^2 + 1), s = sigma alpha, lambda = log alpha - log s, h = lambda_(i+1) - lambda_i,
        D = -alpha_(i+1) (exp(-h) - 1):  x' = (s_(i+1) / s_i) x + D m_i  [+ D / (2 r) (m_i - m_(i-1)),
        r = (lambda_i - lambda_(i-1)) / h].  m is the data prediction: (x - s_i e) / alpha_i for epsilon prediction,
        alpha_i x - s_i v for v-prediction."""
        n = len(self.timesteps)
        alpha = 1.0 / (self.sigmas ** 2 + 1.0) ** 0.5
        s = self.sigmas * alpha
        lam = np.log(alpha) - np.log(s)
        rows = [_idle_row() for _ in range(min(first_step, n))]
        for i in range(first_step, n):
            k = i - first_step
            h = lam[i + 1] - lam[i]
            D = -alpha[i + 1] * (np.exp(-h) - 1.0)
            c_m, c_hist = D, [0.0] * 4
            if k > 0 and not (i == n - 1 and n < 15):
                r = (lam[i] - lam[i - 1]) / h
                c_m = D + D / (2.0 * r)
                c_hist[(k - 1) % 4] = -D / (2.0 * r)
            ci, cn = _next_blend(self, inpaint, i)
            a, b = (alpha[i], -s[i]) if self.prediction_type == "v_prediction" else (1.0 / alpha[i], -s[i] / alpha[i])
            rows.append(_row(a=a, b=b, c_x=s[i + 1] / s[i], c_m=float(c_m), c_hist=c_hist,
                             c_init=ci, c_noise=cn, w=k % 4))
        return _check_finite(np.asarray(rows, dtype=np.float64).reshape(-1, ROW_WORDS), self, "coefficient_rows").astype(dtype)


class LCMScheduler:
    """Multistep latent consistency sampling (Luo et al. 2023, "Latent Consistency Models", Algorithm 3) with diffusers
    0.23's defaults: what ``pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)`` gives beside an LCM-LoRA or
    on a distilled checkpoint.  Restated from the published algorithm, UNPINNED like the other samplers here (diffusers is
    not vendored).  The schedule is a subset of the ``original_inference_steps`` timesteps the model was distilled on:
    c = T // original_inference_steps, origin = c, 2c, ... minus 1, every (original_inference_steps // n)-th of them from
    the top -- 4 steps are [999, 759, 519, 279].  With s = timestep_scaling t, c_skip = sigma_data^2 / (s^2 + sigma_data^2)
    and c_out = s / sqrt(s^2 + sigma_data^2), a step denoises and, but for the last one, noises again to the next timestep:
        den = c_out x0 + c_skip x;    x' = sqrt(a_next) den + sqrt(1 - a_next) z_k    (x' = den on the last step)
    with x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t) for epsilon prediction and sqrt(a_t) x - sqrt(1 - a_t) v for v-prediction.
    z_k is a fresh standard normal tensor per executed step k, drawn before the loop (pipeline ``_variance_noise``) or given
    as ``variance_noise`` [executed steps - 1, B, C, h, w]; the final latents carry no noise.  ``steps_offset``,
    ``set_alpha_to_one`` and ``timestep_spacing`` are carried in ``.config`` for the class a later ``from_config`` builds; the
    LCM schedule does not use them (neither does diffusers')."""
    order = 1
    init_noise_sigma = 1.0
    multistep = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 original_inference_steps: int = 50, timestep_scaling: float = 10.0, sigma_data: float = 0.5,
                 prediction_type: str = "epsilon", steps_offset: int = 0, set_alpha_to_one: bool = True,
                 timestep_spacing: str = "leading"):
        if timestep_spacing not in SPACINGS:
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: one of {SPACINGS}")
        if not 1 <= int(original_inference_steps) <= num_train_timesteps:
            raise ValueError(f"original_inference_steps = {original_inference_steps!r}: 1 .. num_train_timesteps")
        self.prediction_type = _check_prediction_type(prediction_type)
        self.alphas_cumprod = _train_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        self.num_train_timesteps, self.original_inference_steps = num_train_timesteps, int(original_inference_steps)
        self.timestep_scaling, self.sigma_data = float(timestep_scaling), float(sigma_data)
        self.steps_offset, self.timestep_spacing = steps_offset, timestep_spacing
        self.timesteps: np.ndarray = np.zeros(0, dtype=np.int64)
        self.num_inference_steps = 0
        self.config = SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", trained_betas=None, steps_offset=steps_offset,
                           set_alpha_to_one=set_alpha_to_one, timestep_spacing=timestep_spacing,
                           prediction_type=prediction_type, original_inference_steps=int(original_inference_steps),
                           timestep_scaling=float(timestep_scaling), sigma_data=float(sigma_data), clip_sample=False,
                           thresholding=False)

    @classmethod
    def from_config(cls, config, **kwargs) -> "LCMScheduler":
        """``LCMScheduler.from_config(pipe.scheduler.config)``: betas and prediction type of the pipeline's scheduler, the
        LCM defaults for what its config does not name"""
        return cls(**_config_args(config, ("num_train_timesteps", "beta_start", "beta_end", "original_inference_steps",
                                           "timestep_scaling", "sigma_data", "steps_offset", "set_alpha_to_one",
                                           "timestep_spacing"), kwargs))

    def set_timesteps(self, num_inference_steps: int, device=None):
        n, orig = int(num_inference_steps), self.original_inference_steps
        if n < 1 or n > orig:
            raise ValueError(f"num_inference_steps = {num_inference_steps!r}: LCMScheduler takes 1 .. original_inference_steps "
                             f"= {orig} steps")
        self.num_inference_steps = n
        origin = np.arange(1, orig + 1, dtype=np.int64) * (self.num_train_timesteps // orig) - 1
        self.timesteps = origin[::-(orig // n)][:n].copy()

    def scale_model_input(self, sample, t=None):
        return sample

    def add_noise_coefficients(self, t) -> Tuple[float, float]:
        a = float(self.alphas_cumprod[int(t)])
        return a ** 0.5, (1.0 - a) ** 0.5

    def boundary_scalings(self, t) -> Tuple[float, float]:
        """(c_skip, c_out) of the consistency parameterisation at timestep t"""
        s, sd = self.timestep_scaling * float(t), self.sigma_data
        return sd * sd / (s * s + sd * sd), s / (s * s + sd * sd) ** 0.5

    def sag_coefficients(self, t) -> Tuple[float, ...]:
        """(p_x, p_e, q_x, q_e, n_d, n_e) at timestep ``t``: the predicted sample, the predicted noise and add_noise at ``t``"""
        return _vp_sag_coefficients(float(self.alphas_cumprod[int(t)]), self.prediction_type)

    def coefficient_rows(self, inpaint: bool = False, first_step: int = 0, dtype=np.float32) -> np.ndarray:
        """[len(timesteps), 16] multistep rows over entries [first_step, len).  The kernel's m is the predicted sample x0
        (a, b by prediction type), x' = f c_skip x + f c_out m + g z[k] with (f, g) = (sqrt(a_next), sqrt(1 - a_next)) and
        k = i - first_step, or (1, 0) on the last entry, which reads no noise row.  No ring slot, no flags."""
        ts = self.timesteps
        rows = [_idle_row() for _ in range(min(first_step, len(ts)))]
        for i in range(first_step, len(ts)):
            a_t = float(self.alphas_cumprod[int(ts[i])])
            c_skip, c_out = self.boundary_scalings(ts[i])
            if self.prediction_type == "v_prediction":
                a, b = a_t ** 0.5, -(1.0 - a_t) ** 0.5
            elif a_t == 0.0:
                a, b = float("inf"), float("nan")
            else:
                a, b = 1.0 / a_t ** 0.5, -(1.0 - a_t) ** 0.5 / a_t ** 0.5
            f, g, z_row = 1.0, 0.0, 0
            if i < len(ts) - 1:
                f, g = self.add_noise_coefficients(ts[i + 1])
                z_row = i - first_step
            ci, cn = _next_blend(self, inpaint, i)
            rows.append(_row(a=a, b=b, c_x=f * c_skip, c_m=f * c_out, c_z=g, c_init=ci, c_noise=cn, z_row=z_row))
        return _check_finite(np.asarray(rows, dtype=np.float64).reshape(-1, ROW_WORDS), self, "coefficient_rows").astype(dtype)
