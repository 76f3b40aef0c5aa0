"""Test-side restatement of the three samplers that run on cid_cfg_multistep_step_f16 -- PNDM (skip_prk_steps), DPM-Solver++
2M and DDIM with eta -- as STATEFUL step-by-step schedulers on torch ops, the way the published diffusers 0.23 classes
are written: lists of earlier model outputs, a counter, a remembered sample.  PARITY UNPINNED, like oracle/ddim.py
(diffusers is not vendored).  They carry oracle/ddim.py's interface, so ``oracle.loop.denoise`` drives them unchanged.

Nothing here knows the product's linear-coefficient rows: this file is the cross-check of that form.  ``RowEmulator`` at
the end is the other half of the cross-check, a float64 numpy model of the kernel's row contract (include/cid.h,
"multistep row") that is fed the product's rows.

Per-step coefficients are python floats computed in float64 from the float32 ``alphas_cumprod`` table of the Stable
Diffusion configs (scaled_linear betas 0.00085 .. 0.012 over 1000 steps)."""
from __future__ import annotations

import math

import numpy as np
import torch


def alphas_cumprod_table(beta_start=0.00085, beta_end=0.012, T=1000) -> np.ndarray:
    """the trained table: data of the model, not part of any sampler (float32, as the checkpoints' schedulers hold it)"""
    betas = np.linspace(np.float32(beta_start) ** 0.5, np.float32(beta_end) ** 0.5, T, dtype=np.float32) ** 2
    return np.cumprod((1.0 - betas).astype(np.float32), dtype=np.float32)


class _Base:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1, set_alpha_to_one=False,
                 timestep_spacing="leading"):
        self.T, self.steps_offset, self.timestep_spacing = num_train_timesteps, steps_offset, timestep_spacing
        self.ac = alphas_cumprod_table(beta_start, beta_end, num_train_timesteps).astype(np.float64)
        self.final_ac = 1.0 if set_alpha_to_one else float(self.ac[0])
        self.timesteps = None
        self.num_inference_steps = None

    def scale_model_input(self, sample, t=None):
        return sample

    def add_noise(self, original, noise, t):
        a = float(self.ac[int(t)])
        return math.sqrt(a) * original + math.sqrt(1.0 - a) * noise


class PNDMRef(_Base):
    """``PNDMScheduler(skip_prk_steps=True).step_plms``; ``set_timesteps`` makes a fresh scheduler (empty ``ets``)"""

    def set_timesteps(self, num_inference_steps, device=None):
        T, n = self.T, num_inference_steps
        self.num_inference_steps = n
        if self.timestep_spacing == "leading":
            base = np.arange(0, n) * (T // n) + self.steps_offset
        elif self.timestep_spacing == "linspace":
            base = np.linspace(0, T - 1, n).round()
        elif self.timestep_spacing == "trailing":
            base = np.round(np.arange(T, 0, -T / n))[::-1] - 1
        else:
            raise ValueError(self.timestep_spacing)
        base = base.astype(np.int64)
        plms = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        self.timesteps = torch.from_numpy(plms)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def _prev_sample(self, sample, t, prev, m):
        a_t = float(self.ac[t])
        a_p = float(self.ac[prev]) if prev >= 0 else self.final_ac
        sample_coeff = math.sqrt(a_p / a_t)
        denom = a_t * math.sqrt(1.0 - a_p) + math.sqrt(a_t * (1.0 - a_t) * a_p)
        return sample_coeff * sample - ((a_p - a_t) / denom) * m

    def step(self, eps, t, sample):
        t = int(t)
        ratio = self.T // self.num_inference_steps
        prev = t - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(eps)
        else:
            prev = t
            t = t + ratio
        ets = self.ets
        if len(ets) == 1 and self.counter == 0:
            m = eps
            self.cur_sample = sample
        elif len(ets) == 1 and self.counter == 1:
            m = (eps + ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(ets) == 2:
            m = (3 * ets[-1] - ets[-2]) / 2
        elif len(ets) == 3:
            m = (23 * ets[-1] - 16 * ets[-2] + 5 * ets[-3]) / 12
        else:
            m = (55 * ets[-1] - 59 * ets[-2] + 37 * ets[-3] - 9 * ets[-4]) / 24
        self.counter += 1
        return self._prev_sample(sample, t, prev, m)


class DPMSolverPP2MRef(_Base):
    """``DPMSolverMultistepScheduler(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint",
    lower_order_final=True)``: model outputs are converted to data predictions and kept in ``model_outputs``"""

    def __init__(self, *a, steps_offset=0, timestep_spacing="linspace", **kw):
        super().__init__(*a, steps_offset=steps_offset, timestep_spacing=timestep_spacing, **kw)

    def set_timesteps(self, num_inference_steps, device=None):
        T, n = self.T, num_inference_steps
        self.num_inference_steps = n
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1]
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1] + self.steps_offset
        elif self.timestep_spacing == "trailing":
            ts = np.arange(T, 0, -T / n).round() - 1
        else:
            raise ValueError(self.timestep_spacing)
        ts = ts.copy().astype(np.int64)
        train_sigmas = np.sqrt((1.0 - self.ac) / self.ac)
        sigmas = np.interp(ts, np.arange(0, T), train_sigmas)
        self.sigmas = np.concatenate([sigmas, [math.sqrt((1.0 - self.ac[0]) / self.ac[0])]])
        self.timesteps = torch.from_numpy(ts)
        self.model_outputs = [None, None]
        self.lower_order_nums = 0
        self.step_index = None

    def _alpha_sigma(self, i):
        sigma = float(self.sigmas[i])
        alpha_t = 1.0 / math.sqrt(sigma * sigma + 1.0)
        return alpha_t, sigma * alpha_t

    def step(self, eps, t, sample):
        if self.step_index is None:
            self.step_index = int((self.timesteps == int(t)).nonzero()[0])
        i = self.step_index
        alpha_s, sigma_s = self._alpha_sigma(i)
        alpha_t, sigma_t = self._alpha_sigma(i + 1)
        x0_pred = (sample - sigma_s * eps) / alpha_s
        self.model_outputs = [self.model_outputs[1], x0_pred]
        lower_order_final = i == len(self.timesteps) - 1 and len(self.timesteps) < 15
        lambda_t, lambda_s = math.log(alpha_t) - math.log(sigma_t), math.log(alpha_s) - math.log(sigma_s)
        h = lambda_t - lambda_s
        if self.lower_order_nums < 1 or lower_order_final:
            out = (sigma_t / sigma_s) * sample - (alpha_t * (math.exp(-h) - 1.0)) * x0_pred
        else:
            alpha_s1, sigma_s1 = self._alpha_sigma(i - 1)
            lambda_s1 = math.log(alpha_s1) - math.log(sigma_s1)
            m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
            r0 = (lambda_s - lambda_s1) / h
            d0, d1 = m0, (1.0 / r0) * (m0 - m1)
            out = (sigma_t / sigma_s) * sample - (alpha_t * (math.exp(-h) - 1.0)) * d0 \
                - 0.5 * (alpha_t * (math.exp(-h) - 1.0)) * d1
        if self.lower_order_nums < 2:
            self.lower_order_nums += 1
        self.step_index += 1
        return out


class DDIMEtaRef(_Base):
    """``DDIMScheduler.step(..., eta=, variance_noise=)``: ``noises`` is the list of pre-drawn tensors, consumed in call order"""

    def __init__(self, eta, noises, *a, **kw):
        super().__init__(*a, **kw)
        self.eta, self.noises = float(eta), list(noises)

    def set_timesteps(self, num_inference_steps, device=None):
        T, n = self.T, num_inference_steps
        self.num_inference_steps = n
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].astype(np.float64) + self.steps_offset
        elif self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n)[::-1]
        elif self.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / n)) - 1
        else:
            raise ValueError(self.timestep_spacing)
        self.timesteps = torch.from_numpy(ts.round().astype(np.int64))
        self.calls = 0

    def step(self, eps, t, sample):
        t = int(t)
        prev = t - self.T // self.num_inference_steps
        a_t = float(self.ac[t])
        a_p = float(self.ac[prev]) if prev >= 0 else self.final_ac
        variance = (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p)
        std = self.eta * math.sqrt(variance)
        x0 = (sample - math.sqrt(1.0 - a_t) * eps) / math.sqrt(a_t)
        direction = math.sqrt(1.0 - a_p - std * std) * eps
        noise = self.noises[self.calls].to(device=sample.device, dtype=sample.dtype)
        self.calls += 1
        return math.sqrt(a_p) * x0 + direction + std * noise


# ------------------------------------------------------------------------------------------------ the kernel's row contract
class RowEmulator:
    """float64 model of cid_cfg_multistep_step_f16 (include/cid.h, "multistep row").  The ring, ``saved`` and -- through
    ``z`` -- the noise rows start as NaN unless written: a row that weighs something nobody wrote shows up as a
    non-finite sample, and a buffer behind a zero coefficient is never touched, exactly like the kernel's branches."""

    def __init__(self, n: int, z=None):
        self.hist = np.full((4, n), np.nan)
        self.saved = np.full(n, np.nan)
        self.z = None if z is None else np.asarray(z, dtype=np.float64).reshape(len(z), n)

    def step(self, row, x, eps_u, eps_c, g, mask=None, init=None, noise=None):
        row = np.asarray(row, dtype=np.float64)
        a, b, c_x, c_m = row[0:4]
        c_hist, c_init, c_noise, c_z = row[4:8], row[9], row[10], row[11]
        w, flags, z_row = int(row[12]), int(row[13]), int(row[14])
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        e = eps_u.reshape(-1) + g * (eps_c.reshape(-1) - eps_u.reshape(-1))
        m = a * x + b * e
        src = self.saved.copy() if flags & 2 else x
        out = c_x * src + c_m * m
        for s in range(4):
            if c_hist[s] != 0.0:
                out = out + c_hist[s] * self.hist[s]
        if c_z != 0.0 and self.z is not None:
            out = out + c_z * self.z[min(max(z_row, 0), len(self.z) - 1)]
        if 0 <= w < 4:
            self.hist[w] = m
        if flags & 1:
            self.saved = x.copy()
        if mask is not None:
            k = mask.reshape(-1)
            out = (1.0 - k) * (c_init * init.reshape(-1) + c_noise * noise.reshape(-1)) + k * out
        return out
