"""Test-side restatement of the four samplers' diffusers 0.23 ``step`` functions WITH ``prediction_type`` ("epsilon" /
"v_prediction") and, for DDIM, ``rescale_betas_zero_snr`` and ``eta``: stateful step-by-step schedulers in float64 python
floats on torch ops, written the way the published classes are -- predict the original sample, then step -- and not as the
product's linear coefficient rows, which they cross-check.  PARITY UNPINNED, like oracle/ddim.py and tests/multistep_ref.py
(diffusers is not vendored).  They carry the interface tests/multistep_ref.py's classes expose to ``oracle.loop.denoise``.

``rescale_noise_cfg`` and ``RescaledUNet`` restate diffusers' guidance_rescale for the trajectory tests."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from multistep_ref import DDIMEtaRef, DPMSolverPP2MRef, PNDMRef, alphas_cumprod_table

PREDICTION_TYPES = ("epsilon", "v_prediction")


def zero_snr_alphas_cumprod(beta_start=0.00085, beta_end=0.012, T=1000) -> np.ndarray:
    """diffusers' ``rescale_zero_terminal_snr`` on the scaled_linear betas, line by line in float32 as the original, then
    DDIMScheduler.__init__'s cumulative product.  numpy float32 like ``alphas_cumprod_table``, not torch: the trained table
    is data of the model, torch's float32 linspace and cumprod differ from numpy's in the last bit of most entries, and
    1 - alphas_cumprod[0] = 8.5e-4 magnifies such a bit a thousandfold in the last step's coefficients."""
    one = np.float32(1.0)
    betas = np.linspace(np.float32(beta_start) ** 0.5, np.float32(beta_end) ** 0.5, T, dtype=np.float32) ** 2
    alphas = one - betas
    alphas_cumprod = np.cumprod(alphas, dtype=np.float32)
    alphas_bar_sqrt = np.sqrt(alphas_cumprod)
    alphas_bar_sqrt_0 = alphas_bar_sqrt[0].copy()
    alphas_bar_sqrt_T = alphas_bar_sqrt[-1].copy()
    alphas_bar_sqrt -= alphas_bar_sqrt_T                                            # shift so the last timestep is zero
    alphas_bar_sqrt *= alphas_bar_sqrt_0 / (alphas_bar_sqrt_0 - alphas_bar_sqrt_T)  # scale so the first timestep is back
    alphas_bar = alphas_bar_sqrt * alphas_bar_sqrt
    alphas = alphas_bar[1:] / alphas_bar[:-1]
    alphas = np.concatenate([alphas_bar[0:1], alphas])
    betas = one - alphas
    assert betas.dtype == np.float32
    return np.cumprod(one - betas, dtype=np.float32)


def _check(prediction_type):
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(prediction_type)
    return prediction_type


class DDIMRef(DDIMEtaRef):
    """``DDIMScheduler.step(model_output, t, sample, eta=, variance_noise=)``; ``noises`` only for eta > 0"""

    def __init__(self, prediction_type="epsilon", rescale_betas_zero_snr=False, eta=0.0, noises=(), **kw):
        super().__init__(eta, noises, **kw)
        self.prediction_type = _check(prediction_type)
        if rescale_betas_zero_snr:
            self.ac = zero_snr_alphas_cumprod(kw.get("beta_start", 0.00085), kw.get("beta_end", 0.012), self.T).astype(np.float64)
            self.final_ac = 1.0 if kw.get("set_alpha_to_one", False) else float(self.ac[0])

    def step(self, model_output, t, sample):
        t = int(t)
        prev = t - self.T // self.num_inference_steps
        a_t = float(self.ac[t])
        a_p = float(self.ac[prev]) if prev >= 0 else self.final_ac
        b_t = 1.0 - a_t
        if self.prediction_type == "epsilon":
            x0 = (sample - math.sqrt(b_t) * model_output) / math.sqrt(a_t)
            eps = model_output
        else:
            x0 = math.sqrt(a_t) * sample - math.sqrt(b_t) * model_output
            eps = math.sqrt(a_t) * model_output + math.sqrt(b_t) * sample
        variance = (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p)
        std = self.eta * math.sqrt(variance)
        out = math.sqrt(a_p) * x0 + math.sqrt(1.0 - a_p - std * std) * eps
        if self.eta > 0:
            out = out + std * self.noises[self.calls].to(device=sample.device, dtype=sample.dtype)
        self.calls += 1
        return out


class EulerRef:
    """``EulerDiscreteScheduler.step`` (s_churn 0, linear interpolation): sigma_hat = sigma, derivative = (x - x0) / sigma"""
    order = 1

    def __init__(self, prediction_type="epsilon", num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 timestep_spacing="leading"):
        self.prediction_type = _check(prediction_type)
        self.T, self.steps_offset, self.timestep_spacing = num_train_timesteps, steps_offset, timestep_spacing
        ac = alphas_cumprod_table(beta_start, beta_end, num_train_timesteps)
        self._train_sigmas = np.array(((1 - ac) / ac) ** 0.5)
        self.sigmas = np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32)
        self.timesteps = None

    @property
    def init_noise_sigma(self):
        m = float(self.sigmas.max())
        return m if self.timestep_spacing in ("linspace", "trailing") else math.sqrt(m * m + 1.0)

    def set_timesteps(self, num_inference_steps, device=None):
        T, n = self.T, num_inference_steps
        self.num_inference_steps = n
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float64) + self.steps_offset
        elif self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n)[::-1].copy()
        elif self.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / n)) - 1
        else:
            raise ValueError(self.timestep_spacing)
        ts = ts.astype(np.float32)
        sig = np.interp(ts, np.arange(0, len(self._train_sigmas)), self._train_sigmas)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = torch.from_numpy(ts)

    def _index(self, t):
        return int((self.timesteps == float(t)).nonzero()[0])

    def scale_model_input(self, sample, t):
        sigma = float(self.sigmas[self._index(t)])
        return sample / math.sqrt(sigma * sigma + 1.0)

    def step(self, model_output, t, sample):
        i = self._index(t)
        sigma, nxt = float(self.sigmas[i]), float(self.sigmas[i + 1])
        if self.prediction_type == "epsilon":
            x0 = sample - sigma * model_output
        else:
            x0 = model_output * (-sigma / math.sqrt(sigma * sigma + 1.0)) + sample / (sigma * sigma + 1.0)
        derivative = (sample - x0) / sigma
        return sample + derivative * (nxt - sigma)

    def add_noise(self, original, noise, t):
        return original + noise * float(self.sigmas[self._index(t)])


class PNDMVRef(PNDMRef):
    """``PNDMScheduler.step_plms``; ``_get_prev_sample`` turns a v-prediction into epsilon with the sample it steps from"""

    def __init__(self, prediction_type="epsilon", **kw):
        super().__init__(**kw)
        self.prediction_type = _check(prediction_type)

    def _prev_sample(self, sample, t, prev, m):
        if self.prediction_type == "v_prediction":
            a_t = float(self.ac[t])
            m = math.sqrt(a_t) * m + math.sqrt(1.0 - a_t) * sample
        return super()._prev_sample(sample, t, prev, m)


class DPMSolverVRef(DPMSolverPP2MRef):
    """``DPMSolverMultistepScheduler.convert_model_output`` for dpmsolver++: x0 = alpha_t sample - sigma_t v"""

    def __init__(self, prediction_type="epsilon", **kw):
        super().__init__(**kw)
        self.prediction_type = _check(prediction_type)

    def step(self, model_output, t, sample):
        if self.step_index is None:
            self.step_index = int((self.timesteps == int(t)).nonzero()[0])
        i = self.step_index
        alpha_s, sigma_s = self._alpha_sigma(i)
        alpha_t, sigma_t = self._alpha_sigma(i + 1)
        if self.prediction_type == "epsilon":
            x0_pred = (sample - sigma_s * model_output) / alpha_s
        else:
            x0_pred = alpha_s * sample - sigma_s * model_output
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


# ------------------------------------------------------------------------------------------------ guidance_rescale
def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers 0.23 ``rescale_noise_cfg``: ``torch.std`` over the non-batch dimensions in the tensors' own dtype"""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


class RescaledUNet:
    """Wraps an oracle UNet so that ``oracle.loop.denoise``, unchanged, samples with guidance_rescale: it forms the guided
    prediction e, applies ``rescale_noise_cfg`` and returns cat([e', e']) -- the loop's own combine e' + g (e' - e') is then
    e' exactly (e' - e' is 0, also in fp16)."""

    def __init__(self, unet, guidance_scale, guidance_rescale):
        self.unet, self.g, self.phi = unet, guidance_scale, guidance_rescale

    def __call__(self, *a, **kw):
        u, c = self.unet(*a, **kw).sample.chunk(2)
        e = u + self.g * (c - u)
        if self.phi > 0.0:
            e = rescale_noise_cfg(e, c, self.phi)
        return SimpleNamespace(sample=torch.cat([e, e]))
