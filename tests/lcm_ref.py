"""Test-side restatement of multistep latent consistency sampling (Luo et al. 2023, "Latent Consistency Models",
Algorithm 3; diffusers 0.23 defaults) as a STATEFUL step-by-step scheduler in float64, and of the guidance-scale embedding a
UNet with ``time_cond_proj_dim`` is conditioned on.  PARITY UNPINNED, like tests/multistep_ref.py (diffusers is not
vendored).  Written from the algorithm: nothing here knows the product's coefficient rows.

``LCMRef.step(model_output, i, sample, z)`` is the update at schedule entry i; ``LCMLoopRef`` puts oracle/ddim.py's interface
in front of it -- ``step(eps, t, sample)`` with the pre-drawn noise tensors taken in call order, as
``multistep_ref.DDIMEtaRef`` does -- so that ``oracle.loop.denoise`` drives it unchanged."""
from __future__ import annotations

import math

import numpy as np
import torch

from multistep_ref import alphas_cumprod_table


def guidance_scale_embedding(w: float, dim: int) -> np.ndarray:
    """float64 [dim]: sin then cos of 1000 w f_j, f_j = 10000 ** (-j / (dim / 2 - 1)), j < dim / 2"""
    half = dim // 2
    out = np.zeros(dim)
    for j in range(half):
        arg = 1000.0 * w * 10000.0 ** (-j / (half - 1))
        out[j], out[half + j] = math.sin(arg), math.cos(arg)
    return out


class LCMRef:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50,
                 timestep_scaling=10.0, sigma_data=0.5, prediction_type="epsilon"):
        self.T, self.original, self.scaling, self.sigma_data = num_train_timesteps, original_inference_steps, timestep_scaling, sigma_data
        self.prediction_type = prediction_type
        self.ac = alphas_cumprod_table(beta_start, beta_end, num_train_timesteps).astype(np.float64)
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        n = num_inference_steps
        if not 1 <= n <= self.original:
            raise ValueError(n)
        k = self.T // self.original
        distilled = [j * k - 1 for j in range(1, self.original + 1)]        # the timesteps the model was distilled on
        stride = len(distilled) // n
        picked = list(reversed(distilled))[::stride][:n]
        self.timesteps = torch.tensor(picked, dtype=torch.int64)

    def scale_model_input(self, sample, t=None):
        return sample

    def add_noise(self, original, noise, t):
        a = float(self.ac[int(t)])
        return math.sqrt(a) * original + math.sqrt(1.0 - a) * noise

    def step(self, model_output, i, sample, z=None):
        """one consistency step at schedule entry ``i`` (timestep ``timesteps[i]``); ``z``: the standard normal tensor the
        sample is noised with again -- every entry but the last one needs it, the last one ignores it"""
        t = int(self.timesteps[i])
        a_t = float(self.ac[t])
        if self.prediction_type == "epsilon":
            x0 = (sample - math.sqrt(1.0 - a_t) * model_output) / math.sqrt(a_t)
        else:
            x0 = math.sqrt(a_t) * sample - math.sqrt(1.0 - a_t) * model_output
        s = self.scaling * t
        c_skip = self.sigma_data ** 2 / (s ** 2 + self.sigma_data ** 2)
        c_out = s / math.sqrt(s ** 2 + self.sigma_data ** 2)
        denoised = c_out * x0 + c_skip * sample
        if i == len(self.timesteps) - 1:
            return denoised                     # the final latents carry no noise
        a_next = float(self.ac[int(self.timesteps[i + 1])])
        return math.sqrt(a_next) * denoised + math.sqrt(1.0 - a_next) * z


class LCMLoopRef(LCMRef):
    """``LCMRef`` behind oracle/ddim.py's ``step(eps, t, sample)``, so that ``oracle.loop.denoise`` drives it: the entry is
    found from ``t`` and the noise tensors are taken from ``noises`` in call order (``multistep_ref.DDIMEtaRef``'s way)"""

    def __init__(self, noises=(), **kw):
        super().__init__(**kw)
        self.noises = list(noises)

    def set_timesteps(self, num_inference_steps, device=None):
        super().set_timesteps(num_inference_steps)
        self.calls = 0

    def step(self, model_output, t, sample):
        i = [int(v) for v in self.timesteps].index(int(t))
        z = None
        if i < len(self.timesteps) - 1:
            z = self.noises[self.calls].to(device=sample.device, dtype=sample.dtype)
            self.calls += 1
        return super().step(model_output, i, sample, z)


class CondOnly:
    """The oracle UNet on the conditional rows only, behind ``oracle.loop.denoise``'s 2B-row call: the second half of every
    batched argument goes through the UNet once and comes back as both halves, so the loop's u + g (c - u) is exactly c."""

    def __init__(self, unet):
        self.unet = unet

    def __call__(self, sample, t, encoder_hidden_states, cross_attention_kwargs=None, added_cond_kwargs=None,
                 down_block_additional_residuals=None, mid_block_additional_residual=None):
        from oracle.unet import UNetOutput
        B = sample.shape[0] // 2
        kw = {}
        if added_cond_kwargs is not None:
            kw["added_cond_kwargs"] = {k: v[B:] for k, v in added_cond_kwargs.items()}
        if down_block_additional_residuals is not None:
            kw["down_block_additional_residuals"] = [d[B:] for d in down_block_additional_residuals]
            kw["mid_block_additional_residual"] = mid_block_additional_residual[B:]
        out = self.unet(sample[B:], t, encoder_hidden_states=encoder_hidden_states[B:],
                        cross_attention_kwargs=cross_attention_kwargs, **kw).sample
        return UNetOutput(sample=torch.cat([out, out]))
