#!/usr/bin/env python
"""Coefficients of csrc/common.h::gelu_erf_f:  erfc(t / sqrt 2) ~= 2^(-t (c1 + t (c2 + ... + t c6)))  for t >= 0, fitted by
iteratively re-weighted least squares towards the minimax error of erf, then checked in emulated fp32 in the form the kernel
evaluates (gelu(g) = max(g, 0) - |g| / 2 * 2^P(min(|g|, 16))) over [-12, 12], every finite fp16 value and a log-spaced fp32
sweep up to 3e38.  Prints the coefficients and the errors quoted in the kernel comment.
CPU only (numpy / scipy)."""
import numpy as np
from scipy.optimize import least_squares
from scipy.special import erf

DEG = 6
t = np.linspace(0, 8, 40001)
target = erf(t / np.sqrt(2))


def model(c, t):
    p = np.zeros_like(t)
    for ck in c[::-1]:
        p = (p + ck) * t
    return 1 - np.exp2(-np.minimum(p, 200.0))


c = np.zeros(DEG)
c[0], c[1] = 1.151, 0.46
w = np.ones_like(t)
for _ in range(60):
    c = least_squares(lambda c: w * (model(c, t) - target), c, method="lm", xtol=1e-15, ftol=1e-15).x
    e = np.abs(model(c, t) - target)
    w = w * (1 + 2 * e / e.max())
    w /= w.mean()
c32 = (-c).astype(np.float32)
print("P(t) = t * (c1 + t * (c2 + ...)), coefficients (negated: erfc = 2^P):")
print("  " + ", ".join("%.9ef" % v for v in c32))
print("max |erf error| (float64 evaluation):", np.abs(model(c, t) - target).max())
CLAMP = np.float32(16.0)          # common.h: P turns upward near t = 21, so its argument is clamped (2^P(16) is an exact 0)
fin = np.arange(65536, dtype=np.uint16).view(np.float16)
fin = fin[np.isfinite(fin)].astype(np.float32)                       # every finite fp16 value
sweep = np.geomspace(1e-30, 3e38, 200001)
g = np.concatenate([np.linspace(-12, 12, 2000001), np.random.default_rng(0).standard_normal(1000000) * 3,
                    fin, sweep, -sweep]).astype(np.float32)         # + a log-spaced fp32 sweep up to 3e38, both signs


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64"""
    return (a.astype(np.float64) * b + c).astype(np.float32)


a = np.abs(g)
ac = np.minimum(a, CLAMP)
q = fma32(ac, c32[DEG - 1], c32[DEG - 2])
for k in range(DEG - 3, -1, -1):
    q = fma32(ac, q, c32[k])
e = np.exp2((ac * q).astype(np.float32)).astype(np.float32)
r = fma32((np.float32(-0.5) * a).astype(np.float32), e, np.maximum(g, np.float32(0)))
ref = 0.5 * g.astype(np.float64) * (1 + erf(g.astype(np.float64) / np.sqrt(2)))
print("all finite in emulated fp32:", bool(np.isfinite(r).all()))
print("max |gelu error| in emulated fp32, |g| <= 12:", np.abs(r - ref)[a <= 12].max())
print("max |gelu error| / max(1, |gelu|) over every finite fp16 value and the fp32 sweep:",
      (np.abs(r - ref) / np.maximum(1, np.abs(ref))).max())
