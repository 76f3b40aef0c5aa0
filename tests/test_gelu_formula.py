"""The erf GELU of every HIP kernel (csrc/common.h::gelu_erf_f) evaluated on the CPU in the kernel's own fp32 order over the
whole input range: every finite fp16 value and a log-spaced fp32 sweep up to 3e38, against fp64 F.gelu.  The six polynomial
coefficients and the clamp constant are read out of common.h, so this checks the code that ships.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import torch

COMMON_H = Path(__file__).resolve().parents[1] / "consistentid_amd" / "csrc" / "common.h"
FLT = r"([-+]?\d+\.\d*(?:e[-+]?\d+)?)f"


def _product_gelu_source() -> str:
    """the body of gelu_erf_f in the product build (the #else branch; the CID_GELU_AS7126 form is an experiment)"""
    src = COMMON_H.read_text()
    start = src.index("#ifdef CID_GELU_AS7126")
    branch = src[src.index("#else", start):src.index("#endif", start)]
    body = branch[branch.index("CID_DEVINL float gelu_erf_f"):]
    return body[:body.index("\n}") + 2]


def _kernel_constants():
    body = _product_gelu_source()
    clamp = re.findall(r"__builtin_fminf\(t, " + FLT + r"\)", body)
    assert len(clamp) <= 1, body
    coef = re.findall(r"__builtin_fmaf\(tc?, (?:q|" + FLT + r"), " + FLT + r"\)", body)
    # the first FMA carries two coefficients (leading, next); the others one each
    flat = [float(v) for pair in coef for v in pair if v]
    assert len(flat) == 6, f"expected six coefficients in gelu_erf_f, found {flat}"
    return np.array(flat, np.float32), (np.float32(clamp[0]) if clamp else None)


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64, the sum is rounded once more"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32) + np.asarray(c, np.float32)).astype(np.float32)


def gelu_kernel_f32(g: np.ndarray) -> np.ndarray:
    coef, clamp = _kernel_constants()
    g = g.astype(np.float32)
    t = np.abs(g)
    tc = t if clamp is None else np.minimum(t, clamp)
    with np.errstate(over="ignore", invalid="ignore"):
        q = _fma32(tc, coef[0], coef[1])
        for c in coef[2:]:
            q = _fma32(tc, q, c)
        e = np.exp2((tc * q).astype(np.float32)).astype(np.float32)
        return _fma32((np.float32(-0.5) * t).astype(np.float32), e, np.maximum(g, np.float32(0)))


def _inputs():
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    fp16 = h[np.isfinite(h)].astype(np.float32)
    assert fp16.size == 63488
    sweep = np.geomspace(1e-30, 3e38, 100001).astype(np.float32)
    return np.concatenate([fp16, sweep, -sweep])


def test_constants_are_the_fitted_polynomial():
    coef, clamp = _kernel_constants()
    # erfc(t / sqrt 2) = 2^P(t) with P(t) = -t (1.1511 + 0.4591 t + ...) near 0: 2^P(0) = 1 and P'(0) = -sqrt(2 / pi) / ln 2
    assert abs(float(coef[-1]) + np.sqrt(2 / np.pi) / np.log(2)) < 5e-3
    assert clamp is not None, "gelu_erf_f must clamp the polynomial argument (P turns upward near |g| = 21)"


def test_gelu_formula_over_the_whole_range():
    g = _inputs()
    got = gelu_kernel_f32(g).astype(np.float64)
    ref = torch.nn.functional.gelu(torch.from_numpy(g.astype(np.float64))).numpy()
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    bad = ~np.isfinite(got) | ~(err <= 2e-6)
    if bad.any():
        ab = np.abs(g[bad])
        msg = (f"{int(bad.sum())} of {g.size} inputs wrong, |g| from {ab.min():.6g} to {ab.max():.6g}; "
              f"e.g. gelu({g[bad][0]:.6g}) = {got[bad][0]:.6g}, want {ref[bad][0]:.6g}")
        raise AssertionError(msg)
    print(f"[gelu formula] {g.size} inputs, max err / max(1, |ref|) = {err.max():.3e}")
    assert err.max() <= 2e-6
