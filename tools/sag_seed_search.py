#!/usr/bin/env python
"""Choose the input seeds of tests/test_gpu_sag.py's trajectory cases without a GPU ("What the parity tests may say"):

    python tools/sag_seed_search.py CASE H W FIRST LAST [--factor 18]        # CASE: a key of test_gpu_sag.CASES, or "nine"
    python tools/sag_seed_search.py spec H W FIRST LAST --spec "dict(pipe='inpaint', steps=5, strength=0.6, freeu=(0.9, 0.2, 1.2, 1.4))"

The second form searches for an ``engine_cases.Spec`` with any of its switches -- FreeU, merged LoRAs (``loras=((11, 1.0),)``),
``text_len``, ``strength``, the scheduler, SDXL's ``null_post`` / ``time_ids``, ``time_cond`` -- at B = 1, merge 0, sag_scale 1
unless the literal says otherwise, through ``engine_cases.sag_figures`` (the figures tests/test_guidance_features_host.py asserts).

For every seed in [FIRST, LAST) the case runs through the oracle loop in fp32 and on a CPU fp16 copy of the oracle (a stand-in for
the GPU's stock fp16 arm, whose mass deviation is 2 - 4 times larger), and the seeds are printed at which between 1/8 and 7/8 of the
mask cells are set at every evaluation and min |mass - 1| is at least ``factor`` times the stand-in's largest mass deviation."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case")
    ap.add_argument("h", type=int)
    ap.add_argument("w", type=int)
    ap.add_argument("first", type=int)
    ap.add_argument("last", type=int)
    ap.add_argument("--factor", type=float, default=18.0)
    ap.add_argument("--spec", default=None, help="with CASE = spec: a dict literal of engine_cases.Spec fields")
    a = ap.parse_args()
    if a.case == "spec":
        return search_spec(a)
    import test_gpu_sag as T
    from conftest import rel_l2
    half = lambda t: t.half() if isinstance(t, torch.Tensor) and t.is_floating_point() else t
    arms = {}

    def cpu_arm(dev_str, name, nine=False):
        if (name, nine) not in arms:
            arms[name, nine] = copy.deepcopy(T.sag_models(dev_str, name, nine)[3]).half().eval()
        return arms[name, nine], half
    T.arm_unet = cpu_arm
    for seed in range(a.first, a.last):
        if a.case == "nine":            # (its latent size is fixed in the test)
            T.NINE_SEED = seed
            runs = T.nine_channel_runs("cpu")[0]
            moved, fractions, margin, dev = T.nine_channel_figures(runs)
        else:
            T.CASES[a.case] = T.CASES[a.case].but(hw=(a.h, a.w), seed=seed)
            T.sag_oracle.cache_clear()
            ref, masses, masks = T.sag_oracle(a.case, "cpu", False, T.SAG)
            _, arm_masses, _ = T.sag_oracle(a.case, "cpu", True, T.SAG)
            margin = min(float(np.abs(m - 1.0).min()) for m in masses)
            dev = max(float(np.abs(x - m).max()) for x, m in zip(arm_masses, masses))
            fractions = [float(m.mean()) for m in masks]
            moved = rel_l2(ref, T.sag_oracle(a.case, "cpu", False, 0.0)[0]) if margin >= a.factor * dev else float("nan")
        if margin >= a.factor * dev and all(1 / 8 <= x <= 7 / 8 for x in fractions):
            print(f"{a.case} hw=({a.h}, {a.w}) seed={seed}: min |mass - 1| {margin:.2e} = {margin / dev:.1f} x the stand-in's deviation "
                  f"{dev:.2e}; set {[round(x, 2) for x in fractions]}; SAG moves the oracle by {moved:.2e}", flush=True)


def search_spec(a):
    import ast
    import engine_cases as E
    node = ast.parse(a.spec.strip(), mode="eval").body
    if isinstance(node, ast.Call):      # dict(key=literal, ...)
        assert getattr(node.func, "id", None) == "dict" and not node.args
        fields = {k.arg: ast.literal_eval(k.value) for k in node.keywords}
    else:
        fields = ast.literal_eval(node)
    base = E.Spec(**{**dict(B=1, steps=3, merge=0, sag=1.0), **fields})
    for seed in range(a.first, a.last):
        spec = base.but(hw=(a.h, a.w), seed=seed)
        masses, masks, _ = E.guidance_trace(spec, "cpu")
        fractions = [float(m.mean()) for m in masks]
        margin = min(float(np.abs(m - 1.0).min()) for m in masses)
        if margin >= 0.02 and all(1 / 8 <= x <= 7 / 8 for x in fractions):     # (the stand-in's deviation is never below 2e-3)
            f = E.sag_figures(spec, "cpu")
            if f["margin"] >= a.factor * f["dev_arm"]:
                print(f"{a.spec} hw=({a.h}, {a.w}) seed={seed}: min |mass - 1| {f['margin']:.2e} = {f['margin'] / f['dev_arm']:.1f} x the "
                      f"stand-in's deviation {f['dev_arm']:.2e}; set {[round(x, 2) for x in fractions]}; SAG moves the oracle by "
                      f"{f['moved']:.2e}", flush=True)
        for fn in (E.oracle_traced, E.sag_figures, E._inputs):
            fn.cache_clear()


if __name__ == "__main__":
    main()
