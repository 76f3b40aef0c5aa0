#!/usr/bin/env python
"""What FreeU costs, and that the default path did not move (the raw output is profiles/freeu_cost.txt):

    python tools/profile_freeu.py                   # us per denoise step with FreeU on against off, in one process
    python tools/profile_freeu.py --bench-vs DIR    # bench.py's headline, this tree against the tree in DIR, alternating

The first form builds the benchmark's two engines -- SD1.5 512 x 512 batch 4 (CFG batch 8, 50 DDIM steps) and SDXL
1024 x 1024 batch 2 (CFG batch 4, 30 steps), synthetic weights, LoRA rank 128 merged, hipGraph on -- and times whole
generations between synchronisations, off and on alternating.  A switch re-captures the step graph (the four scalars are
launch arguments), so every timed generation follows an untimed one in the same state.  The second form starts one bench.py
process per pass, FreeU off in both trees (it is off by default), the other tree first: DIR is a checkout of the parent
commit with its library built."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FREEU = {"sd15": (0.9, 0.2, 1.2, 1.4), "sdxl": (0.6, 0.4, 1.1, 1.2)}       # the values diffusers' documentation suggests
BENCH = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-torch-baseline", "--no-roofline",
         "--no-secondary"]


def step_cost(family: str, passes: int):
    import torch
    from consistentid_amd import pipeline, synth, unet_spec
    from consistentid_amd.unet import HipUNet
    dev = torch.device("cuda:0")
    if family == "sd15":
        cfg, side, B, steps, g, merge, cls = unet_spec.sd15_config(), 512, 4, 50, 5.0, 30, pipeline.ConsistentIDStableDiffusionPipeline
    else:
        cfg, side, B, steps, g, merge, cls = unet_spec.sdxl_config(), 1024, 2, 30, 7.5, 18, pipeline.ConsistentIDStableDiffusionXLPipeline
    sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
    unet = HipUNet(cfg, sd, ad, device=dev)
    del sd, ad
    torch.cuda.empty_cache()
    inp = synth.random_inputs(cfg, B, side, side, seed_latents=2024, seed_embeds=1, device=dev)
    kw = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]), latents=inp["latents"],
              num_inference_steps=steps, guidance_scale=g, start_merge_step=merge, output_type="latent")
    if family == "sdxl":
        kw.update(pooled_prompt_embeds=inp["pooled_augmented"], pooled_prompt_embeds_text_only=inp["pooled_text"],
                  negative_pooled_prompt_embeds=inp["pooled_null"], add_time_ids=inp["time_ids"])
    pipe = cls(unet, use_graph=True)

    def generation():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(**kw).images
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out.float()).all()
        return dt

    ms = {"off": [], "on": []}
    for p in range(passes):
        for state in ("off", "on"):
            pipe.enable_freeu(*FREEU[family]) if state == "on" else pipe.disable_freeu()
            generation()                                    # untimed: re-captures the step graph
            ms[state].append(generation() * 1e3)
    off, on = min(ms["off"]), min(ms["on"])
    fmt = lambda v: " ".join(f"{x:.2f}" for x in v)
    print(f"{family} {side} x {side}, batch {B} (CFG batch {2 * B}), {steps} DDIM steps, hipGraph on; FreeU {FREEU[family]}")
    print(f"  ms per generation, FreeU off: {fmt(ms['off'])}")
    print(f"  ms per generation, FreeU on:  {fmt(ms['on'])}")
    print(f"  us per step (best pass): off {off / steps * 1e3:.1f}, on {on / steps * 1e3:.1f}, FreeU costs "
          f"{(on - off) / steps * 1e3:.1f} us per step ({(on / off - 1) * 100:+.2f} %): six cid_freeu_f16 calls, twelve launches", flush=True)
    del pipe, unet
    torch.cuda.empty_cache()


def bench_vs(other: str, passes: int):
    import json
    vals = {"other": [], "this": []}
    for p in range(passes):
        for name, cwd in (("other", other), ("this", ROOT)):
            r = subprocess.run([sys.executable, *BENCH], cwd=cwd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"bench.py failed in {cwd} (exit {r.returncode}):\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            vals[name].append(json.loads(line)["value"])
            print(f"## {name} tree, pass {p + 1}\n{line}", flush=True)
    print(f"# images/s, FreeU off: other tree {vals['other']}, this tree {vals['this']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench-vs", metavar="DIR", default=None)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.bench_vs:
        print(f"# python {' '.join(BENCH)}: one process per pass, the other tree first")
        bench_vs(os.path.abspath(a.bench_vs), a.passes)
    else:
        for family in ("sd15", "sdxl"):
            step_cost(family, a.passes)


if __name__ == "__main__":
    main()
