#!/usr/bin/env python
"""What a single-pass LCM step costs against the DDIM step (the raw output is profiles/lcm_cost.txt):

    python tools/profile_lcm.py [--out FILE]

Builds the benchmark's SD1.5 engine -- 512 x 512 batch 4, synthetic weights, LoRA rank 128 merged, hipGraph on -- and times
whole generations between synchronisations, alternating in one process:
  * DDIM, 50 steps, guidance_scale 5: UNet(2B = 8 rows) + cid_cfg_ddim_step_f16, the step this engine always ran;
  * LCMScheduler, 50 steps (its longest schedule, so that both per-step figures amortise the same pre-loop), guidance_scale
    1: UNet(B = 4 rows) + cid_multistep_step_f16, the single pass;
  * LCMScheduler, 50 steps, guidance_scale 2: UNet(8 rows) + cid_cfg_multistep_step_f16;
  * LCMScheduler, 4 steps, guidance_scale 1: the generation a few-step user runs.
The LCM noise tensors are drawn before the clock starts.  A change of scheduler or step count re-captures nothing by itself,
but the single pass has its own graph key, so every timed generation follows an untimed one of the same kind."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    from consistentid_amd import pipeline, scheduler, synth, unet_spec
    from consistentid_amd.unet import HipUNet
    dev = torch.device("cuda:0")
    cfg, side, B, merge = unet_spec.sd15_config(), 512, 4, 30
    sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
    unet = HipUNet(cfg, sd, ad, device=dev)
    del sd, ad
    torch.cuda.empty_cache()
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=True)
    inp = synth.random_inputs(cfg, B, side, side, seed_latents=2024, seed_embeds=1, device=dev)
    embeds = torch.cat([inp["null"], inp["augmented"], inp["text"]])
    gen = torch.Generator(dev).manual_seed(7)
    noise = torch.randn(49, *inp["latents"].shape, generator=gen, device=dev, dtype=torch.float16)
    ddim, lcm = scheduler.DDIMScheduler(), scheduler.LCMScheduler()
    # name -> (scheduler, steps, guidance_scale, start_merge_step): the 4-step run merges after its first step, the others
    # where the benchmark does
    kinds = {"ddim 50 steps, guidance 5 (UNet 2B + cfg_ddim)": (ddim, 50, 5.0, merge),
             "lcm 50 steps, guidance 1 (UNet B + multistep, the single pass)": (lcm, 50, 1.0, merge),
             "lcm 50 steps, guidance 2 (UNet 2B + cfg_multistep)": (lcm, 50, 2.0, merge),
             "lcm 4 steps, guidance 1 (the single pass)": (lcm, 4, 1.0, 1)}
    paths = {}

    def generation(name):
        sch, steps, g, m = kinds[name]
        pipe.scheduler = sch
        kw = dict(variance_noise=noise[:steps - 1]) if sch is lcm else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(prompt_embeds=embeds, latents=inp["latents"], num_inference_steps=steps, guidance_scale=g,
                   start_merge_step=m, output_type="latent", **kw).images
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out.float()).all()
        paths[name] = pipe._engine.step_path
        return dt

    ms = {name: [] for name in kinds}
    for p in range(a.passes):
        for name in kinds:
            generation(name)                                # untimed: captures or re-captures the step graph
            ms[name].append(generation(name) * 1e3)
    lines = [f"{torch.cuda.get_device_name(0)}; SD1.5 {side} x {side}, batch {B}, 77 + 4 context rows, hipGraph on; {a.passes} passes, "
             "kinds alternating, one process"]
    names = list(kinds)
    base = min(ms[names[0]]) / kinds[names[0]][1]
    for name in names:
        steps = kinds[name][1]
        best = min(ms[name])
        lines.append(f"{name}: step_path {paths[name]}; ms per generation {' '.join(f'{x:.2f}' for x in ms[name])}; best pass "
                     f"ms_per_step {best / steps:.3f} ({best / steps / base:.3f} x the DDIM step)")
    report = "\n".join(lines)
    print(report, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
