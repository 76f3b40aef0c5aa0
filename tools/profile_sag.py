#!/usr/bin/env python
"""What self-attention guidance costs per step (the raw output is profiles/sag_cost.txt):

    python tools/profile_sag.py [--passes N] [--out FILE]     # the four kinds below, alternating in one process
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/profile_sag.py --passes 1      # the three new kernels, a run of its own

Builds the benchmark's SD1.5 engine -- 512 x 512 batch 4, synthetic weights, LoRA rank 128 merged, hipGraph on -- and times whole
50-step generations between synchronisations:
  * DDIM, guidance_scale 5, SAG off: UNet(2B = 8 rows) + cid_cfg_ddim_step_f16, the step this engine always ran;
  * DDIM, guidance_scale 5, sag_scale 0.75: UNet(8 rows) + cid_attn_colmass_f16 + cid_sag_degrade_f16 + UNet(4 rows) +
    cid_cfg_sag_ddim_step_f16;
  * LCMScheduler, guidance_scale 1, SAG off: UNet(B = 4 rows) + cid_multistep_step_f16, the single pass;
  * LCMScheduler, guidance_scale 1, sag_scale 0.75: UNet(4 rows) + mass + degrade + UNet(4 rows) + cid_sag_multistep_step_f16.
Every timed generation follows an untimed one of the same kind (the scale is part of the graph key).  With SAG off every launch
is the parent commit's: tools/profile_pag.py --off-vs DIR times that step against another tree."""
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
    cfg, side, B, steps, merge = unet_spec.sd15_config(), 512, 4, 50, 30
    sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
    unet = HipUNet(cfg, sd, ad, device=dev)
    torch.cuda.empty_cache()
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=True)
    inp = synth.random_inputs(cfg, B, side, side, seed_latents=2024, seed_embeds=1, device=dev)
    embeds = torch.cat([inp["null"], inp["augmented"], inp["text"]])
    noise = torch.randn(steps - 1, *inp["latents"].shape, generator=torch.Generator(dev).manual_seed(7), device=dev, dtype=torch.float16)
    ddim, lcm = scheduler.DDIMScheduler(), scheduler.LCMScheduler()
    kinds = {"ddim, guidance 5, SAG off (UNet 2B + cfg_ddim)": (ddim, 5.0, 0.0),
             "ddim, guidance 5, sag_scale 0.75 (UNet 2B + mass + degrade + UNet B + cfg_ddim+sag)": (ddim, 5.0, 0.75),
             "lcm, guidance 1, SAG off (UNet B + multistep, the single pass)": (lcm, 1.0, 0.0),
             "lcm, guidance 1, sag_scale 0.75 (UNet B + mass + degrade + UNet B + multistep+sag)": (lcm, 1.0, 0.75)}
    paths, rows = {}, {}

    def generation(name):
        sch, g, sag = kinds[name]
        pipe.scheduler = sch
        kw = dict(variance_noise=noise) if sch is lcm else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(prompt_embeds=embeds, latents=inp["latents"], num_inference_steps=steps, guidance_scale=g,
                   start_merge_step=merge, output_type="latent", sag_scale=sag, **kw).images
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out.float()).all()
        paths[name], rows[name] = pipe._engine.step_path, pipe._engine._static["kvrow"].numel()
        return dt

    ms = {name: [] for name in kinds}
    for p in range(a.passes):
        for name in kinds:
            generation(name)                                # untimed: captures or re-captures the step graph
            ms[name].append(generation(name) * 1e3)
    lines = [f"{torch.cuda.get_device_name(0)}; SD1.5 {side} x {side}, batch {B}, 77 + 4 context rows, {steps} steps, hipGraph on; "
             f"{a.passes} passes, kinds alternating, one process"]
    names = list(kinds)
    best = {name: min(ms[name]) / steps for name in names}
    for name, base in zip(names, (names[0], names[0], names[2], names[2])):
        lines.append(f"{name}: step_path {paths[name]}, {rows[name]} UNet rows; ms per generation {' '.join(f'{x:.2f}' for x in ms[name])}; "
                     f"best pass ms_per_step {best[name]:.3f} ({best[name] / best[base]:.3f} x the same sampler with SAG off)")
    report = "\n".join(lines)
    print(report, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
