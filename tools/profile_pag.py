#!/usr/bin/env python
"""What perturbed-attention guidance costs per step (the raw output is profiles/pag_cost.txt):

    python tools/profile_pag.py [--passes N] [--out FILE] [--layers IDS]   # the four kinds below, alternating in one process
    python tools/profile_pag.py --off-vs DIR [--passes N]     # the DDIM step with PAG off, this tree against the tree in DIR

Builds the benchmark's SD1.5 engine -- 512 x 512 batch 4, synthetic weights, LoRA rank 128 merged, ``keep_base=True`` (PAG folds
from the un-merged base), hipGraph on -- and times whole 50-step generations between synchronisations:
  * DDIM, guidance_scale 5, PAG off: UNet(2B = 8 rows) + cid_cfg_ddim_step_f16, the step this engine always ran;
  * DDIM, guidance_scale 5, pag_scale 3 on "mid": UNet(3B = 12 rows, the mid block's self-attention one GEMM on the last 4)
    + cid_cfg_pag_ddim_step_f16;
  * LCMScheduler, guidance_scale 1, PAG off: UNet(B = 4 rows) + cid_multistep_step_f16, the single pass;
  * LCMScheduler, guidance_scale 1, pag_scale 3 on "mid": UNet(2B = 8 rows) + cid_pag_multistep_step_f16.
``--layers down.block_0,mid`` times another selection: anything in the two upper levels has more than 2048 perturbed rows per
launch, which run LayerNorm + GEMM on the unfolded weight instead of the folded GEMM.
Every timed generation follows an untimed one of the same kind (PAG on / off has its own graph key).  ``--off-vs``: one
process per tree and pass, the other tree first, each timing the first kind with nothing but keywords both trees know."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# runs with a tree's root as the working directory (python -c puts it first on sys.path)
OFF_SNIPPET = """
import time, torch
from consistentid_amd import pipeline, synth, unet_spec
from consistentid_amd.unet import HipUNet
dev = torch.device("cuda:0")
cfg = unet_spec.sd15_config()
sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
pipe = pipeline.ConsistentIDStableDiffusionPipeline(HipUNet(cfg, sd, ad, device=dev), use_graph=True)
inp = synth.random_inputs(cfg, 4, 512, 512, seed_latents=2024, seed_embeds=1, device=dev)
kw = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]), latents=inp["latents"], num_inference_steps=50,
          guidance_scale=5.0, start_merge_step=30, output_type="latent")
ms = []
for k in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe(**kw)
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3)
print("MS", min(ms[1:]) / 50)
"""


def off_vs(other: str, passes: int):
    vals = {"other": [], "this": []}
    for p in range(passes):
        for name, cwd in (("other", other), ("this", ROOT)):
            r = subprocess.run([sys.executable, "-c", OFF_SNIPPET], cwd=cwd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"the PAG-off step failed in {cwd} (exit {r.returncode}):\n{r.stderr[-2000:]}")
            vals[name].append(float([ln for ln in r.stdout.splitlines() if ln.startswith("MS ")][-1].split()[1]))
            print(f"## {name} tree, pass {p + 1}: {vals[name][-1]:.3f} ms per DDIM step, PAG off", flush=True)
    fmt = lambda v: " ".join(f"{x:.3f}" for x in v)
    print(f"# ms per DDIM step with PAG off (SD1.5 512 x 512, batch 4, best of two timed generations per process): other tree "
          f"{fmt(vals['other'])}, this tree {fmt(vals['this'])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--off-vs", metavar="DIR", default=None)
    ap.add_argument("--layers", default="mid", help="pag_applied_layers, comma-separated (default: mid)")
    a = ap.parse_args()
    if a.off_vs:
        return off_vs(os.path.abspath(a.off_vs), a.passes)
    import torch
    from consistentid_amd import pipeline, scheduler, synth, unet_spec
    from consistentid_amd.unet import HipUNet
    dev = torch.device("cuda:0")
    cfg, side, B, steps, merge = unet_spec.sd15_config(), 512, 4, 50, 30
    sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
    unet = HipUNet(cfg, sd, ad, device=dev, keep_base=True)
    torch.cuda.empty_cache()
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=True)
    pipe.enable_pag(a.layers.split(","))
    inp = synth.random_inputs(cfg, B, side, side, seed_latents=2024, seed_embeds=1, device=dev)
    embeds = torch.cat([inp["null"], inp["augmented"], inp["text"]])
    noise = torch.randn(steps - 1, *inp["latents"].shape, generator=torch.Generator(dev).manual_seed(7), device=dev, dtype=torch.float16)
    ddim, lcm = scheduler.DDIMScheduler(), scheduler.LCMScheduler()
    kinds = {"ddim, guidance 5, PAG off (UNet 2B + cfg_ddim)": (ddim, 5.0, 0.0),
             f"ddim, guidance 5, pag_scale 3 on {a.layers} (UNet 3B + cfg_ddim+pag)": (ddim, 5.0, 3.0),
             "lcm, guidance 1, PAG off (UNet B + multistep, the single pass)": (lcm, 1.0, 0.0),
             f"lcm, guidance 1, pag_scale 3 on {a.layers} (UNet 2B + multistep+pag)": (lcm, 1.0, 3.0)}
    paths, rows = {}, {}

    def generation(name):
        sch, g, pag = kinds[name]
        pipe.scheduler = sch
        kw = dict(variance_noise=noise) if sch is lcm else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(prompt_embeds=embeds, latents=inp["latents"], num_inference_steps=steps, guidance_scale=g,
                   start_merge_step=merge, output_type="latent", pag_scale=pag, **kw).images
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
             f"PAG layers {list(unet.pag_layers)}; {a.passes} passes, kinds alternating, one process"]
    names = list(kinds)
    best = {name: min(ms[name]) / steps for name in names}
    for name, base in zip(names, (names[0], names[0], names[2], names[2])):
        lines.append(f"{name}: step_path {paths[name]}, {rows[name]} UNet rows; ms per generation {' '.join(f'{x:.2f}' for x in ms[name])}; "
                     f"best pass ms_per_step {best[name]:.3f} ({best[name] / best[base]:.3f} x the same sampler with PAG off)")
    report = "\n".join(lines)
    print(report, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
