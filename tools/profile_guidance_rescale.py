#!/usr/bin/env python
"""One SD1.5 512x512 batch-4 generation (the default benchmark workload: 50 DDIM steps, guidance 5, LoRA rank 128 merged,
hipGraph on) with ``guidance_rescale`` = argv[1] (default 0.7), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/profile_guidance_rescale.py 0.7

At 0 the step is cid_cfg_ddim_step_f16's kernel; above it cid_cfg_rescale_f16's and the scaled step kernel run instead
(profiles/guidance_rescale_kernel.txt holds the rows of the three)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    from consistentid_amd import pipeline, synth, unet_spec
    from consistentid_amd.unet import HipUNet
    phi = float(sys.argv[1]) if len(sys.argv) > 1 else 0.7
    dev = torch.device("cuda:0")
    cfg = unet_spec.sd15_config()
    sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
    unet = HipUNet(cfg, sd, ad, device=dev)
    del sd, ad
    inp = synth.random_inputs(cfg, 4, 512, 512, seed_latents=2024, seed_embeds=1, device=dev)
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=True)
    out = pipe(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]), latents=inp["latents"],
               num_inference_steps=50, guidance_scale=5.0, start_merge_step=30, output_type="latent",
               guidance_rescale=phi).images
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    print(f"[profile] guidance_rescale={phi}: step launch {pipe._engine.step_path}, {len(pipe._engine.captures)} capture(s), "
          f"latents std {float(out.float().std()):.4f}")


if __name__ == "__main__":
    main()
