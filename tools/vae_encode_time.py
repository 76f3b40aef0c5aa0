#!/usr/bin/env python3
"""Time the inpaint pre-loop's VAE encode: the init image and the masked image of one request, both through the SD VAE
encoder (synthetic weights), at 512 x 512 and at 768 x 512 (the ControlNet demo's size).

    python tools/vae_encode_time.py [--iters 20] [--warmup 5] [--once]

HIP: HipVAEEncoder.encode_inpaint (one pass, the two images as one batch of 2, posterior samples drawn on the host).
Stock: the oracle's AutoencoderKL.encoder + quant_conv copied to fp16 on the GPU (conftest.half_arm), on the
pre-processed batch of 2 -- what the reference's fp16 pipeline runs with stock PyTorch-ROCm kernels.  FLOPs are counted
from the layer shapes (2 per multiply-add: convolutions, linears and the mid block's two attention products).
--once: a single HIP encode per size and no stock arm (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def encoder_flops(oracle, x) -> float:
    """multiply-adds x 2 of encoder + quant_conv on x, from the shapes seen by forward hooks"""
    total = [0.0]

    def conv_hook(m, inp, out):
        k = m.kernel_size[0] * m.kernel_size[1]
        total[0] += 2.0 * out.numel() * m.in_channels * k

    def lin_hook(m, inp, out):
        total[0] += 2.0 * out.numel() * m.in_features

    def attn_hook(m, inp, out):
        b, c, h, w = inp[0].shape
        total[0] += 2 * 2.0 * b * (h * w) ** 2 * c          # Q K^T and P V

    from oracle.vae import AttnBlock
    hs = []
    for mod in list(oracle.encoder.modules()) + [oracle.quant_conv]:
        if isinstance(mod, torch.nn.Conv2d):
            hs.append(mod.register_forward_hook(conv_hook))
        elif isinstance(mod, torch.nn.Linear):
            hs.append(mod.register_forward_hook(lin_hook))
        elif isinstance(mod, AttnBlock):
            hs.append(mod.register_forward_hook(attn_hook))
    with torch.no_grad():
        oracle.quant_conv(oracle.encoder(x))
    for h in hs:
        h.remove()
    return total[0]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    from consistentid_amd import synth, vae_spec
    from consistentid_amd.vae import HipVAEEncoder
    from conftest import half_arm
    from oracle import vae as ovae
    dev = torch.device("cuda:0")
    cfg = vae_spec.sd_vae_config()
    sd = synth.random_vae_state_dict(cfg, seed=5)
    enc = HipVAEEncoder(cfg, sd, device=dev)
    oracle = ovae.AutoencoderKL(ovae.sd_vae_config())
    oracle.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    arm = None if args.once else half_arm(oracle.eval(), dev)
    print(f"# {torch.cuda.get_device_name(0)}; SD VAE encoder, image + masked image (batch 2), synthetic weights")
    for H, W in ((512, 512), (768, 512)):
        g = torch.Generator().manual_seed(H)
        image = torch.rand(1, 3, H, W, generator=g).to(dev)
        mask = torch.zeros(1, 1, H, W, device=dev)
        mask[:, :, H // 4: 3 * H // 4, W // 4: 3 * W // 4] = 1.0
        eps = [torch.randn(1, 4, H // 8, W // 8, generator=g, dtype=torch.float16).to(dev) for _ in range(2)]
        hip = lambda: enc.encode_inpaint(image, mask, eps_image=eps[0], eps_masked=eps[1])
        if args.once:
            hip()
            torch.cuda.synchronize()
            print(f"{H}x{W}: one encode done")
            continue
        x = torch.cat([image * 2 - 1, (image * 2 - 1) * (mask < 0.5)]).half()

        def stock():
            with torch.no_grad():
                m = arm.quant_conv(arm.encoder(x))
                mean, logvar = m.chunk(2, dim=1)
                return cfg.scaling_factor * (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * torch.cat(eps))

        flops = encoder_flops(arm, x)
        t_hip, t_hip_min = timed(hip, args.iters, args.warmup)
        t_arm, t_arm_min = timed(stock, args.iters, args.warmup)
        rec = {"size": f"{H}x{W}", "batch": 2, "tflop": round(flops / 1e12, 3),
               "hip_ms": round(t_hip, 3), "hip_ms_min": round(t_hip_min, 3), "hip_tflops": round(flops / t_hip / 1e9, 1),
               "torch_fp16_ms": round(t_arm, 3), "torch_fp16_ms_min": round(t_arm_min, 3),
               "torch_fp16_tflops": round(flops / t_arm / 1e9, 1), "speedup": round(t_arm / t_hip, 3)}
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
