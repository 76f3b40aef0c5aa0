#!/usr/bin/env python
"""What AutoencoderTiny decoding costs (the raw output is profiles/taesd_cost.txt):

    python tools/profile_taesd.py [--out FILE] [--skip-lcm]

Three measurements, synthetic weights, one process, device events around back-to-back launches:
  1. the body convolution: cid_tiny_conv64_f16 against cid_gemm_f16 configured for the same convolution (c1 = 64, N = 64,
     taps = 9, act = 1, res, up) -- the path the library had before -- on the net's convolution kinds at the SD1.5 512 x 512
     batch 4 shapes (64^2 .. 512^2 outputs and the three `up` convolutions), variants alternating over rounds; the outputs of
     the two are compared at every shape before anything is timed;
  2. a whole decode: HipAutoencoderTiny against HipVAEDecoder for 4 latents of 64 x 64, and against HipVAEDecoderF32 (the SDXL
     default) for 1 latent of 128 x 128, alternating;
  3. the few-step share: the 4-step single-pass LCM generation of tools/profile_lcm.py with output_type "latent" (the denoise
     loop) alone and followed by each decoder's decode_latents (the images stay on the device)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--skip-lcm", action="store_true", help="leave out measurement 3 (it builds the SD1.5 UNet)")
    a = ap.parse_args()
    import torch
    from consistentid_amd import ops, synth, vae_spec
    from consistentid_amd.vae import make_vae_decoder
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    dev = torch.device("cuda:0")
    lines = [f"{torch.cuda.get_device_name(0)}; synthetic weights; device events around back-to-back launches, variants "
             f"alternating over {a.rounds} rounds in one process; median (min) per call"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3          # microseconds per call

    def alternate(variants, iters):
        """{name: fn} -> {name: [us per call, one per round]}"""
        for fn in variants.values():
            timed(fn, 3)
        out = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                out[k].append(timed(fn, iters))
        return out

    fmt = lambda v: f"{statistics.median(v):9.1f} ({min(v):9.1f})"

    # ------------------------------------------------------------------ 1. the body convolution
    say("\n1. body convolution, B = 4, 64 -> 64 channels, us per launch: cid_tiny_conv64_f16 | cid_gemm_f16 (the parent's path) | "
        "ratio of medians (gemm / tiny); then the tiny kernel's bytes-needed rate (input + output + residual once)")
    g = torch.Generator(dev).manual_seed(0)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=dev) * scale).half()
    w = rnd(64, 9, 64, scale=(2 / 576) ** 0.5)
    bias = rnd(64, scale=0.1)
    B = 4
    kinds = [("conv + bias + relu", dict(bias=True, res=False, relu=True, up=False)),
             ("conv + bias + res + relu", dict(bias=True, res=True, relu=True, up=False)),
             ("upsample + conv", dict(bias=False, res=False, relu=False, up=True))]
    for side in (64, 128, 256, 512):
        for name, k in kinds:
            if k["up"] and side == 64:
                continue
            Hi = side // 2 if k["up"] else side
            x, out_t, out_g = rnd(B, Hi * Hi, 64), torch.empty(B, side * side, 64, dtype=torch.float16, device=dev), None
            out_g = torch.empty_like(out_t)
            res = rnd(B, side * side, 64) if k["res"] else None
            b = bias if k["bias"] else None

            def tiny():
                ops.tiny_conv64(x, out_t, w, b, B=B, H=Hi, W=Hi, res=res, relu=k["relu"], up=k["up"])

            def gemm():
                ops.gemm(x.view(-1, 64), w.view(64, 576), out_g.view(-1, 64), M=B * side * side, N=64, c1=64, bias=b,
                         res=res.view(-1, 64) if res is not None else None, ldr=64 if res is not None else None, taps=9,
                         Hi=Hi, Wi=Hi, Ho=side, Wo=side, stride=1, up=int(k["up"]), act=int(k["relu"]))

            tiny(), gemm()
            torch.cuda.synchronize()
            diff = float((out_t.float() - out_g.float()).abs().max())
            assert diff <= 2.0 ** -9 * float(out_g.float().abs().max()) + 1e-3, (name, side, diff)
            iters = max(20, min(400, int(2e8 / (B * side * side * 64))))
            t = alternate({"tiny": tiny, "gemm": gemm}, iters)
            nbytes = 2 * 64 * B * (Hi * Hi + side * side * (2 if k["res"] else 1))
            say(f"  {side:3d}^2 out  {name:26s} {fmt(t['tiny'])} | {fmt(t['gemm'])} | {statistics.median(t['gemm']) / statistics.median(t['tiny']):5.2f} x"
                f" | {nbytes / statistics.median(t['tiny']) * 1e-6:6.2f} TB/s   (max |tiny - gemm| {diff:.2e})")
            del x, out_t, out_g, res

    # ------------------------------------------------------------------ 2. a whole decode
    import importlib.util
    spec = importlib.util.spec_from_file_location("taesd_ref", os.path.join(ROOT, "tests", "taesd_ref.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    tiny_vae = HipAutoencoderTiny(R.config(), R.synthetic(0).state_dict(), device=dev)
    say("\n2. a whole decode (decode_latents: latents -> [B, 3, 8h, 8w] in [0, 1]), ms per call")
    decoders = {}
    for label, cfg, shape in (("SD1.5 HipVAEDecoder (fp16)", vae_spec.sd_vae_config(), (4, 4, 64, 64)),
                              ("SDXL HipVAEDecoderF32", vae_spec.sdxl_vae_config(), (1, 4, 128, 128))):
        kl = make_vae_decoder(cfg, synth.random_vae_state_dict(cfg, seed=5, device=dev), device=dev)
        decoders[label] = kl
        lat = rnd(*shape, scale=cfg.scaling_factor * 4)
        t = alternate({"tiny": lambda: tiny_vae.decode_latents(lat), "kl": lambda: kl.decode_latents(lat)}, 3)
        ms = lambda v: f"{statistics.median(v) * 1e-3:8.3f} ({min(v) * 1e-3:8.3f})"
        say(f"  latents {shape}: HipAutoencoderTiny {ms(t['tiny'])} | {label} {ms(t['kl'])} | "
            f"{statistics.median(t['kl']) / statistics.median(t['tiny']):6.1f} x")
        if label.startswith("SDXL"):
            del decoders[label], kl
            torch.cuda.empty_cache()

    # ------------------------------------------------------------------ 3. the few-step share
    if not a.skip_lcm:
        from consistentid_amd import pipeline, scheduler, unet_spec
        from consistentid_amd.unet import HipUNet
        cfg, side, merge = unet_spec.sd15_config(), 512, 1
        sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
        ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
        unet = HipUNet(cfg, sd, ad, device=dev)
        del sd, ad
        torch.cuda.empty_cache()
        pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=True, scheduler=scheduler.LCMScheduler())
        inp = synth.random_inputs(cfg, B, side, side, seed_latents=2024, seed_embeds=1, device=dev)
        embeds = torch.cat([inp["null"], inp["augmented"], inp["text"]])
        noise = torch.randn(3, *inp["latents"].shape, generator=torch.Generator(dev).manual_seed(7), device=dev, dtype=torch.float16)
        kl = decoders["SD1.5 HipVAEDecoder (fp16)"]

        def generation(vae):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(prompt_embeds=embeds, latents=inp["latents"], num_inference_steps=4, guidance_scale=1.0,
                       start_merge_step=merge, output_type="latent", variance_noise=noise).images
            if vae is not None:
                out = vae.decode_latents(out)              # what _postprocess_checked runs for every pixel output type
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert torch.isfinite(out.float()).all()
            return dt

        runs = {"denoise loop only (output_type latent)": None, "loop + HipAutoencoderTiny.decode_latents": tiny_vae,
                "loop + HipVAEDecoder.decode_latents": kl}
        ms = {k: [] for k in runs}
        for k, v in runs.items():
            generation(v)                      # untimed: captures the step graph, sizes the decoders' buffers
        for _ in range(a.rounds):
            for k, v in runs.items():
                ms[k].append(generation(v))
        say(f"\n3. the 4-step single-pass LCM generation (SD1.5 {side} x {side}, batch {B}, guidance 1, hipGraph on), host clock "
            "between synchronisations, ms per generation (images left on the device)")
        base = statistics.median(ms["denoise loop only (output_type latent)"])
        for k, v in ms.items():
            say(f"  {k:45s} {statistics.median(v):8.2f} ({min(v):8.2f})   decode = {statistics.median(v) - base:8.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
