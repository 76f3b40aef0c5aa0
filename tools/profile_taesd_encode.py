#!/usr/bin/env python
"""What AutoencoderTiny ENCODING costs (the raw output is profiles/taesd_encode_cost.txt):

    python tools/profile_taesd_encode.py [--out FILE] [--sections 123] [--parent DIR]

The method of tools/profile_taesd.py: synthetic weights, one process, device events around back-to-back launches, variants
alternating over rounds, median and (min .. max) reported.  Every step runs under its own time limit (a watchdog ends the
process) and the first failure ends the run.
  1. the stride-2 convolution: cid_tiny_conv64_s2_f16 against cid_gemm_f16 configured for the same convolution (c1 = 64, N = 64,
     taps = 9, stride = 2, pad_mode = 0) -- the path the library had before -- at the encoder's three levels for 512 x 512
     images (256^2, 128^2, 64^2 outputs), B = 8 (four image + masked-image pairs) and B = 2; the outputs of the two are
     compared at every shape before anything is timed;
  2. a whole encode_inpaint: HipAutoencoderTinyEncoder against HipVAEEncoder (SD VAE) for one and for four 512 x 512 image +
     masked-image pairs;
  3. the pre-loop's share of a few-step inpaint generation: the 4-step single-pass LCM generation (SD1.5 512 x 512, batch 4, a
     9-channel UNet at strength 0.8 of 5 steps, so that both images are encoded) from pre-computed latents (the loop alone),
     and from image= / mask_image= with each encoder; the tiny decoder decodes in all three;
  4. with --parent DIR (a built checkout of the parent commit): bench.py's default line, DIR against this tree, alternating,
     one child process per run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StepLimit:
    """a time limit for one step of the run: past it the process ends with status 124 (a hung launch cannot be interrupted
    from Python, so nothing else is started on the GPU after it)"""

    def __init__(self, seconds, what):
        self.timer = threading.Timer(seconds, self._expired)
        self.timer.daemon = True
        self.what, self.seconds = what, seconds

    def _expired(self):
        print(f"step '{self.what}' exceeded its limit of {self.seconds} s", flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def load_test_module(name):
    import importlib.util
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    spec = importlib.util.spec_from_file_location(name, os.path.join(tests, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def bench_lines(a, say):
    """4. bench.py's default line, the parent commit's tree against this tree: one child process per run, alternating"""
    if "4" not in a.sections or not a.parent:
        return
    say(f"\n4. bench.py --gpus 1 --steps 3 --warmup 1, the parent commit's tree against this tree, alternating, one child process "
        f"per run, {a.bench_runs} runs each: images/s (ms per generation)")
    res = {"parent": [], "this tree": []}
    for _ in range(a.bench_runs):
        for name, root in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"], cwd=root,
                               capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                say(f"  {name}: bench.py ended with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                sys.exit(r.returncode)
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append((rec["value"], rec["ms_per_step"]))
            say(f"  {name:10s} {rec['value']:.4f} images/s ({rec['ms_per_step']:.2f} ms)")
    for name, v in res.items():
        vals = [x[0] for x in v]
        say(f"  {name:10s} median {statistics.median(vals):.4f} images/s, range {min(vals):.4f} .. {max(vals):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--sections", default="1234", help="the measurements to run (3 builds the SD1.5 UNet; 4 needs --parent)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for measurement 4")
    ap.add_argument("--bench-runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    from consistentid_amd import ops, synth, vae_spec
    from consistentid_amd.vae import HipVAEEncoder
    from consistentid_amd.vae_tiny import HipAutoencoderTiny, HipAutoencoderTinyEncoder
    dev = torch.device("cuda:0")
    lines = [f"{torch.cuda.get_device_name(0)}; synthetic weights; device events around back-to-back launches, variants "
             f"alternating over {a.rounds} rounds in one process; median (min .. max) per call"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

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

    fmt = lambda v, s=1.0: f"{statistics.median(v) * s:9.2f} ({min(v) * s:9.2f} .. {max(v) * s:9.2f})"
    g = torch.Generator(dev).manual_seed(0)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=dev) * scale).half()

    # ------------------------------------------------------------------ 1. the stride-2 convolution
    shapes = [(B, side) for B in (8, 2) for side in (256, 128, 64)] if "1" in a.sections else []
    if shapes:
        say("\n1. stride-2 convolution, 64 -> 64 channels, no bias, us per launch: cid_tiny_conv64_s2_f16 | cid_gemm_f16 (the "
            "parent's path: taps 9, stride 2, pad_mode 0) | ratio of medians (gemm / tiny); then the tiny kernel's bytes-needed "
            "rate (input + output once)")
    w = rnd(64, 9, 64, scale=(2 / 576) ** 0.5)
    for B, side in shapes:
        with StepLimit(120, f"stride-2 convolution B={B} {side}^2"):
            Hi = 2 * side
            x = rnd(B, Hi * Hi, 64)
            out_t = torch.empty(B, side * side, 64, dtype=torch.float16, device=dev)
            out_g = torch.empty_like(out_t)

            def tiny():
                ops.tiny_conv64_s2(x, out_t, w, B=B, H=Hi, W=Hi)

            def gemm():
                ops.gemm(x.view(-1, 64), w.view(64, 576), out_g.view(-1, 64), M=B * side * side, N=64, c1=64, taps=9,
                         Hi=Hi, Wi=Hi, Ho=side, Wo=side, stride=2, pad_mode=0)

            tiny(), gemm()
            torch.cuda.synchronize()
            diff = float((out_t.float() - out_g.float()).abs().max())
            assert diff <= 2.0 ** -9 * float(out_g.float().abs().max()) + 1e-3, (B, side, diff)
            iters = max(20, min(400, int(2e8 / (B * side * side * 64))))
            t = alternate({"tiny": tiny, "gemm": gemm}, iters)
            nbytes = 2 * 64 * B * (Hi * Hi + side * side)
            say(f"  B = {B}  {Hi:4d}^2 -> {side:3d}^2  {fmt(t['tiny'])} | {fmt(t['gemm'])} | "
                f"{statistics.median(t['gemm']) / statistics.median(t['tiny']):5.2f} x | "
                f"{nbytes / statistics.median(t['tiny']) * 1e-6:6.2f} TB/s   (max |tiny - gemm| {diff:.2e})")
            del x, out_t, out_g

    # ------------------------------------------------------------------ 2. a whole encode_inpaint
    if not set("23") & set(a.sections):
        return bench_lines(a, say)
    E = load_test_module("taesd_enc_ref")
    R = sys.modules["taesd_ref"]
    tiny_enc = HipAutoencoderTinyEncoder(E.config(), E.synthetic(0).state_dict(), device=dev)
    tiny_dec = HipAutoencoderTiny(R.config(), R.synthetic(0).state_dict(), device=dev)
    kcfg = vae_spec.sd_vae_config()
    kl_enc = HipVAEEncoder(kcfg, synth.random_vae_state_dict(kcfg, seed=5, device=dev), device=dev)
    if "2" in a.sections:
        say("\n2. a whole encode_inpaint (image + masked image in one pass -> image_latents, masked_image_latents, mask_latents), "
            "512 x 512, ms per call")
    for pairs in (1, 4) if "2" in a.sections else ():
        with StepLimit(180, f"encode_inpaint, {pairs} pair(s)"):
            image = torch.rand(pairs, 3, 512, 512, generator=g, device=dev)
            mask = torch.zeros(pairs, 1, 512, 512, device=dev)
            mask[:, :, 128:384, 128:384] = 1.0
            eps = [rnd(pairs, 4, 64, 64) for _ in range(2)]
            t = alternate({"tiny": lambda: tiny_enc.encode_inpaint(image, mask),
                           "kl": lambda: kl_enc.encode_inpaint(image, mask, eps_image=eps[0], eps_masked=eps[1])}, 5)
            say(f"  {pairs} pair(s): HipAutoencoderTinyEncoder {fmt(t['tiny'], 1e-3)} | HipVAEEncoder {fmt(t['kl'], 1e-3)} | "
                f"{statistics.median(t['kl']) / statistics.median(t['tiny']):6.1f} x")

    # ------------------------------------------------------------------ 3. the pre-loop's share
    if "3" in a.sections:
        import dataclasses
        from consistentid_amd import pipeline, scheduler, unet_spec
        from consistentid_amd.unet import HipUNet
        with StepLimit(400, "building the 9-channel SD1.5 UNet"):
            cfg = dataclasses.replace(unet_spec.sd15_config(), in_channels=9)
            sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
            ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
            unet = HipUNet(cfg, sd, ad, device=dev)
            del sd, ad
            torch.cuda.empty_cache()
        B, side, steps, strength = 4, 512, 5, 0.8
        pipe = pipeline.StableDiffusionInpaintConsistentIDPipeline(unet, use_graph=True, scheduler=scheduler.LCMScheduler(),
                                                                   vae=tiny_dec, vae_encoder=tiny_enc)
        inp = synth.random_inputs(unet_spec.sd15_config(), B, side, side, seed_latents=2024, seed_embeds=1, device=dev)
        embeds = torch.cat([inp["null"], inp["augmented"], inp["text"]])
        image = torch.rand(B, 3, side, side, generator=g, device=dev)
        mask = torch.zeros(B, 1, side, side, device=dev)
        mask[:, :, 128:384, 128:384] = 1.0
        pre = tiny_enc.encode_inpaint(image, mask)
        noise = rnd(B, 4, side // 8, side // 8)
        kw = dict(prompt_embeds=embeds, num_inference_steps=steps, strength=strength, guidance_scale=1.0, start_merge_step=1,
                  output_type="pt")

        def generation(encoder):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gen = torch.Generator().manual_seed(3)
            if encoder is None:
                out = pipe(image_latents=pre["image_latents"], noise=noise, mask_latents=pre["mask_latents"],
                           masked_image_latents=pre["masked_image_latents"], generator=gen, **kw).images
            else:
                pipe.vae_encoder = encoder
                out = pipe(image=image, mask_image=mask, generator=gen, **kw).images
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert torch.isfinite(out.float()).all()
            return dt

        runs = {"loop + tiny decode, from pre-computed latents": None, "tiny encode + loop + tiny decode": tiny_enc,
                "KL encode + loop + tiny decode": kl_enc}
        ms = {k: [] for k in runs}
        with StepLimit(400, "the few-step inpaint generations"):
            for k, v in runs.items():
                generation(v)                      # untimed: captures the step graph, sizes the per-shape buffers
            for _ in range(a.rounds):
                for k, v in runs.items():
                    ms[k].append(generation(v))
        say(f"\n3. the 4-step single-pass LCM inpaint generation (SD1.5 {side} x {side}, batch {B}, 9-channel UNet, {steps} steps at "
            f"strength {strength} = 4 executed, guidance 1, hipGraph on, output_type pt), host clock between synchronisations, ms per "
            "generation; the pre-loop column is the difference to the first row (encode + the host's draws and copies)")
        base = statistics.median(ms["loop + tiny decode, from pre-computed latents"])
        for k, v in ms.items():
            say(f"  {k:48s} {fmt(v)}   pre-loop = {statistics.median(v) - base:8.2f}")
        del pipe, unet
        torch.cuda.empty_cache()

    bench_lines(a, say)


if __name__ == "__main__":
    main()
