#!/usr/bin/env python
"""What a long context costs (the raw output is profiles/long_context_cost.txt):

    python tools/profile_long_context.py [--out FILE]

Builds the benchmark's SD1.5 engine -- 512 x 512 batch 4 (CFG batch 8, 50 DDIM steps), synthetic weights, LoRA rank 128
merged, hipGraph on -- and times whole generations between synchronisations at 77, 154 and 231 text rows (+ 4 ID tokens).
77 rows run the default launch sequences (the one-launch fused kernel at level 0, the query projection with the attention
epilogue below it); 154 and 231 rows run every cross-attention layer as q GEMM + cid_id_xattn_long_f16 + out GEMM.  A
change of context length re-captures the step graph, so every timed generation follows an untimed one of the same length."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXT_ROWS = (77, 154, 231)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    from consistentid_amd import pipeline, synth, unet_spec
    from consistentid_amd.unet import HipUNet
    dev = torch.device("cuda:0")
    cfg, side, B, steps, g, merge = unet_spec.sd15_config(), 512, 4, 50, 5.0, 30
    sd = synth.random_unet_state_dict(cfg, seed=0, device=dev)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=128, seed=1, device=dev)
    unet = HipUNet(cfg, sd, ad, device=dev)
    del sd, ad
    torch.cuda.empty_cache()
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=True)
    calls = {}
    for T in TEXT_ROWS:
        inp = synth.random_inputs(cfg, B, side, side, seed_latents=2024, seed_embeds=1, text_len=T, device=dev)
        calls[T] = dict(prompt_embeds=torch.cat([inp["null"], inp["augmented"], inp["text"]]), latents=inp["latents"],
                        num_inference_steps=steps, guidance_scale=g, start_merge_step=merge, output_type="latent")

    def generation(T):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(**calls[T]).images
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out.float()).all()
        return dt

    ms = {T: [] for T in TEXT_ROWS}
    paths = {}
    for p in range(a.passes):
        for T in TEXT_ROWS:
            generation(T)                                   # untimed: re-captures the step graph
            ms[T].append(generation(T) * 1e3)
            if T not in paths:
                seen = {}
                for blk in unet.downs:                      # one transformer per width: 64 x 64, 32 x 32, 16 x 16 tokens
                    for t in blk.attentions[:1]:
                        n = (side // 8) ** 2 * 320 * 320 // t.channels ** 2
                        seen[t.channels] = unet.cross_attention_path(f"{t.name}.transformer_blocks.0", t.channels, 2 * B, n)
                paths[T] = seen
    lines = [f"{torch.cuda.get_device_name(0)}; SD1.5 {side} x {side}, batch {B} (CFG batch {2 * B}), {steps} DDIM steps, hipGraph on; "
             f"{a.passes} passes, context lengths alternating, one process"]
    base = min(ms[TEXT_ROWS[0]])
    for T in TEXT_ROWS:
        best = min(ms[T])
        lines.append(f"{T:4d} text rows + 4 ID rows: ms per generation {' '.join(f'{x:.2f}' for x in ms[T])}; best pass "
                     f"{best / steps * 1e3:.1f} us per step ({(best / base - 1) * 100:+.2f} % against {TEXT_ROWS[0]} rows)")
        for c, path in sorted(paths[T].items()):
            lines.append(f"       C = {c:4d}: {path}")
    report = "\n".join(lines)
    print(report, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
