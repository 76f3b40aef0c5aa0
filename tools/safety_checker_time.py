#!/usr/bin/env python3
"""Time one safety-checker call at B = 4 on the ViT-L/14 geometry (random weights; tests/safety_ref.py builds them).

    python tools/safety_checker_time.py

HipSafetyChecker.__call__ on a 4 x 3 x 512 x 512 fp16 device tensor (tower, cid_clip_head_f16, cid_blackout_f16, the flags
read back), cosines() alone, and the two kernels alone.  The checker runs once per generation, after the VAE decode;
bench.py does not include it.  Raw lines of one run: profiles/safety_checker_time.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import safety_ref
from transformers import CLIPVisionConfig
from consistentid_amd import ops
from consistentid_amd.safety import HipSafetyChecker

VIT_L = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14, projection_dim=768)
dev = torch.device("cuda:0")
ref = safety_ref.SafetyCheckerRef(CLIPVisionConfig(**VIT_L), seed=1)
sd = ref.checkpoint_state_dict()
sd["concept_embeds_weights"] = torch.full((17,), 0.2); sd["special_care_embeds_weights"] = torch.full((3,), 0.2)
chk = HipSafetyChecker({"vision_config": {"num_attention_heads": 16, "patch_size": 14}}, sd, device=dev)
B = 4
x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(2)).half().to(dev)
img = torch.rand(B, 3, 512, 512, generator=torch.Generator().manual_seed(3)).half().to(dev)

def timed(fn, n):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3

print("device", torch.cuda.get_device_name(0))
print("checker __call__ (tower + head + blackout + flags to host), B=4: median %.3f ms (min %.3f, max %.3f)" % timed(lambda: chk(clip_input=x, images=img), 30))
print("cosines only (tower + head), B=4: median %.3f ms (min %.3f, max %.3f)" % timed(lambda: chk.cosines(x), 30))
hx, g, b, w = chk.vision.head_inputs(x)
Bn, Np, C = hx.shape
def head(): ops.clip_head(hx, g, b, w, B=Bn, ldx=Np * C, eps=1e-5, concepts=chk.concepts, thresholds=chk.thresholds, n_special=3)
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(5): head()
torch.cuda.synchronize(); s.record()
for _ in range(200): head()
e.record(); torch.cuda.synchronize()
print("cid_clip_head_f16 alone, B=4, C=1024, P=768, K=20: %.2f us per launch (200 back-to-back launches, includes 3 torch.empty)" % (s.elapsed_time(e) / 200 * 1e3))
flags = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)
for _ in range(5): ops.blackout_(img, flags)
torch.cuda.synchronize(); s.record()
for _ in range(200): ops.blackout_(img, flags)
e.record(); torch.cuda.synchronize()
print("cid_blackout_f16 alone, 4 x 3 x 512 x 512 fp16, two flagged: %.2f us per launch" % (s.elapsed_time(e) / 200 * 1e3))
c, sc, fl = chk.cosines(x)
print("cos range", float(c.min()), float(c.max()), "flags", fl.tolist())
