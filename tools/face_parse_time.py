#!/usr/bin/env python3
"""Time the face parse of one ID image (B = 1 at 512 x 512, random conditioned weights with the checkpoint's shapes).

    python tools/face_parse_time.py [--iters 20] [--warmup 5]

HIP: HipBiSeNet labels (stem, cid_gemm_f16 with the ReLU epilogue, pooled branches, bilinear + argmax head).
Torch fp32: the restatement of tests/bisenet_ref.py on the same GPU in fp32 (the reference's precision), main head and the
argmax included.  The parse runs once per image, before the denoise loop; bench.py does not include it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


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
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from bisenet_ref import _Net, calibrate, make_image, random_state_dict
    from consistentid_amd.face_parsing import HipBiSeNet
    dev = torch.device("cuda:0")
    sd = random_state_dict(seed=11)
    calibrate(sd, make_image(1, 512, 512, seed=100))
    img = make_image(1, 512, 512, seed=201).to(dev)
    net = HipBiSeNet(sd, device=dev)
    hip_ms = timed(lambda: net(img), args.iters, args.warmup)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    ref = _Net(sd_dev, torch.float32)

    def torch_fp32():
        with torch.no_grad():
            ref.forward(img).argmax(1).to(torch.uint8)

    torch_ms = timed(torch_fp32, args.iters, args.warmup)
    print(json.dumps({"face_parse_512_b1": {"hip_ms": round(hip_ms, 3), "torch_fp32_ms": round(torch_ms, 3),
                                            "speedup": round(torch_ms / hip_ms, 2)}}))


if __name__ == "__main__":
    main()
