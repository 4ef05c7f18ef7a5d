#!/usr/bin/env python3
"""Throughput of the Inception-v3 pool3 tower at full size: float images [B, 3, 299, 299] on the GPU -> 2048 features, B = 32 (one
plan invocation), fp32 storage, synthetic weights; and the whole FID path from uint8 [B, 512, 512, 3] (Pillow's resize to 256, the
tower with its resize to 299).  Recorded, not gated: writes profiles/inception_bench.json."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_denoiser_amd.inception import InceptionV3  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inception_bench.json"))
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(args.batch, 3, 299, 299, generator=g, device="cuda")
    u8 = torch.randint(0, 256, (args.batch, 512, 512, 3), generator=g, device="cuda", dtype=torch.uint8)
    m = InceptionV3()
    m.load_synthetic_on_device(7)
    ms_tower = timed(lambda: m(x), args.warmup, args.iters)
    ms_chain = timed(lambda: m.get_activations(u8, args.batch), args.warmup, args.iters)
    total, _ = m.flops(args.batch)
    result = {"batch": args.batch, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "weights": "synthetic",
              "tower_ms": ms_tower, "tower_images_per_s": 1e3 * args.batch / ms_tower, "tower_tflops": total / ms_tower / 1e9,
              "gflop_per_image": total / args.batch / 1e9, "fid_path_from_u8_512_ms": ms_chain,
              "fid_path_images_per_s": 1e3 * args.batch / ms_chain}
    m.profile_next()
    m(x)
    torch.cuda.synchronize()
    result["kernels"] = m.profile_read()
    print(json.dumps(result, indent=1))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
