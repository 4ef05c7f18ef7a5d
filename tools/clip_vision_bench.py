#!/usr/bin/env python3
"""Throughput of the Q16 image path at full size: uint8 images [B, 512, 512, 3] on the GPU -> resize + normalise -> CLIP ViT-L/14
tower -> similarities, B = 64, fp16 and bf16 storage, synthetic weights.  Recorded, not gated: writes
profiles/clip_vision_bench.json (images per second, milliseconds per batch for the tower alone and for the whole chain)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_denoiser_amd import clip_vision as V  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision_bench.json"))
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    u8 = torch.randint(0, 256, (args.batch, args.side, args.side, 3), generator=g, device="cuda", dtype=torch.uint8)
    prompts = torch.randn(2, 768, generator=torch.Generator().manual_seed(1))
    result = {"batch": args.batch, "side": args.side, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    for tag, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        m = V.CLIPVisionModelWithProjection(dtype=dt)
        m.load_synthetic_on_device(7)
        q16 = V.Q16Classifier(m, prompts)
        pv = V.clip_preprocess(u8)
        ms_pre = timed(lambda: V.clip_preprocess(u8), args.warmup, args.iters)
        ms_tower = timed(lambda: m(pv, output_hidden_state=False), args.warmup, args.iters)
        ms_chain = timed(lambda: q16.classify(u8), args.warmup, args.iters)
        total, _ = m.flops(args.batch)
        result[tag] = {"preprocess_ms": ms_pre, "tower_ms": ms_tower, "chain_ms": ms_chain, "images_per_s": 1e3 * args.batch / ms_chain,
                       "tower_tflops": total / ms_tower / 1e9}
        print(tag, result[tag])
        del m, q16
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
