"""SD-v3 MMDiT precision plans: forward time of the fp16, fp32 and bf16x3 plans of SD3-medium at 512^2 (B = 32) and 1024^2 (B = 16),
and each plan's rel-L2 from the pure-fp32 oracle (OracleMMDiT, act_dtype=None, its torch ops on the GPU with TF32 off) on the same
inputs (the first two samples of the timed batch: samples do not interact).
    python tools/bench_sd3_precision.py [--out profiles/sd3_precision.json] [--iters N] [--sizes 64:32,128:16]
Timing: one warm-up forward, then N forwards between two device events (their mean).  Synthetic weights (seed 3)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.mmdit import OracleMMDiT  # noqa: E402
from safe_denoiser_amd.mmdit import SD3Transformer2DModel  # noqa: E402

PLANS = {"fp16": dict(dtype=torch.float16), "fp32": dict(precision="fp32"), "bf16x3": dict(precision="bf16x3")}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sizes", default="64:32,128:16", help="latent side:batch, comma separated")
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda")
    t0 = time.time()
    sd = SD3Transformer2DModel(sample_size=64).synthetic_state_dict(3)
    print(f"state dict: {time.time() - t0:.1f} s", flush=True)
    rows = []
    for spec in args.sizes.split(","):
        side, B = (int(v) for v in spec.split(":"))
        g = torch.Generator().manual_seed(4)
        x = torch.randn(B, 16, side, side, generator=g).to(dev)
        e = torch.randn(B, 333, 4096, generator=g).to(dev)
        pl = torch.randn(B, 2048, generator=g).to(dev)
        net = OracleMMDiT(sd, {"sample_size": side}, act_dtype=None, device=dev)
        ref = net(x[:2], 812.0, e[:2], pl[:2])
        del net
        torch.cuda.empty_cache()
        for name, kw in PLANS.items():
            m = SD3Transformer2DModel(sample_size=side, **kw)
            m.load_state_dict(sd)
            text, pooled = m.prepare_text(e), pl.to(m.dtype).contiguous()
            y = torch.empty(B, 16, side, side, device=dev)
            m.forward_into(x, 812.0, text, pooled, y)                       # warm-up (plan, workspace)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                m.forward_into(x, 812.0, text, pooled, y)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            flops = m.flops(B)[0]
            r = rel_l2(y[:2], ref)
            row = dict(plan=name, image=side * 8, batch=B, ms_per_forward=round(ms, 2), ms_per_sample=round(ms / B, 3),
                       tflops_algorithmic=round(flops / ms / 1e9, 1), rel_l2_vs_fp32_oracle=float(f"{r:.3e}"),
                       finite=bool(torch.isfinite(y).all()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del m, text, pooled, y
            torch.cuda.empty_cache()
    for side in sorted({r["image"] for r in rows}):
        base = next(r for r in rows if r["image"] == side and r["plan"] == "fp16")
        for r in rows:
            if r["image"] == side:
                r["speed_vs_fp16"] = round(base["ms_per_forward"] / r["ms_per_forward"], 3)
    result = dict(tool="tools/bench_sd3_precision.py", device=torch.cuda.get_device_name(0), iters=args.iters, timestep=812.0,
                  weights="synthetic seed 3", oracle="OracleMMDiT act_dtype=None on the GPU, TF32 off", rows=rows)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
