#!/usr/bin/env python3
"""The two projected CLIP text encoders of SD-v3 on the engine (OpenCLIP bigG, 32 layers, and CLIP-L, 12 layers; synthetic weights,
device events) at the shape encode_prompt runs them: 128 sequences of 77 tokens = 64 prompts + 64 negatives, fp16 and bf16.
Reports ms per forward (median of --iters after --warmup), achieved TFLOP/s against the plan's own FLOP count (sdn_unet_flops), the
per-kernel split of one profiled forward (sdn_unet_profile_next: event-to-event times per launch, summed by kernel label), and the
feed-forward's first GEMM alone (M = 9856, 1280 -> 5120 / 768 -> 3072) with SDN_ACT_GELU, SDN_ACT_QUICK_GELU and SDN_ACT_NONE, so
that the cost of the activation epilogue is a number.  `transformers` on the same card is recorded beside it when it can be run
there (--hf), left out with a note otherwise: a comparison, not a gate.  Writes profiles/clip_proj_bench.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import safe_denoiser_amd as sda  # noqa: E402
from safe_denoiser_amd import _lib  # noqa: E402
from safe_denoiser_amd.clip import CLIPTextModelWithProjection, SD3_CLIP_G_CONFIG, SD3_CLIP_L_CONFIG  # noqa: E402

ENCODERS = {"big_g": dict(SD3_CLIP_G_CONFIG, hidden_act="gelu", projection_dim=1280, eos_token_id=2),
            "clip_l": dict(SD3_CLIP_L_CONFIG, hidden_act="quick_gelu", projection_dim=768, eos_token_id=2)}
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def ff1_alone(tag, M, N, K, warmup, iters):
    """FF1 of one layer as the plan launches it, once per activation code."""
    dt = DT[tag]
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(M, K, generator=g, device="cuda").to(dt)
    w = (torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).to(dt)
    bias = torch.randn(N, generator=g, device="cuda") * 0.1
    out = torch.empty(M, N, dtype=dt, device="cuda")
    fn = sda.lib().sdn_gemm_f16 if tag == "f16" else sda.lib().sdn_gemm_bf16
    row = {}
    for name, act in (("none", 0), ("quick_gelu", 4), ("gelu_erf", 7), ("gelu_tanh", 3)):
        d = _lib.GemmDesc(M=M, N=N, K=K, act=act)

        def run():
            _lib.check(fn(C.byref(d), a.data_ptr(), None, w.data_ptr(), bias.data_ptr(), None, None, None, out.data_ptr(), _lib.stream_ptr()), "gemm")
        med, lo, hi = timed(run, warmup + 3, 4 * iters)
        row[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "tflops": 2.0 * M * N * K / med / 1e9}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hf", action="store_true", help="also time transformers' CLIPTextModelWithProjection (random weights) on this card")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_proj_bench.json"))
    args = ap.parse_args()
    B = args.batch
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "warmup": args.warmup, "iters": args.iters, "cases": {}, "ff1_alone": {}}
    if not args.hf:
        res["transformers_note"] = "not measured in this run (pass --hf)"
    ids = torch.randint(1, 49000, (B, 77), generator=torch.Generator().manual_seed(0))
    ids[:, 0] = 49406
    ids[:, 20:] = 49407
    ids = ids.cuda()
    for name, cfg in ENCODERS.items():
        for tag, dt in DT.items():
            m = CLIPTextModelWithProjection(dtype=dt, **cfg).load_synthetic_on_device(7)
            hidden = torch.zeros(B, 333, 4096, dtype=dt, device="cuda")
            pooled = torch.zeros(B, 2048, dtype=dt, device="cuda")
            hv, pv = hidden[:, :77, :cfg["hidden_size"]], pooled[:, :cfg["projection_dim"]]
            run = lambda: m.forward_into(ids, hv, pv)                   # noqa: E731  (into slices of the joint buffers, as the front end does)
            med, lo, hi = timed(run, args.warmup, args.iters)
            flops, attn = m.flops(B)
            row = {"ms_median": med, "ms_min": lo, "ms_max": hi, "flops": flops, "attention_core_flops": attn, "tflops": flops / med / 1e9}
            m.profile_next()
            run()
            row["per_kernel"] = sorted(m.profile_read(), key=lambda r: -r["ms"])
            if args.hf:
                try:
                    from transformers import CLIPTextConfig, CLIPTextModelWithProjection as HF
                    with torch.device("cuda"):
                        hf = HF(CLIPTextConfig(attention_dropout=0.0, pad_token_id=1, bos_token_id=0, **cfg))
                    hf = hf.to(dt).eval()
                    with torch.no_grad():
                        row["transformers_ms_median"] = timed(lambda: hf(ids.long(), output_hidden_states=True), args.warmup, args.iters)[0]
                    del hf
                except Exception as e:                                   # noqa: BLE001
                    res["transformers_note"] = f"not measured: {type(e).__name__}: {e}"
            res["cases"][f"{name}/{tag}"] = row
            print(name, tag, json.dumps({k: v for k, v in row.items() if k != "per_kernel"}))
            for r in row["per_kernel"]:
                print("   ", json.dumps(r))
            del m
            torch.cuda.empty_cache()
        for tag in DT:
            res["ff1_alone"][f"{name}/{tag}"] = ff1_alone(tag, B * 77, cfg["intermediate_size"], cfg["hidden_size"], args.warmup, args.iters)
            print(name, tag, "ff1 alone", json.dumps(res["ff1_alone"][f"{name}/{tag}"]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
