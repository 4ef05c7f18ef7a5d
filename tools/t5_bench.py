#!/usr/bin/env python3
"""T5-XXL on the engine at the three shapes the SD-v3 SAFREE front end runs (bf16, synthetic weights, device events):
  (a) encode_prompt's T5 part for 64 prompts + 64 negatives: two [64, 256] forwards without a mask;
  (b) the 17 concept phrases: [17, 256] with the padding mask;
  (c) one masked-token batch: [19, 21] without a mask.
Reports ms (median of --iters after --warmup), achieved TFLOP/s against the plan's own FLOP count (sdn_t5_flops), and for (c) the
GB/s of weight traffic (that forward reads every matrix once for 399 rows) plus the per-kernel split of one profiled forward
(sdn_unet_profile_next: event-to-event times per launch, summed by kernel).  `transformers` on the same card is
recorded beside it when it can be run there (--hf), left out with a note otherwise.  Writes profiles/t5_xxl_bench.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_denoiser_amd.t5 import T5EncoderModel, T5_XXL_CONFIG  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=T5_XXL_CONFIG["num_layers"])
    ap.add_argument("--hf", action="store_true", help="also time transformers' T5EncoderModel (bf16, random weights) on this card")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_xxl_bench.json"))
    args = ap.parse_args()
    m = T5EncoderModel(dtype=torch.bfloat16, num_layers=args.layers).load_synthetic_on_device(7)
    g = torch.Generator().manual_seed(0)
    mat_bytes = sum(p["rows"] * p["cols"] * 2 for p in m.manifest if p["cols"] and p["name"] != "embed_tokens.weight")
    shapes = {"a_encode_prompt_2x[64,256]": ((64, 256), False, 2), "b_phrases_[17,256]_masked": ((17, 256), True, 1),
              "c_masked_tokens_[19,21]": ((19, 21), False, 1)}
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "num_layers": args.layers, "warmup": args.warmup, "iters": args.iters,
           "matrix_weight_bytes": mat_bytes, "cases": {}}
    hf = None
    if args.hf:
        try:
            from transformers import T5Config, T5EncoderModel as HF
            cfg = {k: v for k, v in T5_XXL_CONFIG.items()}
            cfg["num_layers"] = args.layers
            with torch.device("cuda"):
                hf = HF(T5Config(feed_forward_proj="gated-gelu", is_encoder_decoder=False, use_cache=False, dropout_rate=0.0, **cfg))
            hf = hf.to(torch.bfloat16).eval()
        except Exception as e:                                         # noqa: BLE001
            res["transformers_note"] = f"not measured: {type(e).__name__}: {e}"
    else:
        res["transformers_note"] = "not measured in this run (pass --hf)"
    for name, ((b, n), masked, reps) in shapes.items():
        ids = torch.randint(2, 32128, (b, n), generator=g).cuda()
        mask = None
        if masked:
            mask = (torch.arange(n)[None] < torch.randint(2, 8, (b, 1), generator=g)).long().cuda()

        def run():
            for _ in range(reps):
                m(ids, attention_mask=mask)
        med, lo, hi = timed(run, args.warmup, args.iters)
        flops = reps * m.flops(b, n)[0]
        row = {"ms_median": med, "ms_min": lo, "ms_max": hi, "flops": flops, "tflops": flops / med / 1e9}
        if name.startswith("c_"):
            row["weight_gb_per_s"] = mat_bytes / med / 1e6
            m.profile_next()
            run()
            row["per_kernel"] = sorted(m.profile_read(), key=lambda r: -r["ms"])
        if hf is not None:
            with torch.no_grad():
                def run_hf():
                    for _ in range(reps):
                        hf(ids.long(), attention_mask=mask)
                row["transformers_ms_median"] = timed(run_hf, args.warmup, args.iters)[0]
        res["cases"][name] = row
        print(name, json.dumps(row))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
