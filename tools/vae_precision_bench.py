#!/usr/bin/env python3
"""Cost and distance of the AutoencoderKL storage modes -> profiles/vae_precision.json.

Timing (full SD-v1.4 configuration, 512 x 512, random weights): decode and encode of ONE chunk (what one plan invocation takes: 8
images for the 16-bit plans, 4 for the fp32-storage ones) for bf16, fp16, fp32 and bf16x3 -- device events around the call, `--warmup`
untimed calls of the same shape, `--repeats` timed ones; median, minimum and maximum are recorded, per chunk and per image, with the
achieved algorithmic TFLOP/s (sdn_unet_flops over the median).  The clocks `rocm-smi --showclocks` reports are noted before and
after (read only).  Then a 64-image decode_latents_uint8 on the bf16 and the bf16x3 VAE; with `--bench-json FILE` (a line printed
by `bench.py --gpus 1`, whose ms_per_step is one 64-prompt end-to-end call with the bf16 decode inside) the share of that call a
bf16x3 decode would add is (t_bf16x3 - t_bf16) / ms_per_step.  Without the file the share is recorded as not measured.

Distance (small configurations of tests/test_gpu_vae_precise.py, synthetic weights): rel L2 of every mode's decoder / encoder from
the float64 reference on the same inputs, next to the CPU fp32 oracle's own distance (e32), and the share of uint8 values that
differ from the float64 image on the small pipeline's latents.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.vae import OracleVAEDecoder, OracleVAEEncoder  # noqa: E402
from safe_denoiser_amd.vae import AutoencoderKL  # noqa: E402
from tests_support.vae_oracle64 import OracleVAE64, rel_l2  # noqa: E402

MODES = {"bf16": dict(dtype=torch.bfloat16), "fp16": dict(dtype=torch.float16), "fp32": dict(precision="fp32"),
         "bf16x3": dict(precision="bf16x3")}


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k or "fclk" in k}
    except Exception as e:                                                   # the figure is a note, not a measurement
        return {"not read": repr(e)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=repeats)


def time_modes(args):
    out = {}
    for name, kw in MODES.items():
        v = AutoencoderKL(**kw)
        v.load_synthetic_on_device(5)
        enc = v._encoder()
        enc.load_synthetic_on_device(6)
        n = v.MAX_CHUNK
        z = torch.randn(n, 4, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        x = torch.rand(n, 3, 512, 512, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 2 - 1
        row = {"images_per_chunk": n}
        for what, fn, model in (("decode", lambda: v.decode(z), v), ("encode", lambda: v.encode(x), enc)):
            t = timed(fn, args.warmup, args.repeats)
            fl, _ = model.flops(n)
            t.update(ms_per_image=t["median_ms"] / n, tflop_per_image=fl / n / 1e12, tflops=fl / t["median_ms"] / 1e9)
            row[what] = t
            print(f"{name:7s} {what}: {n} images {t['median_ms']:9.2f} ms (min {t['min_ms']:.2f}, max {t['max_ms']:.2f}) "
                  f"= {t['ms_per_image']:.2f} ms per image, {t['tflops']:.1f} TFLOP/s", flush=True)
        out[name] = row
        del v, enc
        torch.cuda.empty_cache()
    return out


def time_64(args):
    out = {}
    lat = torch.randn(64, 4, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 0.18215
    for name in ("bf16", "bf16x3"):
        v = AutoencoderKL(**MODES[name])
        v.load_synthetic_on_device(5)
        out[name] = timed(lambda: v.decode_latents_uint8(lat), 1, max(3, args.repeats // 2))
        print(f"{name:7s} decode_latents_uint8 of 64 images: {out[name]['median_ms']:.1f} ms", flush=True)
        del v
        torch.cuda.empty_cache()
    added = out["bf16x3"]["median_ms"] - out["bf16"]["median_ms"]
    res = {"decode_64_images": out, "bf16x3_minus_bf16_ms": added}
    if args.bench_json:
        line = json.loads([l for l in open(args.bench_json).read().splitlines() if l.startswith("{")][-1])
        res["e2e_call_ms"] = line["ms_per_step"]
        res["e2e_call"] = f"bench.py --gpus 1, {line['config']['prompts_per_batch']} prompts per call, {line['value']:.3f} images/sec"
        res["share_of_e2e_call_added"] = added / line["ms_per_step"]
        print(f"a bf16x3 decode adds {added:.1f} ms to a {line['ms_per_step']:.0f} ms call: {100 * res['share_of_e2e_call_added']:.2f} %")
    else:
        res["share_of_e2e_call_added"] = "not measured (no --bench-json)"
    return res


def distances():
    small = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=16)
    small_o = dict(block_out_channels=(64, 128), layers_per_block=1)
    sd = AutoencoderKL(**small).synthetic_state_dict(3, with_encoder=True)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(3, 4, 8, 8, generator=g)
    x = torch.randn(3, 3, 16, 16, generator=g).clamp(-1, 1)
    o64 = OracleVAE64(sd, small_o)
    d64, m64 = o64.decode(z, 1.0 / 0.18215), o64.encode(x)
    out = {"config": "block_out_channels (64, 128), layers_per_block 1, 16 x 16 images, batch 3, synthetic weights (seed 3)",
           "measure": "rel L2 against the float64 reference",
           "cpu_fp32_oracle": {"decoder": rel_l2(OracleVAEDecoder(sd, small_o).decode(z, 1.0 / 0.18215), d64),
                               "encoder": rel_l2(OracleVAEEncoder(sd, small_o).encode(x), m64)}}
    # uint8 images: the small pipeline's VAE (32 x 32 images) on latents of its scale
    pcfg = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=32)
    psd = AutoencoderKL(**pcfg).synthetic_state_dict(4)
    lat = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(7)) * 0.18215 * 3.0
    ref8 = OracleVAE64(psd, small_o).image_uint8(lat).int()
    for name, kw in MODES.items():
        v = AutoencoderKL(**kw, **small)
        v.load_state_dict(sd)
        p = AutoencoderKL(**kw, **pcfg)
        p.load_state_dict(psd)
        d8 = (p.decode_latents_uint8(lat.cuda()).cpu().int() - ref8).abs()
        out[name] = {"decoder": rel_l2(v.decode(z.cuda(), latent_scale=1.0 / 0.18215).sample, d64),
                     "encoder": rel_l2(v.encode(x.cuda()).latent_dist.parameters, m64),
                     "uint8_share_differing": float((d8 > 0).float().mean()), "uint8_max_levels": int(d8.max())}
        print(f"{name:7s} distance from float64: decoder {out[name]['decoder']:.3e}, encoder {out[name]['encoder']:.3e}, "
              f"uint8 values differing {100 * out[name]['uint8_share_differing']:.3f} %", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_precision.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bench-json", help="file holding a result line of `bench.py --gpus 1` taken in the same session")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vae_precision_bench.py measures on an MI355X: there is nothing to record without one")
    res = {"device": torch.cuda.get_device_name(0), "clocks_before": clocks(),
           "method": "device events around each call, median of `repeats` after `warmup` untimed calls; one process, nothing else timed",
           "warmup": args.warmup}
    res["distance"] = distances()
    res["time_per_chunk_512"] = time_modes(args)
    res["end_to_end"] = time_64(args)
    res["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
