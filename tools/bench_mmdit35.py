#!/usr/bin/env python3
"""MMDiT forward timing, SD3-medium beside SD-3.5-medium (q/k RMS norm, 13 dual-attention blocks), in ONE process and session:

    python tools/bench_mmdit35.py --config both --batch 32 --side 64 --iters 20 --out profiles/sd35_mmdit.json

Per configuration: the forward time over `iters` timed forwards after two warm-up forwards (device events; median, min, max), the
per-kernel rows of one profiled forward (HIP events around every launch: sdn_unet_profile_read), and for the row-wise norm kernels
(k_qk_rmsnorm, k_layernorm) one line per (kernel, rows, width) with the algorithmic bytes of the plan over the measured time.
To compare with another commit, copy this file into that commit's tools/ directory and run it there with --config sd3-medium (the
configurations are looked up lazily, so a tree without SD35_MEDIUM still runs SD3-medium); alternate the two commands to see the
run-to-run spread before reading a difference."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safe_denoiser_amd as sda  # noqa: E402
from safe_denoiser_amd import mmdit  # noqa: E402

CONFIGS = {"sd3-medium": lambda: mmdit.SD3_MEDIUM, "sd35-medium": lambda: mmdit.SD35_MEDIUM}
NORM_KERNELS = ("k_qk_rmsnorm", "k_layernorm")


def per_op_rows(m):
    """(label, M, N) -> [launches, ms, bytes] of the profiled forward (sdn_debug_profile_ops: one row per launch, in plan order)."""
    lib = sda.lib()
    lib.sdn_debug_profile_ops.restype = C.c_int
    lib.sdn_debug_profile_ops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    out = (C.c_double * (6 * 32768))()
    lab = C.create_string_buffer(24 * 32768)
    n = lib.sdn_debug_profile_ops(m._h, out, lab, 32768)
    agg = collections.OrderedDict()
    for i in range(max(n, 0)):
        name = lab.raw[i * 24:(i + 1) * 24].split(b"\0")[0].decode()
        a = agg.setdefault((name, int(out[i * 6 + 3]), int(out[i * 6 + 4])), [0, 0.0, 0.0])
        a[0] += 1; a[1] += out[i * 6]; a[2] += out[i * 6 + 2]
    return agg


def measure(name, batch, side, iters, dtype):
    cfg = dict(CONFIGS[name](), sample_size=side)
    m = mmdit.SD3Transformer2DModel(dtype=dtype, **cfg)
    m.load_synthetic_on_device(3)
    x = torch.randn(batch, 16, side, side, device="cuda"); e = torch.randn(batch, 333, 4096, device="cuda")
    pl = torch.randn(batch, 2048, device="cuda")
    call = lambda: m(x, timestep=900.0, encoder_hidden_states=e, pooled_projections=pl)[0]
    for _ in range(2):
        y = call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    fl, at = m.flops(batch)
    m.profile_next(); call(); torch.cuda.synchronize()
    rows = sorted(m.profile_read(), key=lambda r: -r["ms"])
    norm_rows = []
    for (label, M, N), (launches, ms, nbytes) in per_op_rows(m).items():
        if label in NORM_KERNELS:
            norm_rows.append(dict(kernel=label, rows=M, width=N, launches=launches, ms=ms, bytes=nbytes,
                                  tb_per_s=nbytes / (ms * 1e-3) / 1e12 if ms > 0 else None))
    med = statistics.median(ts)
    res = dict(config=name, batch=batch, side=side, dtype=str(dtype), iters=iters, forward_ms_median=med, forward_ms_min=min(ts),
               forward_ms_max=max(ts), forward_ms_all=ts, tflops=fl / med / 1e9, attention_flop_share=at / fl,
               parameters=sum(torch.Size(s).numel() for k, s in m.state_dict_shapes().items() if k != "pos_embed.pos_embed"),
               kernels=[dict(r, tflops=(r["flops"] / r["ms"] / 1e9) if r["ms"] > 0 else None,
                             tb_per_s=(r["bytes"] / r["ms"] / 1e9) if r["ms"] > 0 else None) for r in rows],
               norm_kernels=norm_rows)
    print(f"{name} side {side} B={batch} {dtype}: {med:.2f} ms per forward (min {min(ts):.2f}, max {max(ts):.2f}), {fl / med / 1e9:.1f} TFLOP/s")
    for r in rows[:14]:
        print(f"  {r['kernel']:20s} x{r['launches']:4d} {r['ms']:8.3f} ms  {(r['flops'] / r['ms'] / 1e9) if r['flops'] else 0:7.1f} TF/s  "
              f"{r['bytes'] / r['ms'] / 1e9:6.2f} TB/s")
    for r in norm_rows:
        print(f"  {r['kernel']:14s} rows {r['rows']:7d} width {r['width']:5d} x{r['launches']:3d}  {r['ms']:7.3f} ms  {r['tb_per_s']:.2f} TB/s")
    del m
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=list(CONFIGS) + ["both"], default="both")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=["float16", "bfloat16"], default="float16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    names = list(CONFIGS) if a.config == "both" else [a.config]
    res = dict(runs=[measure(n, a.batch, a.side, a.iters, getattr(torch, a.dtype)) for n in names])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
