#!/usr/bin/env python3
"""MMDiT forward timing, SD3-medium beside SD-3.5-medium (q/k RMS norm, 13 dual-attention blocks), in ONE process and session:

    python tools/bench_mmdit35.py --config both --batch 32 --side 64 --iters 20 --out profiles/sd35_mmdit.json

Per configuration: the forward time over `iters` timed forwards after two warm-up forwards (device events; median, min, max), the
per-kernel rows of one profiled forward (HIP events around every launch: sdn_unet_profile_read), and for the row-wise norm kernels
(k_qk_rmsnorm, k_layernorm) one line per (kernel, rows, width) with the algorithmic bytes of the plan over the measured time.
To compare with another commit, copy this file into that commit's tools/ directory and run it there with --config sd3-medium (the
configurations are looked up lazily, so a tree without SD35_MEDIUM still runs SD3-medium); alternate the two commands to see the
run-to-run spread before reading a difference.

SD-3.5-large (38 blocks, 2432 wide) beside SD-3.5-medium, with the full-size row check (the B = 2 forward is finite and each of its
rows equals that row's B = 1 forward, bit for bit):

    python tools/bench_mmdit35.py --config sd35-medium,sd35-large --batch 8 --iters 10 --check-rows --out profiles/sd35_large.json"""
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

CONFIGS = {"sd3-medium": lambda: mmdit.SD3_MEDIUM, "sd35-medium": lambda: mmdit.SD35_MEDIUM, "sd35-large": lambda: mmdit.SD35_LARGE}
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


def measure(name, batch, side, iters, dtype, check_rows=False):
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
    rows_ok = None
    if check_rows:                                              # full plan at B = 2: finite, and every row is its own B = 1 forward
        y2 = m(x[:2], timestep=900.0, encoder_hidden_states=e[:2], pooled_projections=pl[:2])[0]
        y1 = [m(x[i:i + 1], timestep=900.0, encoder_hidden_states=e[i:i + 1], pooled_projections=pl[i:i + 1])[0] for i in range(2)]
        torch.cuda.synchronize()
        rows_ok = dict(finite=bool(torch.isfinite(y2).all()), rows_equal_b1=bool(torch.equal(y2[:1], y1[0]) and torch.equal(y2[1:], y1[1])),
                       std=float(y2.float().std()))
        print(f"{name}: B = 2 forward {rows_ok}")
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
               norm_kernels=norm_rows, b2_row_check=rows_ok)
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
    ap.add_argument("--config", default="both", help="one of %s, a comma-separated list of them, or both (= the two medium ones)" % ", ".join(CONFIGS))
    ap.add_argument("--check-rows", action="store_true", help="also run the plan at B = 2 and compare each row with its B = 1 forward")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=["float16", "bfloat16"], default="float16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    names = ["sd3-medium", "sd35-medium"] if a.config == "both" else a.config.split(",")
    assert all(n in CONFIGS for n in names), names
    res = dict(runs=[measure(n, a.batch, a.side, a.iters, getattr(torch, a.dtype), a.check_rows) for n in names])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
