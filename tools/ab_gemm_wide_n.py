#!/usr/bin/env python3
"""A/B of the GEMMs of a 2432-wide MMDiT block whose N neither 256 nor 320 divides (SD-3.5-large: attention output projection
N = K = 2432, FF2 N = 2432 / K = 9728, stacked QKV N = 7296 / K = 2432), each with its real epilogue (bias; row gate + residual for
the first two), fp16 and bf16, M = 8 x 1024 image rows and 8 x 333 text rows, in ONE process:

    python tools/ab_gemm_wide_n.py --out profiles/sd35_large_gemm_ab.json

  base   what sdn_gemm_pick_tile chooses: the 128 x 128 tile (NREP 4, WGM 2)
  tall   candidate (a): the same 128 columns on 256 rows (k_gemm_dma<T, 4, 4>, debug variant 7)
  pad    candidate (b): the weight padded with zero rows to the next multiple of 320 (2560, 7360), n_valid = N, on whatever tile the
         padded N is given (256 x 320 once the grid fills the chip)

Per shape the three run alternating (base, tall, pad, base, ...) for `rounds` rounds of `iters` launches each, timed with device events
around the `iters` launches; the figure of a round is the mean per launch.  `spread` = (max - min) / median of base's rounds: a candidate
wins a shape only if its median is below base's by more than that.  Before timing, every candidate's output is compared with base's
(same operands: the tiles sum in the same k order, so the results are expected equal bit for bit; the maximum difference is recorded)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safe_denoiser_amd as sda  # noqa: E402
from tests_support import ops  # noqa: E402

SHAPES = {"attn_out": (2432, 2432, True), "ff2": (2432, 9728, True), "qkv": (7296, 2432, False)}


def last_launch():
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    return list(rec)[:9]


def run_shape(name, M, rpb, dt, rounds, iters):
    N, K, gated = SHAPES[name]
    Np = (N + 319) // 320 * 320
    g = torch.Generator().manual_seed(N + K + M)
    a = torch.randn(M, K, generator=g).to(dt).cuda()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).cuda()
    wp = torch.zeros(Np, K, dtype=dt, device="cuda"); wp[:N] = w
    bias = torch.zeros(Np, device="cuda"); bias[:N] = torch.randn(N, generator=g).cuda()
    nb = (M + rpb - 1) // rpb
    gate = res = None
    if gated:
        gate = torch.zeros(nb, Np, device="cuda"); gate[:, :N] = (torch.randn(nb, N, generator=g) * 0.5).cuda()
        res = torch.randn(M + 8, N, generator=g).to(dt).cuda()[:M]      # (slack rows: a padded tile's residual fetch runs past column N)
    outs = {k: torch.empty(M, N, dtype=dt, device="cuda") for k in ("base", "tall", "pad")}
    kw = dict(residual=res, rows_per_batch=rpb if gated else 0)

    def launch(kind):
        if kind == "pad":
            ops.gemm(a, wp, bias=bias, rowgate=gate, n_valid=N, out=outs[kind], **kw)
        else:
            sda.lib().sdn_debug_set_gemm_variant(7 if kind == "tall" else 0)
            ops.gemm(a, w, bias=bias[:N], rowgate=None if gate is None else gate[:, :N], out=outs[kind], **kw)
            sda.lib().sdn_debug_set_gemm_variant(0)

    tiles = {}
    for kind in outs:
        launch(kind)
        tiles[kind] = last_launch()
    torch.cuda.synchronize()
    diff = {k: float((outs[k].float() - outs["base"].float()).abs().max()) for k in ("tall", "pad")}
    ms = {k: [] for k in outs}
    for _ in range(rounds):
        for kind in outs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                launch(kind)
            e1.record(); torch.cuda.synchronize()
            ms[kind].append(e0.elapsed_time(e1) / iters)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms["base"]) - min(ms["base"])) / med["base"]
    fl = 2.0 * M * N * K
    row = dict(shape=name, M=M, N=N, K=K, dtype=str(dt), launch_record=tiles, max_abs_diff_vs_base=diff, ms_median=med,
               ms_rounds=ms, base_spread=spread, tflops={k: fl / v / 1e9 for k, v in med.items()},
               ratio_vs_base={k: med[k] / med["base"] for k in ("tall", "pad")},
               wins={k: bool(med[k] < med["base"] * (1 - spread)) for k in ("tall", "pad")})
    print(f"{name:9s} M {M:5d} {str(dt):15s} base {med['base']:.4f} ms (spread {spread * 100:.1f} %)  tall x{row['ratio_vs_base']['tall']:.3f}  "
          f"pad x{row['ratio_vs_base']['pad']:.3f}  diff {diff}  tiles {tiles}")
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    rows = [run_shape(n, M, rpb, dt, a.rounds, a.iters) for n in SHAPES for (M, rpb) in ((8 * 1024, 1024), (8 * 333, 333))
            for dt in (torch.float16, torch.bfloat16)]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(rounds=a.rounds, iters=a.iters, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
