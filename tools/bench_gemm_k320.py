#!/usr/bin/env python3
"""k_gemm_k320 (sdn_gemm_k320) against the generic entries (k_gemm_dma) on the five K = 320 forms of the C = 320 transformer
blocks, in process and interleaved (rounds alternate the two kernels on the same operands; median per kernel).  B = batch of the
forward (M = B * 4096 at the 64 x 64 level); the shared-prefix launches of a latent_repeat = 3 plan run at B / 3."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safe_denoiser_amd as sda  # noqa: E402
from safe_denoiser_amd import _lib  # noqa: E402
from tests_support import ops  # noqa: E402

B = int(os.environ.get("B", "192"))
DT = torch.float16 if os.environ.get("DTYPE") == "f16" else torch.bfloat16
ROUNDS, INNER = int(os.environ.get("ROUNDS", "7")), int(os.environ.get("INNER", "10"))
FORMS = [  # name, N, bias, residual, LayerNorm fold
    ("proj_in          N=320", 320, True, False, False),
    ("to_out + res /rp N=320", 320, True, True, False),
    ("to_q /ln1        N=320", 320, False, False, True),
    ("qkv /ln1         N=960", 960, False, False, True),
    ("plain            N=960", 960, False, False, False),
]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / INNER


def main():
    lib = sda.lib()
    code = 1 if DT == torch.float16 else 0
    print(f"# dtype {DT}, {ROUNDS} interleaved rounds x {INNER} launches, median us | TFLOP/s | algorithmic GB/s (A + out [+ residual])")
    print(f"{'form':24s} {'M':>8s}   {'k_gemm_dma':>26s}   {'k_gemm_k320':>26s}   ratio")
    for M in (B * 4096, B * 4096 // 3):
        for name, N, has_bias, has_res, ln in FORMS:
            a = torch.randn(M, 320, device="cuda").to(DT)
            w = (torch.randn(N, 320, device="cuda") * 320 ** -0.5).to(DT)
            bias = torch.randn(N, device="cuda") if has_bias else None
            res = torch.randn(M, N, device="cuda").to(DT) if has_res else None
            out0, out1 = torch.empty(M, N, device="cuda", dtype=DT), torch.empty(M, N, device="cuda", dtype=DT)
            p = lambda t: None if t is None else t.data_ptr()
            d = _lib.GemmDesc()
            d.M, d.N, d.K, d.res_pre = M, N, 320, 1 if has_res else 0
            if ln:
                gamma, beta = torch.rand(320, device="cuda") + 0.5, torch.randn(320, device="cuda") * 0.1
                fold = {}
                ops.gemm_ln(a[:64], w, gamma, beta, fold=fold)
                wf, c, dv = fold["w_folded"], fold["c"], fold["d"]
                gen = getattr(lib, "sdn_gemm_ln_f16" if code else "sdn_gemm_ln_bf16")
                old = lambda: gen(C.byref(d), p(a), p(wf), p(c), p(dv), 1e-5, None, p(out0), None)
                new = lambda: lib.sdn_gemm_k320(code, C.byref(d), p(a), p(wf), None, p(c), p(dv), 1e-5, None, p(out1), None)
            else:
                gen = getattr(lib, "sdn_gemm_f16" if code else "sdn_gemm_bf16")
                old = lambda: gen(C.byref(d), p(a), None, p(w), p(bias), None, None, p(res), p(out0), None)
                new = lambda: lib.sdn_gemm_k320(code, C.byref(d), p(a), p(w), p(bias), None, None, 0.0, p(res), p(out1), None)
            assert old() == 0 and new() == 0
            torch.cuda.synchronize()
            assert torch.equal(out0.view(torch.int16), out1.view(torch.int16)), f"{name}: the two kernels disagree"
            t = {0: [], 1: []}
            for _ in range(ROUNDS):
                t[0].append(timed(old))
                t[1].append(timed(new))
            flops = 2.0 * M * N * 320
            gbytes = 2.0 * M * (320 + N * (2 if has_res else 1)) / 1e9
            cell = lambda us: f"{us:8.1f} us {flops / us / 1e6:6.0f} TF {gbytes / us * 1e6:7.0f} GB/s"
            m0, m1 = statistics.median(t[0]), statistics.median(t[1])
            print(f"{name:24s} {M:8d}   {cell(m0)}   {cell(m1)}   {m0 / m1:5.3f}", flush=True)


if __name__ == "__main__":
    main()
