"""The GEMMs of a 2432-wide MMDiT block (SD-3.5-large) whose N neither 256 nor 320 divides -- the attention output projection
(N = K = 2432), FF2 (N = 2432, K = 9728) and the stacked QKV (N = 7296, K = 2432) -- each with its real epilogue (bias only for QKV;
bias, per-sample row gate and residual for the other two), element by element against float64 arithmetic on the same 16-bit operands by
the criterion of tests/test_gpu_gemm_exact.py (tests_support/exact.py).  M = 333 (three tiles of 128 with a ragged last one) and
1024 + 19 (one row block past eight tiles, the gate's sample boundary inside a tile).

No new tile is selected for these shapes (both candidates were measured and not kept: DESIGN 10.24,
profiles/sd35_large_gemm_ab.json): they run where sdn_gemm_pick_tile put them before, which the launch record pins -- the 128 x 128 tile (NREP 4, WGM 2) once the grid fills the chip, the 128 x 64 one (NREP 2) below 256 workgroups -- together
with the tiles of N = 1536, 4608 and 1280 at a batch that fills the chip."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from tests_support import exact as X
from tests_support import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = {"attn_out": dict(N=2432, K=2432, gated=True), "ff2": dict(N=2432, K=9728, gated=True), "qkv": dict(N=7296, K=2432, gated=False)}
ROWS = {333: 111, 1043: 1024}                  # M -> rows per sample of the gate


def _last_launch():
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    return list(rec)


def _small_tile_key(M, N):
    """sdn_gemm_pick_tile for an N that only 128 divides: NREP 4 unless that leaves fewer than 256 workgroups."""
    return ("dma", 4 if ((M + 127) // 128) * (N // 128) >= 256 else 2, 2, 2, 0)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("M", list(ROWS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_wide_block_gemm_is_exact(shape, M, dt):
    N, K, gated = SHAPES[shape]["N"], SHAPES[shape]["K"], SHAPES[shape]["gated"]
    rpb = ROWS[M]
    g = torch.Generator().manual_seed(K + M + (1 if dt == torch.float16 else 0))
    t = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dt).cuda()
    a = X.with_nan_tail(t(M, K), 64)
    w = t(N, K, scale=K ** -0.5)
    bias = torch.randn(N, generator=g).cuda()
    gate = res = None
    if gated:
        gate = (torch.randn((M + rpb - 1) // rpb, N, generator=g) * 0.5).cuda()
        res = X.nan_strided(t(M, N), N + 8)                           # (the residual shares the output's row stride)
    buf, out = X.guarded(M, N, dt, "cuda", ldc=N + 8)
    ops.gemm(a, w, bias=bias, rowgate=gate, residual=res, rows_per_batch=rpb if gated else 0, out=out)
    rec = _last_launch()
    torch.cuda.synchronize()
    assert X.launch_key(rec) == _small_tile_key(M, N), (rec, _small_tile_key(M, N))
    y, s, e, y32 = X.reference(a, w, bias=bias, rowgate=gate, residual=res, rpb=rpb if gated else 0)
    st = X.analyse(out, y, s, e, dtype=dt)
    fails = X.failures(st, exact_fn=True, ref_rate=X.ref_rate(y32, y, dt) if y32 is not None else None)
    bad = X.sentinels_intact(buf, out)
    if bad:
        fails.append(f"{bad} guard-band sentinels overwritten")
    print(dict(case=f"{shape} M {M}", dtype=str(dt), inst=X.launch_key(rec), tiles=rec[6:9], max_ulp=round(st["max_ulp"], 3),
               max_err_over_bound=round(st["max_err_over_tol"], 3), rate=round(st["rate"], 4)))
    assert not fails, f"{shape} M {M} [{dt}]: " + "; ".join(fails)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_tile_choice_at_a_batch_that_fills_the_chip(dt):
    """M = 8 x 1024 image rows: the three wide shapes on the 128 x 128 tile, and the widths of the existing MMDiT plans (1536: output
    projection / FF2 with their epilogue reads, 4608: QKV) and of the UNet (1280) where they were."""
    M = 8192
    want = {(2432, 2432, True): ("dma", 4, 2, 2, 0), (2432, 9728, True): ("dma", 4, 2, 2, 0), (7296, 2432, False): ("dma", 4, 2, 2, 0),
            (1536, 1536, False): ("dma", 8, 4, 2, 0), (1536, 6144, True): ("dma", 8, 4, 2, 0), (4608, 1536, False): ("dma", 8, 4, 2, 0),
            (1280, 1280, False): ("dma", 5, 2, 2, 0)}
    got = {}
    for (N, K, gated) in want:
        a = torch.zeros(M, K, dtype=dt, device="cuda")
        w = torch.zeros(N, K, dtype=dt, device="cuda")
        gate = torch.zeros(8, N, device="cuda") if gated else None
        res = torch.zeros(M, N, dtype=dt, device="cuda") if gated else None
        ops.gemm(a, w, bias=torch.zeros(N, device="cuda"), rowgate=gate, residual=res, rows_per_batch=1024 if gated else 0)
        got[(N, K, gated)] = X.launch_key(_last_launch())
    torch.cuda.synchronize()
    assert got == want
