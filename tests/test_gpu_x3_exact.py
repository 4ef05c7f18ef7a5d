"""The fp32-storage GEMM forms -- the contractions of the precise plans (precision="bf16x3", dtype=torch.float32) -- element by
element against float64 arithmetic (criterion: tests_support/exact.py, "fp32-storage GEMM forms"):

  x3t   the triple-operand path: sdn_gemm_bf16 on [hi | lo | hi] rows and [hi | hi | lo] weights (K' = 3K) with the x3_out
        epilogues 1 (f32 rows), 2 (GEGLU triple), 3 (triple), 4 (hi | lo pair rows) and 0 + NCHW (conv_out); the instantiation is
        asserted through sdn_debug_gemm_last_launch and the last test asserts that every reachable one ran;
  x3    sdn_gemm_x3 = k_gemm_x3<CONV, XNJ> for M >= 64 (operands split in the kernel, every load clamped), k_gemm_f32 below;
  f32   sdn_gemm_f32 = k_gemm_f32 (f32-input MFMA).

The bf16x3 product is a defined function of the split operands, so each kernel is held to ACCUMULATION error against
y3 = Ahi Whi^T + Alo Whi^T + Ahi Wlo^T, not to the 2^-16 of the scheme (that bound is tests/test_exact_checker.py's).  Triple and
pair outputs must be, bit for bit, the split of the f32 result of the same operands.

Outputs are views into NaN-sentinel buffers (before, after, every ldc gap).  The operands of the clamped-load kernels sit in
exact-size allocations bracketed by NaN rows; triples, residuals and row biases carry NaN tails (and NaN ldc gaps)."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import safe_denoiser_amd as sda
from tests_support import exact as X
from tests_support import ops

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
_SEEN = set()                 # (family, instantiation / kernel) of every case that ran and passed
_STATS = []                   # per-case statistics (written to $SDN_EXACT_STATS when set)


def _last_launch():
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    return list(rec)


def _r(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _binade_rows(a):
    """Rows scaled by 2^(i % 40 - 26): hi and lo span 40 binades, everything stays normal in bf16 (lo >= ~2^-45)."""
    return a * torch.exp2(torch.arange(a.shape[0], dtype=F32, device=a.device) % 40 - 26.0)[:, None]


def _judge(name, family, inst, out, buf, y, s, e, *, value=None):
    """Bound, NaN and guard-band verdict of one launch; records the case.  value: what to compare instead of out (hi + lo)."""
    torch.cuda.synchronize()
    bad = X.sentinels_intact(buf, out)
    st = X.analyse(out if value is None else value, y, s, e, dtype=F32, acc=X.X3_ACC[family])
    fails = X.failures(st, exact_fn=False, direction=False)  # (f32 outputs: no 16-bit rounding to judge, exact.py)
    if bad:
        fails.append(f"{bad} guard-band sentinels overwritten")
    row = dict(case=name, family=family, inst="/".join(map(str, inst)), n=st["n"], max_err_over_bound=round(st["max_err_over_tol"], 3),
               log2_err_over_S=round(math.log2(max(st["err_over_s"], 1e-300)), 2))
    _STATS.append(row)
    print(row)
    return [f"{name} [{family}] on {inst}: " + "; ".join(fails)] if fails else []


def _conv_geometry(conv):
    H, stride, ups, asym = conv["H"], conv.get("stride", 1), conv.get("upsample", 0), conv.get("asym_pad", 0)
    Ho = ((2 * H if ups else H) + (1 if asym else 2) - 3) // stride + 1
    return dict(Hs=H, Ws=H, Cin=conv.get("Cin", 64), Ho=Ho, Wo=Ho, stride=stride, upsample=ups, asym_pad=asym), conv["B"] * Ho * Ho, Ho * Ho


def _epilogue_operands(g, M, N, width, ldc, rpb, *, bias, rowbias, rowgate, residual, residual_bcast):
    bv = torch.randn(N, generator=g).cuda() if bias else None
    nb = (M + rpb - 1) // rpb if rpb else 0
    rb = X.with_nan_tail(_r(g, nb, N), 4) if rowbias else None
    gt = X.with_nan_tail(_r(g, nb, N, scale=0.5), 4) if rowgate else None
    res = X.nan_strided(_r(g, rpb if residual_bcast else M, width), ldc) if residual else None        # (shares the output's ldc)
    return bv, rb, gt, res


def _shape_output(t, M, rpb, n_valid, out_kind):
    if t is None:
        return None
    if n_valid:
        t = t[:, :n_valid]
    return t.reshape(M // rpb, rpb, -1).permute(0, 2, 1) if out_kind == 2 else t


# ---------------------------------------------------------------------------------------- sdn_gemm_x3 / sdn_gemm_f32 (sdn_f32.hip)
def _kernel_of(entry, M, N, act, conv):
    """gemm_f32_storage's choice, restated: the x3 entry takes k_gemm_x3 iff M >= 64; its tile is the 160-column one (XNJ = 5)
    iff the epilogue is not GEGLU and (N % 160 == 0 or N % 128 != 0), else the 128-column one; everything else is k_gemm_f32.
    Both require K % 64 == 0 and N % 32 == 0 (Cin % 64 == 0 for a conv)."""
    if entry == "x3" and M >= 64:
        return ("k_gemm_x3", conv, 5 if act != 2 and (N % 160 == 0 or N % 128 != 0) else 4)
    return ("k_gemm_f32", conv)


def _f32_case(name, entry, kern, *, N, M=0, K=64, K2=0, conv=None, bias=True, rowbias_rpb=0, rowbias=False, rowgate=False,
              residual=False, residual_bcast=0, act=0, out_kind=0, n_valid=0, ldc_pad=0, scale_rows=False, exact_bf16=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    geo, rpb = None, rowbias_rpb
    if conv:
        geo, M, rpb = _conv_geometry(conv)
        K = 9 * geo["Cin"]
    want = kern if entry == "x3" else ("k_gemm_f32", bool(conv))
    assert _kernel_of(entry, M, N, act, bool(conv)) == want and K % 64 == 0 and K2 % 64 == 0 and N % 32 == 0, (name, entry)
    if conv:
        a = X.bracketed(_r(g, conv["B"] * conv["H"] ** 2, geo["Cin"])).view(conv["B"], conv["H"], conv["H"], geo["Cin"])
    else:
        a = _r(g, M, K)
        a = _binade_rows(a) if scale_rows else a
        a = X.bracketed(a.bfloat16().float() if exact_bf16 else a)
    a2 = X.bracketed(_r(g, M, K2)) if K2 else None
    w = X.bracketed(_r(g, N, K + K2, scale=(2 if act == 2 else 1) * (K + K2) ** -0.5))
    width = N // 2 if act == 2 else (n_valid or N)
    ldc = width + (0 if out_kind == 2 else ldc_pad)
    bv, rb, gt, res = _epilogue_operands(g, M, N, width, ldc, rpb, bias=bias, rowbias=rowbias or (rpb and not rowgate and not conv),
                                         rowgate=rowgate, residual=residual, residual_bcast=residual_bcast)
    if out_kind == 2:
        buf, out = X.guarded_like((M // rpb, width, rpb), F32, "cuda")
    else:
        buf, out = X.guarded(M, width, F32, "cuda", ldc=ldc)
    ops.X3 = entry == "x3"
    try:
        ops.gemm(a, w, bias=bv, rowbias=rb, rowgate=gt, residual=res, residual_bcast=residual_bcast, act=act, out_kind=out_kind,
                 n_valid=n_valid, rows_per_batch=rpb, a2=a2, conv=geo, out=out)
    finally:
        ops.X3 = False
    A, W = X.operands(a, w, a2=a2, conv=geo)
    split = want[0] == "k_gemm_x3"
    if split:                                 # the kernel's own split, reproduced: y3 and S3 over the bf16 planes
        A, W = X.x3_operands(A, W)
    res_n = res if res is None or width == N else torch.nn.functional.pad(res, (0, N - width))   # (columns >= n_valid: never read)
    y, s, e, _ = X.reference_aw(A, W, BF if split else F32, bias=bv, rowbias=rb, rowgate=gt, residual=res_n, residual_bcast=residual_bcast,
                                rpb=rpb, act=act, exact_gelu=True, plain32=False)
    y, s, e = (_shape_output(t, M, rpb, n_valid, out_kind) for t in (y, s, e))
    family = "x3" if split else "f32"
    fails = _judge(name, family, want + (entry,), out, buf, y, s, e)
    if exact_bf16 and split:                  # all lo are zero: the hi-only product, within the same bound
        assert not bool(A[:, A.shape[1] // 3:2 * A.shape[1] // 3].any()), name
    assert not fails, "\n".join(fails)
    _SEEN.add((entry, want))


X5, X4, C5, C4 = ("k_gemm_x3", False, 5), ("k_gemm_x3", False, 4), ("k_gemm_x3", True, 5), ("k_gemm_x3", True, 4)
PLAIN = {
    # name: (kernel the x3 entry takes -- the f32 entry runs k_gemm_f32 on the same case, kwargs)
    "M 197 (2 row tiles, 69 rows valid), N 320 (2 column tiles), K 192": (X5, dict(M=197, N=320, K=192)),
    "M 64 (threshold, clamped tile), N 192 (32-column ragged tile), K 64 (prologue alone)": (X5, dict(M=64, N=192, K=64, ldc_pad=4)),
    "N 256 (128-wide), two-source K1 64 of 192, row bias rpb 77": (X4, dict(M=197, N=256, K=64, K2=128, rowbias_rpb=77)),
    "N 256 GEGLU (128-wide, value / gate pairs), ldc gap": (X4, dict(M=197, N=256, K=192, act=2, ldc_pad=4)),
    "row gate + residual, rpb 77": (X5, dict(M=197, N=320, K=64, rowbias_rpb=77, rowgate=True, residual=True)),
    "row bias + residual_bcast, rpb 77": (X4, dict(M=197, N=256, K=64, rowbias_rpb=77, residual=True, residual_bcast=1)),
    "SiLU after residual, N 192": (X5, dict(M=197, N=192, K=64, act=1, residual=True)),
    "tanh-GELU, N 256": (X4, dict(M=197, N=256, K=192, act=3)),
    "n_valid N - 28 (wide), residual, ldc gap": (X5, dict(M=197, N=320, K=64, n_valid=292, residual=True, ldc_pad=4)),
    "n_valid N - 28 (128-wide)": (X4, dict(M=197, N=256, K=64, n_valid=228)),
    "out_kind 1, M 64": (X5, dict(M=64, N=320, K=192, out_kind=1)),
    "NCHW f32, n_valid 4 of 32, row bias rpb 77": (X5, dict(M=231, N=32, K=64, out_kind=2, rowbias_rpb=77, n_valid=4)),
    "A rows scaled 2^-26 ... 2^13": (X5, dict(M=197, N=320, K=192, bias=False, scale_rows=True)),
    "A exactly representable in bf16 (every lo zero)": (X4, dict(M=197, N=256, K=64, exact_bf16=True)),
}
CONV = {   # Cin = 64 (K = 576)
    "stride 1, B 3 H 8 (M 192), N 320, row bias": (C5, dict(conv=dict(B=3, H=8), N=320, rowbias=True)),
    "B 5 H 4 (map narrower than a fragment, M 80), N 96, residual": (C5, dict(conv=dict(B=5, H=4), N=96, residual=True, ldc_pad=4)),
    "stride 2 symmetric, N 128, row bias + residual": (C4, dict(conv=dict(B=3, H=16, stride=2), N=128, rowbias=True, residual=True)),
    "stride 2 + asym_pad, N 320, residual": (C5, dict(conv=dict(B=2, H=16, stride=2, asym_pad=1), N=320, residual=True)),
    "upsample, N 256, row bias": (C4, dict(conv=dict(B=3, H=4, upsample=1), N=256, rowbias=True)),
    "conv_out: 4 of 32, f32 NCHW": (C5, dict(conv=dict(B=2, H=8), N=32, n_valid=4, out_kind=2)),
}
F1, F1C = ("k_gemm_f32", False), ("k_gemm_f32", True)
SMALL_M = {   # below the x3 entry's threshold: k_gemm_f32 from BOTH entry points
    "M 1": (F1, dict(M=1, N=320, K=192)),
    "M 2, GEGLU": (F1, dict(M=2, N=256, K=64, act=2)),
    "M 63, two-source, row bias rpb 21, residual": (F1, dict(M=63, N=192, K=64, K2=128, rowbias_rpb=21, residual=True)),
    "conv B 3 H 4 (M 48), residual": (F1C, dict(conv=dict(B=3, H=4), N=96, residual=True)),
}


@pytest.mark.parametrize("entry", ["x3", "f32"])
def test_f32_storage_plain_forms_are_exact(entry):
    X.run_all(_f32_case, entry, PLAIN)


@pytest.mark.parametrize("entry", ["x3", "f32"])
def test_f32_storage_conv_forms_are_exact(entry):
    X.run_all(_f32_case, entry, CONV)


@pytest.mark.parametrize("entry", ["x3", "f32"])
def test_small_m_runs_the_f32_kernel_from_both_entry_points(entry):
    X.run_all(_f32_case, entry, SMALL_M)


# ------------------------------------------------------------------------------ the triple-operand path (sdn_gemm_bf16 + x3_out)
def _x3t_case(name, _family, key, *, N, M=0, K=64, K2=0, conv=None, x3_out=1, bias=True, rowbias_rpb=0, rowbias=False, residual=False,
              act=0, out_kind=1, n_valid=0, ldc_pad=0, scale_rows=False, exact_bf16=False, slab=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    geo, rpb = None, rowbias_rpb
    if conv:
        geo, M, rpb = _conv_geometry(conv)
        a = _r(g, conv["B"] * conv["H"] ** 2, geo["Cin"])
        K = 9 * geo["Cin"]
    else:
        a = _r(g, M, K)
        a = _binade_rows(a) if scale_rows else a
        a = a.bfloat16().float() if exact_bf16 else a
    a3 = X.with_nan_tail(ops.split3(a, _r(g, M, K2) if K2 else None), 64)      # two-source: one triple of the concatenation
    if exact_bf16:
        assert not bool(a3[:, K:2 * K].any()), name
    w = _r(g, N, K + K2, scale=(2 if act == 2 else 1) * (K + K2) ** -0.5)
    w3 = ops.expand3(w, group=geo["Cin"] if conv else None)
    geo3 = None
    if conv:
        a3 = a3.view(conv["B"], conv["H"], conv["H"], 3 * geo["Cin"])
        geo3 = dict(geo, Cin=3 * geo["Cin"])
    width = N // 2 if act == 2 else (n_valid or N)
    ldc = width + ldc_pad
    bv, rb, _, res = _epilogue_operands(g, M, N, width, ldc, rpb, bias=bias, rowbias=rowbias or (rpb and not conv), rowgate=False,
                                        residual=residual, residual_bcast=0)
    kw = dict(bias=bv, rowbias=rb, residual=res, conv=geo, act=act, rows_per_batch=rpb)
    y, s, e, _ = X.reference(a3, w3, conv=geo3, bias=bv, rowbias=rb, residual=res, rpb=rpb, act=act, exact_gelu=True, plain32=False)
    fails = []

    def ran(what):
        rec = _last_launch()
        got = X.launch_key(rec)
        assert got == key, f"{name} ({what}): ran {got} (record {rec}), written for {key}"

    if x3_out == 0:                           # conv_out: the 16-bit NCHW f32 form on triple operands
        buf, out = X.guarded_like((M // rpb, width, rpb), F32, "cuda")
        ops.gemm_x3t(a3, w3, N, K + K2, x3_out=0, out_kind=2, n_valid=n_valid, out=out, **kw)
        ran("NCHW")
        fails += _judge(name, "x3t", key, out, buf, *(_shape_output(t, M, rpb, n_valid, 2) for t in (y, s, e)))
    elif x3_out == 2:                         # GEGLU has no f32-row form on this path: hi + lo against the exact value
        buf, out = X.guarded_planes(M, 3, width, BF, "cuda", ldc=ldc)
        ops.gemm_x3t(a3, w3, N, K + K2, x3_out=2, out=out, ldc=ldc, **kw)
        ran("GEGLU triple")
        fails += _judge(name, "x3t", key, out, buf, y, s, e + X.PAIR_REL * y.abs(), value=out[:, 0].double() + out[:, 1].double())
        if not torch.equal(out[:, 0].contiguous().view(torch.int16), out[:, 2].contiguous().view(torch.int16)):
            fails.append(f"{name}: the two hi planes of the GEGLU triple differ")
    else:
        if slab:
            sda.lib().sdn_debug_gemm_launch_counts(None, 1)
        fbuf, f = X.guarded(M, width, F32, "cuda", ldc=ldc)
        ops.gemm_x3t(a3, w3, N, K + K2, x3_out=1, out=f, ldc=ldc, **kw)
        ran("f32 rows")
        if slab:                              # not vacuous: the slab kernel took it
            cnt = (C.c_longlong * 2)()
            sda.lib().sdn_debug_gemm_launch_counts(cnt, 0)
            assert cnt[0] == 1 and cnt[1] == 0, (name, list(cnt))
        fails += _judge(name, "x3t", key, f, fbuf, y, s, e)
        if x3_out in (3, 4):
            planes = 3 if x3_out == 3 else 2
            buf, out = X.guarded_planes(M, planes, width, BF, "cuda", ldc=ldc)
            ops.gemm_x3t(a3, w3, N, K + K2, x3_out=x3_out, out=out, ldc=ldc, **kw)
            ran("triple" if planes == 3 else "pairs")
            torch.cuda.synchronize()
            bad = X.check_split_planes(out, f, planes)
            if X.sentinels_intact(buf, out):
                bad.append(f"{X.sentinels_intact(buf, out)} guard-band sentinels overwritten")
            if bool(torch.isnan(out.float()).any()):
                bad.append(f"{int(torch.isnan(out.float()).sum())} NaN outputs")
            fails += [f"{name} (x3_out {x3_out}) on {key}: " + "; ".join(bad)] if bad else []
    assert not fails, "\n".join(fails)
    _SEEN.add(("x3t", key))


D = ("dma",)
TRIPLE = {
    # small M: pick_tile falls back to the 64-wide tile (N % 64 == 0) or the 32-wide one; logical K 64 ... 192, K' = 3K
    "f32 rows, M 197, N 320, K 192, bias + row bias rpb 77 + f32 residual": (D + (2, 2, 2, 0), dict(M=197, N=320, K=192, rowbias_rpb=77, residual=True, ldc_pad=4)),
    "triple, N 192, K 64, ldc gap": (D + (2, 2, 2, 0), dict(M=197, N=192, K=64, x3_out=3, ldc_pad=4)),
    "pairs, N 256, K 64, residual": (D + (2, 2, 2, 0), dict(M=197, N=256, K=64, x3_out=4, residual=True)),
    "GEGLU triple, N 256, K 192": (D + (2, 2, 2, 0), dict(M=197, N=256, K=192, x3_out=2, act=2, ldc_pad=4)),
    "two-source split3(a1, a2), K1 64 of 192, N 32": (D + (1, 2, 2, 0), dict(M=197, N=32, K=64, K2=128)),
    "triple, N 96, row bias + residual": (D + (1, 2, 2, 0), dict(M=64, N=96, K=64, x3_out=3, rowbias_rpb=21, residual=True)),
    "A rows scaled 2^-26 ... 2^13": (D + (2, 2, 2, 0), dict(M=197, N=320, K=64, bias=False, scale_rows=True, x3_out=3)),
    "A exactly representable in bf16 (every lo zero), pairs": (D + (2, 2, 2, 0), dict(M=197, N=256, K=64, exact_bf16=True, x3_out=4)),
    # conv, logical Cin 64 (K' = 1728)
    "conv stride 1, B 3 H 8, N 320, row bias + residual": (D + (2, 2, 2, 0), dict(conv=dict(B=3, H=8), N=320, rowbias=True, residual=True)),
    "conv B 5 H 4 (map narrower than a fragment), N 96, triple": (D + (1, 2, 2, 0), dict(conv=dict(B=5, H=4), N=96, x3_out=3, ldc_pad=4)),
    "conv stride 2 symmetric, N 128, pairs": (D + (2, 2, 2, 0), dict(conv=dict(B=3, H=16, stride=2), N=128, x3_out=4, rowbias=True)),
    "conv stride 2 + asym_pad, N 320, residual": (D + (2, 2, 2, 0), dict(conv=dict(B=2, H=16, stride=2, asym_pad=1), N=320, residual=True)),
    "conv upsample, N 256, triple": (D + (2, 2, 2, 0), dict(conv=dict(B=3, H=4, upsample=1), N=256, x3_out=3, residual=True)),
    "conv_out: x3_out 0, 4 of 32, f32 NCHW": (D + (1, 2, 2, 0), dict(conv=dict(B=2, H=8), N=32, x3_out=0, n_valid=4)),
}
TRIPLE_TILES = {
    # the wider tiles need >= 256 tiles of 128 rows (pick_tile), the 256-row ones >= 192 tiles and K' >= 320 (short_ok), i.e.
    # M > 191 * 256 at one n-tile: the smallest M that reaches them at K' = 3K
    "258 tiles of 128 x 160, tail 19, triple + residual": (D + (5, 2, 2, 0), dict(M=128 * 128 + 19, N=320, K=64, x3_out=3, residual=True)),
    "256 tiles, K' 576: deep ring, tail 69, row bias": (D + (5, 2, 4, 0), dict(M=128 * 128 - 59, N=320, K=192, rowbias_rpb=333)),
    "258 tiles of 128 x 128, tail 37, pairs": (D + (4, 2, 2, 0), dict(M=85 * 128 + 37, N=384, K=64, x3_out=4)),
    "256 tiles of 128 x 128, GEGLU triple, tail 19": (D + (4, 2, 2, 0), dict(M=127 * 128 + 19, N=256, K=64, x3_out=2, act=2)),
    "192 tiles of 256 x 320, tail 19, row bias + residual": (D + (10, 4, 2, 0), dict(M=191 * 256 + 19, N=320, K=128, rowbias_rpb=333, residual=True)),
    "192 tiles of 256 x 256, tail 37, triple": (D + (8, 4, 2, 0), dict(M=191 * 256 + 37, N=256, K=128, x3_out=3)),
}
SLAB = {
    "slab ring W = 32, logical Cin 64, row bias + f32 residual": (("slab",), dict(conv=dict(B=48, H=32), N=320, rowbias=True, residual=True, slab=True)),
}


def test_triple_path_small_tiles_and_conv_forms_are_exact():
    X.run_all(_x3t_case, "x3t", TRIPLE)


def test_triple_path_wide_and_256_row_tiles_are_exact():
    X.run_all(_x3t_case, "x3t", TRIPLE_TILES)


def test_triple_path_slab_ring_conv_is_exact():
    X.run_all(_x3t_case, "x3t", SLAB)


def test_every_listed_instantiation_ran():
    """The cases above covered exactly the instantiations tests_support/exact.py lists for the fp32-storage forms: the triple
    path's (by launch record), every k_gemm_x3 template and k_gemm_f32 from the x3 entry, k_gemm_f32 from its own."""
    want = ({("x3t", k) for k in X.X3T_INSTANTIATIONS} | {("x3", k) for k in X.X3_KERNELS}
            | {("f32", k) for k in X.X3_KERNELS if k[0] == "k_gemm_f32"})
    if os.environ.get("SDN_EXACT_STATS"):                 # per-case table: worst error over the bound and over S
        with open(os.environ["SDN_EXACT_STATS"], "w") as f:
            json.dump(_STATS, f, indent=0)
    assert _SEEN == want, dict(missing=sorted(map(str, want - _SEEN)), unexpected=sorted(map(str, _SEEN - want)))
