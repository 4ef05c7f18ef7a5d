"""Element-exact criterion for the 16-bit GEMM family: a kernel's output against float64 arithmetic on the SAME 16-bit operands.

For every output element with exact value y (float64 GEMM + exact epilogue), the kernel's stored value must satisfy

    |out - y| <= 1/2 ulp_T(y) + ACC * S' + E_epi

  ulp_T(y)  spacing of the output type T at |y| (subnormal range included; for f32 outputs T = float32).
  S'        the magnitude the fp32 arithmetic works at: S = sum_k |a_k| |w_k| (+ |bias| + |rowbias|) (x |gate|) (+ |residual|),
            computed in float64 like y; through an activation f it is carried as max|f'| S (GELU, SiLU: <= 1.13), through
            GEGLU h * gelu(g) as S_h |gelu(g)| + 1.13 |h| S_g.
  ACC       = 2^-20 per unit of S'.  Measured on MI355X: the f32 outputs of the matrix (out_kind 1 and 2, no 16-bit rounding,
            K = 128 ... 576, both dtypes) lie within 2^-22.2 S of y, and fp16 probes at K = 64 / 256 with normal operands within
            2^-22.5 S (tests/test_gpu_gemm_exact.py records |out - y| / S per case as log2_err_over_S).  A plain fp32 dot product
            of K terms has a worst-case bound of K 2^-24 S and a random-walk size of sqrt(K) 2^-24 S (2^-18.4 / 2^-21.5 S at
            K = 2304).  2^-20 is 4.6x the measured worst and covers the few fp32 roundings of the epilogue (bias, row bias, gate,
            residual: each <= 2^-24 S).  An instantiation that needs more is a finding, not a constant to raise.
  E_epi     the documented error of an approximate activation (csrc/sdn_gemm_common.h):
              GEGLU  gelu_erf (quintic-argument logistic): |gelu_erf(g) - GELU(g)| <= 2.6e-5 absolute (the comment's figure;
                     a float32 emulation of its 9 instructions over |g| <= 12 in steps of 1.2e-5 peaks at 2.55e-5 near g = 3.07),
                     so E_epi = 2.6e-5 |h|.
              tanh-GELU and SiLU evaluate their exact formulas with v_exp_f32 / v_rcp_f32 (<= 1 ulp each) or __expf:
                     float32 emulation peaks at 1.2e-7 |x|; E_epi = 2^-20 |x| (8x that) -- and they are not approximations
                     of another function, so they also join the rounding-direction statistic.
  E_sub     fp16 subnormal operands: the MFMA's result carries an ABSOLUTE error of up to 2^-36 when an operand is
            subnormal (measured: fp16 rows of N(0, 1) 2^-24 ... 2^-20 -- mostly subnormals -- at K = 64 / 256 give |out - y| up to
            2^-36.1 ... 2^-35.9 on f32 outputs, where the SAME products from operands scaled by 2^20, all normal, stay within
            2^-44 ... 2^-38 = 2^-23 S; with normal operands the floor does not appear).  So each element whose A row or W row
            holds a subnormal gets E_sub = 2^-35 on top (1/2^11 of an fp16 subnormal ulp: it matters only to exact ties), carried
            in S' as E_sub / ACC so that it passes through the epilogue like the accumulation error it is.
  LayerNorm fold   the folded operands (w', c, d of sdn_ln_fold) are the GEMM's operands; mean / rstd are exact float64
                   statistics of x, and S = rstd (sum_k |x_k| |w'_k| + |mean| |c|) + |d|.

Also, per case:
  overflow        where RN_T(y) = +-inf (fp16 |y| >= 65520) the output is that inf; no NaN for finite inputs.
  direction       |mean(sign(y) (out - y) / ulp_T(y))| <= 0.02 (round toward zero gives ~ -0.25), over the elements whose
                  non-rounding budget ACC S' + E_epi is below 1/16 ulp_T(y) -- where the storage rounding decides the error --
                  when there are >= 10^5 of them.  Not for GEGLU: its quintic GELU errs systematically by up to 1/3 of an fp16
                  half-ulp (sdn_gemm_common.h), so the mean would measure the approximation, not the rounding.  Not for f32
                  outputs: no 16-bit rounding to judge.
  rounding rate   for exact-function epilogues (none, bias, residual, row bias, row gate, SiLU) the fraction of elements
                  with out == RN_T(y) >= that of a plain torch fp32 GEMM on the same operands (rounded once to T) minus 0.01
                  (double rounding drops it to ~0.75).  f32 outputs: the rate is recorded, not asserted -- with no 16-bit
                  rounding it measures the MFMA's internal accumulation against hipBLASLt's (measured: bf16 MFMA chains sit
                  ~8 f32 ulps toward zero on average at K = 576, 0.19 exact vs torch's 0.46), all of it inside the ACC S bound.

Guard bands: outputs are views into larger buffers filled with a NaN bit pattern (before, after and in the ldc gap); the
pattern must survive bit for bit.  Inputs carry NaN rows past their valid extent, so a stray read poisons a checked value.

fp32-storage GEMM forms (the contractions of the precise plans; tests/test_gpu_x3_exact.py).  The bf16x3 product is a defined
function of the split operands, so the kernels are held to ACCUMULATION error, not to the 2^-16 of the scheme:

    |out - y3| <= 1/2 ulp_f32(y3) + X3_ACC[family] * S3 + E_epi

  x3t   triple-operand path (sdn_gemm_bf16 with x3_out over [hi | lo | hi] rows and [hi | hi | lo] weights, K' = 3K): the kernel's
        inputs ARE the bf16 triples (ops.split3 / ops.expand3), y3 = A3 . W3^T in float64 over those values, S3 = |A3| . |W3|^T
        (+ |bias| + |rowbias| + |residual|).
  x3    sdn_gemm_x3 (k_gemm_x3: operands split in the kernel): hi = RNE_bf16(x), lo = RNE_bf16(x - hi) reproduced on the host
        (x3_operands), y3 = Ahi Whi^T + Alo Whi^T + Ahi Wlo^T, S3 the same three terms of absolute values.
  f32   sdn_gemm_f32 (k_gemm_f32, also the M < 64 fallback of the x3 entry): y = A . W^T of the f32 operands, S = |A| . |W|^T.
  E_epi SiLU / tanh-GELU as above (ACT_REL |x|); GEGLU on these paths evaluates an erf (erff, or Abramowitz-Stegun 7.1.26 with
        |error| <= 1.5e-7), not the quintic: E_epi = ACT_REL |h|, no 2.6e-5 term.
  Triple (x3_out 3) and pair (x3_out 4) outputs: bit equality with the split of the checked f32-row result (x3_out 1) of the same
        operands -- hi == bf16(f), lo == bf16(f - hi), third plane == hi.  The GEGLU triple (x3_out 2) has no f32-row form on that
        path: hi + lo is held to ACC S' + E_epi + 2^-16 |y| (PAIR_REL: what a hi | lo pair can carry) and its two hi planes to
        bit equality.
  X3_ACC  starts from ACC = 2^-20, which was measured on 16-bit chains; the derivable hard bound of a K'-term fp32 chain is
        K' 2^-24 S (2^-16.4 at K' = 192, 2^-13.2 at the slab case's K' = 1728).  Measured on MI355X, normal operands
        (profiles/x3_exact.json, log2_err_over_S per case; worst per family): k_gemm_x3 2^-22.4 S3 (K' = 192 ... 1728), k_gemm_f32's f32-input MFMA 2^-21.7 S (K = 64 ... 576),
        the triple path 2^-21.0 S3 on the plain tiles (K' = 192 ... 1728) and 2^-20.7 S3 on the slab ring at K' = 1728 (15.7 M
        elements; 0.6 of the whole bound there, the closest any case comes).  No family exceeds 2^-20 S, so all three keep
        X3_ACC = ACC = 2^-20 unchanged: a margin of 5.3x / 3.3x / 1.6x over the measured worst (2^-20 is 1/12 of
        the hard bound at K' = 192, 1/110 at K' = 1728).  (The GEGLU triple's hi + lo sits at 2^-19.1 S': that is the 2^-16 |y| of the pair, not accumulation.)  A
        family that comes to need more gets its own constant of 4x its measured worst, below K' 2^-24, stated here with the
        measurement; a value above the hard bound is a bug to find.
  The scheme itself, |y3 - y| <= 3 * 2^-16 S (SCHEME_REL), is pinned on the CPU (tests/test_exact_checker.py); the operator-level
  3e-5 rel-L2 bounds of tests/test_gpu_f32.py and tests/test_gpu_x3t.py rest on it.
  Clamped loads: k_gemm_x3 fetches rows past M / N from the last valid row instead of predicating, so its A and W operands live
  in exact-size allocations bracketed by NaN rows (bracketed): one row past the clamp poisons a checked value.

Normalisation kernels (GroupNorm, LayerNorm, adaLN, row statistics; tests/test_gpu_norm_exact.py).  y = (x - mu) r g + b with
mu, v the exact population mean / variance of the normalised set, r = (v + eps)^-1/2, g = gamma (1 + scale for adaLN), b = beta
(shift), all in float64 on the 16-bit or f32 values the kernel reads.  For every element

    |out - f(y)| <= 1/2 ulp_T(f(y)) + ARITH S + STAT Q          (f = identity or SiLU, carried as apply_act(..., 1) does)
    S = |g| r (|x| + |mu|) + |b|
    Q = |g| r (m1 + |x - mu| M2 / (2 (v + eps)))

  m1      mean |x| over the set: a statistics error of STAT m1 in the mean moves y by |g| r STAT m1.
  M2      mean x^2 over the set for the kernels that form E[x^2] - mean^2 (both statistic sources of the 16-bit GroupNorm, the
          three f32 GroupNorm forms), v for the kernels that sum centred squares (every LayerNorm form, k_row_stats): an error
          of STAT M2 in the variance moves r by r STAT M2 / (2 (v + eps)).  Q therefore GROWS with M2 / v = 1 + (mean / std)^2:
          that is the price of the one-pass variance, and the cancellation cases put a number on it.
  ARITH   derived, NORM_ARITH[family] = (fp32 roundings between the statistics and the stored value) x 2^-24, each rounding taken
          as <= 2^-24 S and rsqrtf / (1 / sqrt) as 2 of them:
            gn16     k_gn_apply: a = rstd gamma, mean a, beta - mean a, fmaf(x, a, cb): 4, + rsqrtf 2               = 6
            ln16     k_layernorm: x - mean, . rstd, . gamma, + beta: 4, + rsqrtf 2                                   = 6
            ln16mod  the same with 1 + scale formed first: 5, + rsqrtf 2                                             = 7
            gnf32    k_gn_rows_apply / k_groupnorm_f32 / _any: x - mean, . rstd, . gamma, + beta: 4; (float) mean and
                     (float)(1 / sqrt(double)) one rounding each                                                     = 6
            lnf32    k_layernorm_f32_regs / k_layernorm_f32: 4, + 1.0f / sqrtf 2                                     = 6
            lnf32mod k_layernorm_mod_f32: 5, + 1.0f / sqrtf 2                                                        = 7
          None needs more than 8 (2^-21).  SiLU adds apply_act's GELU_D and ACT_REL |y| on top, as in the GEMM epilogues.
  STAT    measured per family against the float64 statistics -- on stats_ws[b][g] = (mean, rstd) after sdn_groupnorm_* /
          sdn_groupnorm_cols_*, on the output of sdn_row_stats_* (the reduction code of k_layernorm), and for the f32 forms, which
          expose no statistics, on their f32 outputs (what of |out - y| is left after 1/2 ulp + ARITH S, per unit of Q) -- as the
          worst |mean_out - mu| / m1 and |rstd_out - r| / (r M2 / (2 (v + eps))) over the cases; the constant is 4x that worst
          (the margin of X3_ACC), and must stay below the hard bound (family's longest serial fp32 chain) x 2^-24:
            family      measured worst (MI355X, profiles/norm_exact.json)          constant      longest chain -> hard bound
            gn16        0.507 x 2^-20  rstd, |mean| / std 100 at hw 4097 (fp16)     2.03 x 2^-20  268 (C 1928, G 8: 241 + 17 + ...)  2^-15.9
            gn16serial  3.913 x 2^-20  rstd, hw 100, C 64, G 1 (bf16)               15.65 x 2^-20 2059 (rt x cpg = 32 x 64 = 2048)   2^-13.0
            gn16cols    0.238 x 2^-20  rstd, hw 384, 320 + 640 (fp16)               0.95 x 2^-20  140 (128 rows per partial + 12)    2^-16.9
            ln16        0.426 x 2^-20  rstd, C 1536 with a common offset of 40      1.70 x 2^-20  39 (4 x 8 + 6 + 1)                 2^-18.7
            gnf32       0  (every f32 output within 1/2 ulp + ARITH S)              2^-24         2 (mean, rstd rounded once each)   2^-23
            lnf32       0.001 x 2^-20  k_layernorm_mod_f32, C 1024                  2^-24         39 (C 1538 / 64 + 6 + 1 ...)       2^-18.7
          mean errors are far smaller throughout (<= 0.174 x 2^-20 m1).  The two f32 families measure nothing above a single
          rounding, so their constant is floored at the 2^-24 of rounding a statistic to f32.  gn16serial is ONE shape: k_gn_stats
          lets one thread per group add the group's rt x cpg LDS partials in a serial chain, 2048 terms at C = 64, G = 1 against
          <= 241 for every other tested shape and <= 80 for the shapes the models run; its statistics are 7x less accurate -- inside
          the hard bound, so a constant and not a bug by this criterion's own rule, but recorded as a finding (norm_cases.GN16_CASES).
          A value above the hard bound is a bug to find, not a constant to raise.
  The statistics themselves are asserted: |mean_out - mu| <= 1/2 ulp_f32(mu) + STAT m1 and |rstd_out - r| <= 1/2 ulp_f32(r) +
  STAT r M2 / (2 (v + eps)) (rsqrtf's own error is part of what STAT measures; where M2 / (2 (v + eps)) < 1/4 -- an all-zero group of
  a probe input -- the term is floored at rsqrtf's 2 ulp, 2^-22 r, which it would otherwise leave no room for).  Triple outputs (*_f32_triple) are held to bit equality with the split of the
  checked f32 output of the same inputs (check_split_planes).
  Clean share: in every case not named a cancellation case at least 98 % of the elements have ARITH S + STAT Q <= 1/4 ulp_T(y),
  i.e. the storage rounding decides -- the bound is not hiding a failure behind its own slack (16-bit outputs only; for f32
  outputs the constants' distance to the hard bounds is the control).
  Clamped loads: k_layernorm, k_row_stats and k_gn_stats fetch tail rows from the last valid row, so their inputs carry NaN rows
  right behind the valid extent (with_nan_tail): one row past the clamp poisons a checked value.
"""
import math

import torch
import torch.nn.functional as F

ACC = 2.0 ** -20
GELU_D = 1.13                  # max |d/dx| of GELU (erf or tanh form) and SiLU (1.0998)
GEGLU_ABS = 2.6e-5             # |gelu_erf - GELU| (sdn_gemm_common.h)
ACT_REL = 2.0 ** -20           # tanh-GELU / SiLU evaluation error per unit |x|
DIRECTION_MAX = 0.02
RATE_SLACK = 0.01
MIN_DIRECTION_ELEMS = 100_000
SUBNORMAL_ABS = 2.0 ** -35     # E_sub

_FMT = {torch.float16: (10, -14, 65504.0), torch.bfloat16: (7, -126, float.fromhex("0x1.fep127")),
        torch.float32: (23, -126, float.fromhex("0x1.fffffep127"))}


def ulp(y: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at |y| (float64), subnormals included."""
    mant, emin, _ = _FMT[dtype]
    _, ex = torch.frexp(y.abs())
    e = torch.clamp(ex.to(torch.float64) - 1, min=emin)
    return torch.exp2(e - mant)


def round_to(y: torch.Tensor, dtype) -> torch.Tensor:
    """RN_T(y) in float64 (ties to even, +-inf past the largest finite value) -- one rounding, no detour through float32."""
    _, _, vmax = _FMT[dtype]
    u = ulp(y, dtype)
    r = torch.round(y / u) * u                 # torch.round: half to even
    return torch.where(r.abs() > vmax, torch.copysign(torch.full_like(r, math.inf), y), r)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def silu64(x):
    return x * torch.sigmoid(x)


def subnormal_term(A: torch.Tensor, W: torch.Tensor, dtype) -> torch.Tensor:
    """E_sub [M, N] for the operands A [M, K], W [N, K] (float64 copies of the 16-bit values)."""
    tiny = 2.0 ** _FMT[dtype][1]
    sub = lambda t: ((t != 0) & (t.abs() < tiny)).any(1).to(torch.float64)
    return SUBNORMAL_ABS * torch.clamp(sub(A)[:, None] + sub(W)[None, :], max=1.0)


def apply_act(y, s, act, exact_gelu=False):
    """Exact activation of the float64 pre-activation y with magnitude s: (value, S', E_epi).  act codes as sdn_gemm_desc.
    exact_gelu: the GEGLU gate is evaluated with an erf (the fp32-storage paths), not the quintic: E_epi = ACT_REL |h|."""
    zero = torch.zeros_like(y)
    if act == 0:
        return y, s, zero
    if act == 1:
        return silu64(y), GELU_D * s, ACT_REL * y.abs()
    if act == 3:
        return gelu_tanh64(y), GELU_D * s, ACT_REL * y.abs()
    if act == 2:                               # GEGLU: 16-column value / gate blocks interleaved (unet._interleave16)
        M, N = y.shape
        h, g = y.view(M, N // 32, 2, 16).unbind(2)
        sh, sg = s.view(M, N // 32, 2, 16).unbind(2)
        gg = gelu64(g)
        v = (h * gg).reshape(M, N // 2)
        sp = (sh * gg.abs() + GELU_D * h.abs() * sg).reshape(M, N // 2)
        return v, sp, ((ACT_REL if exact_gelu else GEGLU_ABS) * h.abs()).reshape(M, N // 2)
    raise ValueError(act)


def analyse(out: torch.Tensor, y: torch.Tensor, s: torch.Tensor, e_epi=None, dtype=None, acc=None) -> dict:
    """Statistics of out (any float dtype, the kernel's output) against the exact y (float64) with magnitude s.
    acc: the accumulation constant per unit of S' (default ACC; the fp32-storage families pass theirs, X3_ACC)."""
    acc = ACC if acc is None else acc
    dtype = dtype or out.dtype
    o = out.to(torch.float64)
    y = y.to(torch.float64)
    u = ulp(y, dtype)
    rn = round_to(y, dtype)
    tol = 0.5 * u + acc * s + (0 if e_epi is None else e_epi)
    fin_rn = torch.isfinite(rn)
    nan = torch.isnan(o)
    # overflow: required where y shrunk by the non-rounding budget still rounds to inf, allowed where y grown by it does
    slack = tol - 0.5 * u
    lo_inf = ~torch.isfinite(round_to(y - torch.sign(y) * torch.minimum(slack, y.abs()), dtype))
    hi_inf = ~torch.isfinite(round_to(y + torch.sign(y) * slack, dtype))
    oinf = torch.isinf(o)
    bad_inf = (lo_inf & ~(oinf & (torch.sign(o) == torch.sign(y)))) | (oinf & ~(hi_inf & (torch.sign(o) == torch.sign(y))))
    finite = torch.isfinite(o) & fin_rn
    err = torch.where(finite, (o - y).abs(), torch.zeros_like(y))
    over = finite & (err > tol)
    ulps = torch.where(finite, err / u, torch.zeros_like(y))
    # direction: over the elements whose non-rounding budget (ACC S' + E_epi) is below 1/16 ulp, i.e. where the storage rounding
    # decides the error (near-cancellations, whose |y| is far below S, would otherwise dominate the mean with accumulation noise)
    clean = finite & (tol - 0.5 * u <= u / 16)
    dirv = torch.where(clean, torch.sign(y) * (o - y) / u, torch.zeros_like(y))
    n_dir = int(clean.sum())
    n_fin = int(finite.sum())
    worst = int(torch.argmax(torch.where(over, err / tol, torch.zeros_like(y)).flatten())) if bool(over.any()) else -1
    return dict(n=o.numel(), nan=int(nan.sum()), bad_inf=int(bad_inf.sum()), over=int(over.sum()),
                max_ulp=float(ulps.max()) if o.numel() else 0.0,
                max_err_over_tol=float((err / tol)[finite].max()) if n_fin else 0.0,
                direction=float(dirv.sum()) / max(n_dir, 1), n_dir=n_dir, rate=float((finite & (o == rn)).sum()) / max(n_fin, 1),
                err_over_s=float((err / s.clamp_min(1e-300))[finite].max()) if n_fin else 0.0,
                worst=worst, worst_out=float(o.flatten()[worst]) if worst >= 0 else None,
                worst_ref=float(y.flatten()[worst]) if worst >= 0 else None)


def failures(st: dict, *, exact_fn: bool, ref_rate=None, direction=True) -> list:
    """The criterion's verdict on analyse()'s statistics: a list of what failed (empty = pass)."""
    f = []
    if st["nan"]:
        f.append(f"{st['nan']} NaN outputs")
    if st["bad_inf"]:
        f.append(f"{st['bad_inf']} outputs with the wrong overflow behaviour")
    if st["over"]:
        f.append(f"{st['over']} elements outside the bound (worst {st['max_err_over_tol']:.3g} x the bound at flat index "
                 f"{st['worst']}: out {st['worst_out']!r}, exact {st['worst_ref']!r})")
    if direction and st["n_dir"] >= MIN_DIRECTION_ELEMS and abs(st["direction"]) > DIRECTION_MAX:
        f.append(f"rounding-direction statistic {st['direction']:+.4f} (|.| must be <= {DIRECTION_MAX})")
    if exact_fn and ref_rate is not None and st["rate"] < ref_rate - RATE_SLACK:
        f.append(f"exact-rounding rate {st['rate']:.4f} < torch fp32's {ref_rate:.4f} - {RATE_SLACK}")
    return f


def ref_rate(y32: torch.Tensor, y: torch.Tensor, dtype) -> float:
    """Exact-rounding rate of a plain fp32 computation y32 (rounded once to dtype) against the exact y."""
    r = y32.to(dtype).to(torch.float64)
    rn = round_to(y.to(torch.float64), dtype)
    fin = torch.isfinite(rn)
    return float((fin & (r == rn)).sum()) / max(int(fin.sum()), 1)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------
SENTINEL_BITS = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FDADADA}   # quiet NaNs, distinctive payloads


def _int_view(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sent_value(dtype):
    bits, width = SENTINEL_BITS[dtype], 8 * torch.empty((), dtype=dtype).element_size()
    return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def sentinel_fill(t: torch.Tensor) -> torch.Tensor:
    """Fills t (16- or 32-bit floats) with its dtype's sentinel NaN pattern, in place."""
    _int_view(t).fill_(_sent_value(t.dtype))
    return t


def guarded(rows: int, width: int, dtype, device, *, ldc=None, pad=256):
    """(buffer, view): view [rows, width] with row stride ldc (>= width) inside a flat buffer of the sentinel NaN, with `pad`
    elements before and after.  pad keeps 16-byte alignment for 16- and 32-bit elements when it is a multiple of 8."""
    ldc = ldc or width
    buf = sentinel_fill(torch.empty(2 * pad + rows * ldc, dtype=dtype, device=device))
    return buf, buf[pad:pad + rows * ldc].view(rows, ldc)[:, :width]


def guarded_planes(rows: int, planes: int, width: int, dtype, device, *, ldc=None, pad=256):
    """(buffer, view): view [rows, planes, width] of rows made of `planes` planes of ldc (>= width) elements each -- the bf16
    hi | lo | hi triples (3 planes) and hi | lo pairs (2) of the bf16x3 plan -- inside a sentinel buffer: guards before, after and
    in every plane's ldc gap."""
    ldc = ldc or width
    n = rows * planes * ldc
    buf = sentinel_fill(torch.empty(2 * pad + n, dtype=dtype, device=device))
    return buf, buf[pad:pad + n].view(rows, planes, ldc)[:, :, :width]


def guarded_like(shape, dtype, device, pad=256):
    """(buffer, view) of a contiguous tensor of `shape` between two sentinel bands."""
    n = math.prod(shape)
    buf = sentinel_fill(torch.empty(2 * pad + n, dtype=dtype, device=device))
    return buf, buf[pad:pad + n].view(*shape)


def sentinels_intact(buf: torch.Tensor, view: torch.Tensor) -> int:
    """Number of sentinel elements of buf OUTSIDE view whose bits changed (0 = none)."""
    idx = torch.arange(buf.numel(), device=buf.device)
    off = view.storage_offset() - buf.storage_offset()
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside[idx.as_strided(view.shape, view.stride(), off).flatten()] = True
    return int((_int_view(buf)[~inside] != _sent_value(buf.dtype)).sum())


def bracketed(t: torch.Tensor, rows: int = 8) -> torch.Tensor:
    """Copy of t [R, ...] in an allocation of rows + R + rows rows whose first and last `rows` rows are NaN; returns the [R, ...]
    view.  For operands a kernel fetches with CLAMPED row indices (k_gemm_x3: a row past the end legitimately re-reads the last
    valid row, so zero-fill guard rows say nothing): one row past the clamp, either side, poisons a checked value."""
    buf = torch.full((t.shape[0] + 2 * rows,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    buf[rows:rows + t.shape[0]] = t
    return buf[rows:rows + t.shape[0]]


def nan_strided(t: torch.Tensor, ld: int, extra_rows: int = 64) -> torch.Tensor:
    """Copy of t [R, W] as a view with row stride ld >= W inside a NaN allocation of R + extra_rows rows (a residual that shares
    the output's ldc): the gap columns and the rows past R are NaN."""
    R, W = t.shape
    buf = torch.full((R + extra_rows, ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[:R, :W] = t
    return buf[:R, :W]


def with_nan_tail(t: torch.Tensor, extra_rows: int) -> torch.Tensor:
    """Copy of t [R, ...] in an allocation of R + extra_rows rows whose tail is NaN; returns the [R, ...] view."""
    buf = torch.full((t.shape[0] + extra_rows,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


# ---- the instantiations the 16-bit dispatch can reach (dispatch_dma in csrc/sdn_gemm.hip + the other GEMM-family kernels) --------
# ("dma", NREP, WGM, NSTAGE, LNF); tests/test_exact_checker.py parses dispatch_dma and asserts the "dma" part equals its launch_dma
# list, tests/test_gpu_gemm_exact.py asserts that its cases ran every entry in both dtypes.
INSTANTIATIONS = (
    [("dma", n, w, s, 0) for n, w, s in ((10, 4, 2), (8, 4, 2), (5, 2, 4), (5, 2, 2), (4, 2, 2), (2, 2, 2), (1, 2, 2))]
    + [("dma", n, 4 if n == 10 else 2, 2, 2) for n in (10, 5, 4, 2)]        # LayerNorm fold, pre-pass statistics
    + [("dma", n, 4 if n == 10 else 2, 2, 1) for n in (10, 5, 2)]           # LayerNorm fold, fragment statistics
    + [("slab",), ("splitk",), ("ffn",)])

FAMILY = {1: "dma", 2: "slab", 3: "splitk", 4: "ffn"}


def launch_key(rec) -> tuple:
    """sdn_debug_gemm_last_launch's record -> the INSTANTIATIONS key it ran."""
    fam = FAMILY[rec[0]]
    return ("dma",) + tuple(rec[2:6]) if fam == "dma" else (fam,)


# ---- float64 references shared by the element-exact GPU tests ---------------------------------------------------------------------
F64 = torch.float64


def im2col(x, conv):
    """NHWC map -> float64 [B * Ho * Wo, Cin * 9] (channel-major taps, F.unfold order) of the conv the kernel runs."""
    xc = x.to(F64).permute(0, 3, 1, 2)
    if conv.get("upsample"):
        xc = xc.repeat_interleave(2, 2).repeat_interleave(2, 3)
    xc = F.pad(xc, (0, 1, 0, 1) if conv.get("asym_pad") else (1, 1, 1, 1))
    cols = F.unfold(xc, 3, stride=conv.get("stride", 1))
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def operands(a, w, *, a2=None, conv=None):
    """(A [M, K], W [N, K]) in float64: the matrices of the contraction a GEMM-family call runs (im2col of an NHWC map with the
    weight's taps reordered to match, or the two sources side by side)."""
    if conv:
        N = w.shape[0]
        return im2col(a, conv), w.to(F64).view(N, 3, 3, -1).permute(0, 3, 1, 2).reshape(N, -1)
    return (a.to(F64) if a2 is None else torch.cat([a.to(F64), a2.to(F64)], 1)), w.to(F64)


def split_bf16(x):
    """The in-kernel bf16x3 split of float64-held f32 values: hi = RNE_bf16(x), lo = RNE_bf16(x - hi), both as float64."""
    x32 = x.float()
    hi = x32.bfloat16()
    lo = (x32 - hi.float()).bfloat16()
    return hi.to(F64), lo.to(F64)


def x3_operands(A, W):
    """(A3 [M, 3K], W3 [N, 3K]) with A3 . W3^T = Ahi Whi^T + Alo Whi^T + Ahi Wlo^T: what a bf16x3 kernel contracts after
    splitting f32 operands A, W itself (the dropped lo . lo term is part of the SCHEME, not of the kernel's error)."""
    ah, al = split_bf16(A)
    wh, wl = split_bf16(W)
    return torch.cat([ah, al, ah], 1), torch.cat([wh, wh, wl], 1)


def reference_aw(A, W, op_dtype, *, bias=None, rowbias=None, rowgate=None, residual=None, residual_bcast=0, rpb=0, act=0,
                 exact_gelu=False, plain32=True):
    """(y, S', E_epi, y32) of the float64 operand matrices A, W (values of `op_dtype`, for the subnormal term) and the epilogue;
    y32 = plain fp32 arithmetic on the same operands (tf32 off) for the exact-rounding-rate baseline, or None."""
    M = A.shape[0]
    y, s = A @ W.T, A.abs() @ W.abs().T + subnormal_term(A, W, op_dtype) / ACC      # (E_sub rides in S' through the epilogue)
    y32 = A.float() @ W.float().T if plain32 else None
    add32 = lambda t: None if y32 is None else y32 + t
    b_of = torch.arange(M, device=A.device) // rpb if rpb else None
    if bias is not None:
        y, s, y32 = y + bias.to(F64), s + bias.to(F64).abs(), add32(bias)
    if rowbias is not None:
        rb = rowbias[b_of]
        y, s, y32 = y + rb.to(F64), s + rb.to(F64).abs(), add32(rb)
    if rowgate is not None:
        gt = rowgate[b_of]
        y, s, y32 = y * gt.to(F64), s * gt.to(F64).abs(), None if y32 is None else y32 * gt
    if residual is not None:
        r = residual[torch.arange(M, device=A.device) % rpb] if residual_bcast else residual
        y, s, y32 = y + r.to(F64), s + r.to(F64).abs(), add32(r.float())
    y, s, e = apply_act(y, s, act, exact_gelu=exact_gelu)
    if act == 1 and y32 is not None:
        y32 = F.silu(y32)
    return y, s, e, (y32 if act in (0, 1) else None)


def reference(a, w, *, a2=None, conv=None, **epilogue):
    """reference_aw on the operands of a 16-bit (or bf16-triple) GEMM / conv call as the kernel is given them."""
    A, W = operands(a, w, a2=a2, conv=conv)
    return reference_aw(A, W, w.dtype, **epilogue)


def run_all(fn, dt, cases):
    """Runs every case of a table (a failure does not hide the cases after it), then reports all failures at once."""
    errs = []
    for name, (key, kw) in cases.items():
        try:
            fn(name, dt, key, **kw)
        except AssertionError as e:
            errs.append(str(e).split("\n")[0])
    assert not errs, "\n".join(errs)


# ---- the fp32-storage GEMM forms (tests/test_gpu_x3_exact.py) ----------------------------------------------------------------------
# Accumulation constant per family, in units of S3 / S (docstring above: "fp32-storage GEMM forms").
X3_ACC = {"x3t": ACC, "x3": ACC, "f32": ACC}
SCHEME_REL = 3 * 2.0 ** -16       # |y3 - y| <= SCHEME_REL S: the bf16x3 scheme itself (tests/test_exact_checker.py)
PAIR_REL = 2.0 ** -16             # |hi + lo - v| <= PAIR_REL |v|: a value carried as a bf16 hi | lo pair

# The instantiations the triple-operand path (sdn_gemm_bf16 with x3_out, K' = 3K) reaches, bf16 only: the seven plain k_gemm_dma
# tiles and the slab-ring convolution.  Not reachable with x3_out, each refused by sdn_gemm_impl: the LayerNorm-folded forms
# (x3 && ln_c -> invalid: the precise plans normalise in f32 and write the triple), split-K (x3 && split_k > 1 -> invalid: the
# partials would need a triple-aware reduce) and k_ffn320 (a 16-bit-only fusion with its own entry point, which takes no triples).
# sdn_gemm_x3 / sdn_gemm_f32 (k_gemm_x3<CONV, XNJ>, k_gemm_f32 in sdn_f32.hip) keep no launch record; their tiles follow from the
# shape by the rules restated in the case tables of tests/test_gpu_x3_exact.py.
X3T_INSTANTIATIONS = [("dma", n, w, s, 0) for n, w, s in ((10, 4, 2), (8, 4, 2), (5, 2, 4), (5, 2, 2), (4, 2, 2), (2, 2, 2), (1, 2, 2))] \
    + [("slab",)]
X3_KERNELS = [("k_gemm_x3", conv, xnj) for conv in (False, True) for xnj in (5, 4)] + [("k_gemm_f32", conv) for conv in (False, True)]


def check_split_planes(out16, f, planes):
    """Bit equality of the bf16 planes a kernel wrote (out16 [M, planes, W]: hi | lo [| hi]) with the split of the f32 result f
    [M, W] of the same operands: hi = RNE_bf16(f), lo = RNE_bf16(f - hi), third plane = hi.  Returns the list of what differs."""
    hi = f.bfloat16()
    lo = (f - hi.float()).bfloat16()
    bits = lambda t: t.contiguous().view(torch.int16)
    bad = []
    if not torch.equal(bits(out16[:, 0]), bits(hi)):
        bad.append(f"hi plane differs from bf16(f) in {int((bits(out16[:, 0]) != bits(hi)).sum())} elements")
    if not torch.equal(bits(out16[:, 1]), bits(lo)):
        bad.append(f"lo plane differs from bf16(f - hi) in {int((bits(out16[:, 1]) != bits(lo)).sum())} elements")
    if planes == 3 and not torch.equal(bits(out16[:, 2]), bits(out16[:, 0])):
        bad.append(f"third plane differs from hi in {int((bits(out16[:, 2]) != bits(out16[:, 0])).sum())} elements")
    return bad


# ---- the normalisation kernels (tests/test_gpu_norm_exact.py; docstring above: "Normalisation kernels") -----------------------------
NORM_ARITH = {"gn16": 6 * 2.0 ** -24, "gn16serial": 6 * 2.0 ** -24, "gn16cols": 6 * 2.0 ** -24, "ln16": 6 * 2.0 ** -24, "ln16mod": 7 * 2.0 ** -24, "gnf32": 6 * 2.0 ** -24, "lnf32": 6 * 2.0 ** -24,
              "lnf32mod": 7 * 2.0 ** -24}
# Statistics constant per family, 4x the measured worst (profiles/norm_exact.json); NORM_STAT_CHAIN: the longest serial fp32 chain
# of the family's statistics over the tested shapes (norm_cases.gn16_chain / ln16_chain restate the code), whose 2^-24 multiple is
# the hard bound the constant must stay below.
NORM_STAT = {"gn16": 4 * 0.507 * ACC, "gn16serial": 4 * 3.913 * ACC, "gn16cols": 4 * 0.238 * ACC, "ln16": 4 * 0.426 * ACC,
             "gnf32": 2.0 ** -24, "lnf32": 2.0 ** -24}
NORM_STAT_FAMILY = {"gn16": "gn16", "gn16serial": "gn16serial", "gn16cols": "gn16cols", "ln16": "ln16", "ln16mod": "ln16", "gnf32": "gnf32", "lnf32": "lnf32",
                    "lnf32mod": "lnf32"}
CLEAN_SHARE_MIN = 0.98

# What the launchers of sdn_norm.hip and sdn_f32.hip can launch (tests/test_exact_checker.py parses them), as
# (name, NQ or NV, R): the key sdn_debug_norm_last_launch's record maps to (norm_launch_key).
NORM_KERNEL = {1: "gn_stats", 2: "gn_cols", 3: "layernorm", 4: "layernorm_mod", 5: "row_stats", 6: "gn_f32_rows", 7: "gn_f32_pairs",
               8: "gn_f32_any", 9: "ln_f32_regs", 10: "ln_f32", 11: "ln_mod_f32"}
NORM_INSTANTIATIONS = (
    [("gn_stats", 0, 0), ("gn_cols", 0, 0)]
    + [(k, nq, r) for k in ("layernorm", "layernorm_mod", "row_stats") for nq, r in ((1, 4), (2, 2), (4, 1))]
    + [("gn_f32_rows", 0, 0), ("gn_f32_pairs", 0, 0), ("gn_f32_any", 0, 0), ("ln_f32_regs", 0, 0), ("ln_f32", 0, 0)]
    + [("ln_mod_f32", nv, 0) for nv in (2, 4, 8)])
NORM_16BIT = {"gn_stats", "gn_cols", "layernorm", "layernorm_mod", "row_stats"}       # run in bf16 and fp16; the others in f32
NORM_TRIPLE = {"gn_f32_rows", "gn_f32_pairs", "gn_f32_any", "ln_f32_regs", "ln_f32"}   # have a *_f32_triple entry point
NL_FIELDS = ("kernel", "dtype", "nq", "r", "nch", "ct", "ntiles", "rows_per_tile", "rpc", "nchunk", "stats_src", "triple")


def norm_launch_key(rec) -> tuple:
    """sdn_debug_norm_last_launch's record -> the NORM_INSTANTIATIONS key it ran."""
    return (NORM_KERNEL[rec[0]], rec[2], rec[3])


def norm_coverage_wanted() -> set:
    """(key, dtype code, triple) of everything the norm launchers can run: 16-bit kernels in bf16 (0) and fp16 (1), f32 ones (2)
    plain and, where the entry point exists, triple."""
    want = set()
    for k in NORM_INSTANTIATIONS:
        if k[0] in NORM_16BIT:
            want |= {(k, 0, 0), (k, 1, 0)}
        else:
            want |= {(k, 2, 0)} | ({(k, 2, 1)} if k[0] in NORM_TRIPLE else set())
    return want


def norm_reference(x, g, b, dims, eps, *, e2, family, act=0, stat=None):
    """Float64 reference of y = (x - mu) r g + b over the sets spanned by `dims` of x (g, b broadcastable to x).
    e2: the kernel forms E[x^2] - mean^2 (M2 = mean x^2) rather than centred squares (M2 = v).
    Returns dict(y, s, e, pre_y, pre_budget, mu, r, m1, k2, S, Q): s = (ARITH S + STAT Q) / ACC for analyse(), carried through the
    activation; pre_y / pre_budget = y and ARITH S + STAT Q before the activation (the clean share's terms); k2 = M2 / (2 (v + eps))."""
    x, g, b = x.to(F64), g.to(F64), b.to(F64)
    eps = float(torch.tensor(eps, dtype=torch.float32))       # the kernels take eps as a float
    arith = NORM_ARITH[family]
    stat = NORM_STAT[NORM_STAT_FAMILY[family]] if stat is None else stat
    mu = x.mean(dims, keepdim=True)
    v = ((x - mu) ** 2).mean(dims, keepdim=True)
    r = (v + eps) ** -0.5
    m1 = x.abs().mean(dims, keepdim=True)
    k2 = ((x * x).mean(dims, keepdim=True) if e2 else v) / (2 * (v + eps))
    y = (x - mu) * r * g + b
    S = g.abs() * r * (x.abs() + mu.abs()) + b.abs()
    Q = g.abs() * r * (m1 + (x - mu).abs() * k2)
    pre_y = y
    y, s, e = apply_act(y, (arith * S + stat * Q) / ACC, act)
    return dict(y=y, s=s, e=e, pre_y=pre_y, pre_budget=arith * S + stat * Q, mu=mu, r=r, m1=m1, k2=k2, S=S, Q=Q)


def clean_share(ref, dtype) -> float:
    """Fraction of the elements with ARITH S + STAT Q <= 1/4 ulp_T(y), y = (x - mu) r g + b: where the storage rounding decides."""
    return float((ref["pre_budget"] <= 0.25 * ulp(ref["pre_y"], dtype)).double().mean())


def stat_errors(mean_out, rstd_out, ref) -> dict:
    """Statistics a kernel exposed (f32) against the reference's, in the units STAT is measured in: the worst |mean_out - mu| / m1
    and |rstd_out - r| / (r k2).  Sets with k2 < 1/4 (v + eps dominated by eps: an all-zero group, a set of one zero) are left out
    of the rstd figure: there the variance carries no error to measure and what is left is rsqrtf's own (stat_failures)."""
    mu, r, m1, k2 = (ref[k].reshape(mean_out.shape) for k in ("mu", "r", "m1", "k2"))
    dm, dr = (mean_out.to(F64) - mu).abs(), (rstd_out.to(F64) - r).abs()
    rel_m = torch.where(m1 > 0, dm / m1.clamp_min(1e-300), torch.zeros_like(dm))
    rel_r = torch.where(k2 >= 0.25, dr / (r * k2.clamp_min(0.25)), torch.zeros_like(dr))
    return dict(mean_err=float(rel_m.max()), rstd_err=float(rel_r.max()), dm=dm, dr=dr, mu=mu, r=r, m1=m1, k2=k2)


RSQRT_REL = 2.0 ** -22            # rsqrtf / 1 / sqrt: <= 2 ulp, the figure ARITH uses


def stat_failures(se, stat) -> list:
    """Sets outside |mean_out - mu| <= 1/2 ulp_f32(mu) + STAT m1 or |rstd_out - r| <= 1/2 ulp_f32(r) + max(STAT k2, RSQRT_REL) r.
    The floor RSQRT_REL only acts where k2 < RSQRT_REL / STAT (<= 1/4 for STAT >= 2^-20), i.e. where eps dominates v + eps and
    the formula's M2 / (2 (v + eps)) would leave the reciprocal square root's own 2 ulp no room at all."""
    f = []
    bad_m = se["dm"] > 0.5 * ulp(se["mu"], torch.float32) + stat * se["m1"]
    bad_r = se["dr"] > 0.5 * ulp(se["r"], torch.float32) + torch.clamp(stat * se["k2"], min=RSQRT_REL) * se["r"]
    if bool(bad_m.any()):
        f.append(f"{int(bad_m.sum())} means outside the bound (worst {se['mean_err']:.3g} m1)")
    if bool(bad_r.any()):
        f.append(f"{int(bad_r.sum())} rstd outside the bound (worst {se['rstd_err']:.3g} r M2 / (2 (v + eps)))")
    if bool(torch.isnan(se["dm"]).any() | torch.isnan(se["dr"]).any()):
        f.append("NaN statistics")
    return f
