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
"""
import math

import torch

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


def apply_act(y, s, act):
    """Exact activation of the float64 pre-activation y with magnitude s: (value, S', E_epi).  act codes as sdn_gemm_desc."""
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
        return v, sp, (GEGLU_ABS * h.abs()).reshape(M, N // 2)
    raise ValueError(act)


def analyse(out: torch.Tensor, y: torch.Tensor, s: torch.Tensor, e_epi=None, dtype=None) -> dict:
    """Statistics of out (any float dtype, the kernel's output) against the exact y (float64) with magnitude s."""
    dtype = dtype or out.dtype
    o = out.to(torch.float64)
    y = y.to(torch.float64)
    u = ulp(y, dtype)
    rn = round_to(y, dtype)
    tol = 0.5 * u + ACC * s + (0 if e_epi is None else e_epi)
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
