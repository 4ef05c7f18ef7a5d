"""Every 16-bit GEMM-family instantiation, both dtypes, element by element against float64 arithmetic on the same 16-bit operands
(criterion: tests_support/exact.py).  Each case names the instantiation it is written for and asserts through the launch record
(sdn_debug_gemm_last_launch) that it ran there; the last test asserts that the cases covered every reachable instantiation.

Outputs are views into NaN-sentinel buffers (before, after, ldc gap); A rows past M, conv map tails and residual rows past M are
NaN in the same allocation, so an unwritten tile, a stray store or a stray read cannot pass unnoticed."""
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
DTYPES = [torch.bfloat16, torch.float16]
_SEEN = set()                 # (dtype name, instantiation key) of every case that ran and passed its launch check
_STATS = []                   # per-case statistics (written to $SDN_EXACT_STATS when set)
F64 = torch.float64


def _last_launch():
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    return list(rec)


def _t(g, *shape, scale=1.0, dt=torch.bfloat16):
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


_im2col, _reference = X.im2col, X.reference       # (shared with tests/test_gpu_x3_exact.py)


def _check(name, dt, key, out, buf, y, s, e, y32, *, exact_fn, out_dtype=None, direction=True):
    rec = _last_launch()
    got = X.launch_key(rec)
    assert got == key, f"{name}: ran {got} (record {rec}), written for {key}"
    torch.cuda.synchronize()
    bad = X.sentinels_intact(buf, out) if buf is not None else 0
    od = out_dtype or out.dtype
    st = X.analyse(out, y, s, e, dtype=od)
    rr = X.ref_rate(y32, y, od) if (exact_fn and y32 is not None) else None
    f32 = od == torch.float32                                # (no 16-bit rounding to judge: exact.py)
    fails = X.failures(st, exact_fn=exact_fn and not f32, ref_rate=rr, direction=direction and not f32)
    if bad:
        fails.append(f"{bad} guard-band sentinels overwritten")
    _STATS.append(dict(case=name, dtype=str(dt).split(".")[-1], inst="/".join(map(str, key)), tiles=rec[6:9], n=st["n"],
                       rate=round(st["rate"], 4), torch_rate=None if rr is None else round(rr, 4), max_ulp=round(st["max_ulp"], 3),
                       max_err_over_bound=round(st["max_err_over_tol"], 3), direction=round(st["direction"], 4), n_dir=st["n_dir"],
                       log2_err_over_S=round(math.log2(max(st["err_over_s"], 1e-300)), 2)))
    assert not fails, f"{name} [{dt}] on {key}: " + "; ".join(fails)
    _SEEN.add((str(dt), key))


def _gemm_case(name, dt, key, *, M, N, K, K2=0, bias=True, rowbias_rpb=0, rowgate=False, residual=False, residual_bcast=0,
               res_pre=0, act=0, out_kind=0, n_valid=0, ldc_pad=0, split_k=0, scale_rows=False, subnormal_a=False, w_scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + (1 if dt == torch.float16 else 0))
    a = _t(g, M, K, dt=dt)
    if scale_rows:                           # fp16 range: rows scaled 2^-26 ... 2^13 (zero / subnormal outputs ... overflow)
        sc = torch.exp2(torch.arange(M, dtype=torch.float32) % 40 - 26.0).cuda()
        a = (a.float() * sc[:, None]).to(dt)
    if subnormal_a:                          # every 4th row entirely subnormal (fp16: < 2^-14), the others normal
        a[::4] = (a[::4].float() * 2.0 ** -17).to(dt)
    a = X.with_nan_tail(a, 64)
    a2 = X.with_nan_tail(_t(g, M, K2, dt=dt), 64) if K2 else None
    w = _t(g, N, K + K2, scale=w_scale * (K + K2) ** -0.5, dt=dt)
    if act == 2:
        w = w * 2
    bv = torch.randn(N, generator=g).cuda() if bias else None
    rpb = rowbias_rpb
    nb = (M + rpb - 1) // rpb if rpb else 0
    rb = torch.randn(nb, N, generator=g).cuda() if (rpb and not rowgate) else None
    gt = (torch.randn(nb, N, generator=g) * 0.5).cuda() if rowgate else None
    res = None
    if residual:
        rrows = rpb if residual_bcast else M
        res = X.with_nan_tail(_t(g, rrows, N, dt=dt), 64)
    width = N // 2 if act == 2 else (n_valid or N)
    if out_kind == 2:
        buf, out = X.guarded_like((M // rpb, width, rpb), torch.float32, "cuda")
    else:
        buf, out = X.guarded(M, width, torch.float32 if out_kind == 1 else dt, "cuda", ldc=width + ldc_pad)
    kw = dict(bias=bv, rowbias=rb, rowgate=gt, residual=res, residual_bcast=residual_bcast, res_pre=res_pre, act=act,
              out_kind=out_kind, n_valid=n_valid, rows_per_batch=rpb, a2=a2, out=out)
    ops.gemm(a, w, split_k=split_k, **kw)
    if split_k:                               # deterministic: a second run gives the same bits
        rec = _last_launch()
        buf2, out2 = X.guarded(M, width, dt, "cuda", ldc=width + ldc_pad)
        ops.gemm(a, w, split_k=split_k, **dict(kw, out=out2))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), f"{name}: split-K is not deterministic"
        assert _last_launch() == rec
    y, s, e, y32 = _reference(a, w, a2=a2, bias=bv, rowbias=rb, rowgate=gt, residual=res, residual_bcast=residual_bcast, rpb=rpb, act=act)
    if n_valid:
        y, s, e, y32 = y[:, :n_valid], s[:, :n_valid], e[:, :n_valid], None if y32 is None else y32[:, :n_valid]
    if out_kind == 2:                        # NCHW f32: [B, n_valid, rows_per_batch]
        nchw = lambda t: t.reshape(M // rpb, rpb, -1).permute(0, 2, 1)
        y, s, e, y32 = nchw(y), nchw(s), nchw(e), None if y32 is None else nchw(y32)
    _check(name, dt, key, out, buf, y, s, e, y32, exact_fn=act in (0, 1), out_dtype=torch.float32 if out_kind else dt, direction=act != 2)
    return out


def _conv_case(name, dt, key, *, B, H, Cin, N, stride=1, upsample=0, asym_pad=0, bias=True, rowbias=False, residual=False,
               col_stats=False, res_pre=0, n_valid=0, out_kind=0, seed=0):
    g = torch.Generator().manual_seed(seed + (1 if dt == torch.float16 else 0))
    Hi = 2 * H if upsample else H
    Ho = (Hi + (1 if asym_pad else 2) - 3) // stride + 1
    conv = dict(Hs=H, Ws=H, Cin=Cin, Ho=Ho, Wo=Ho, stride=stride, upsample=upsample, asym_pad=asym_pad)
    x = X.with_nan_tail(_t(g, B * H * H, Cin, dt=dt), 64).view(B, H, H, Cin)          # NaN past the map
    w = _t(g, N, 9 * Cin, scale=(9 * Cin) ** -0.5, dt=dt)
    M, rpb = B * Ho * Ho, Ho * Ho
    bv = torch.randn(N, generator=g).cuda() if bias else None
    rb = torch.randn(B, N, generator=g).cuda() if rowbias else None
    res = X.with_nan_tail(_t(g, M, N, dt=dt), 64) if residual else None
    width = n_valid or N
    if out_kind == 2:
        buf, out = X.guarded_like((B, width, rpb), torch.float32, "cuda")
    else:
        buf, out = X.guarded(M, width, dt, "cuda", ldc=width + (8 if not col_stats else 0))
    cs = None
    if col_stats:
        cbuf, cs = X.guarded_like(((M + 127) // 128, N, 2), torch.float32, "cuda")
    ops.gemm(x, w, bias=bv, rowbias=rb, residual=res, conv=conv, col_stats=cs, res_pre=res_pre, n_valid=n_valid, out_kind=out_kind,
             out=out)
    y, s, e, y32 = _reference(x, w, conv=conv, bias=bv, rowbias=rb, residual=res, rpb=rpb)
    if n_valid:
        y, s, y32 = y[:, :n_valid], s[:, :n_valid], y32[:, :n_valid]
    if out_kind == 2:
        nchw = lambda t: t.reshape(B, rpb, -1).permute(0, 2, 1)
        y, s, y32 = nchw(y), nchw(s), nchw(y32)
    e = torch.zeros_like(y)                  # (no activation on a conv)
    _check(name, dt, key, out, buf, y, s, e, y32, exact_fn=True, out_dtype=torch.float32 if out_kind else dt)
    if col_stats:
        _check_col_stats(name, out, cs, cbuf, M)
    return out


def _check_col_stats(name, out, cs, cbuf, M):
    """col_stats [ceil(M / 128)][N][2] = fp32 (sum, sum of squares) of the STORED values of each 128-row block; rows >= M add nothing."""
    v = out.to(F64)
    pad = (-M) % 128
    v = torch.cat([v, torch.zeros(pad, v.shape[1], dtype=F64, device=v.device)]).view(-1, 128, v.shape[1])
    for i, ref, mag in ((0, v.sum(1), v.abs().sum(1)), (1, (v * v).sum(1), (v * v).sum(1))):
        err = (cs[..., i].to(F64) - ref).abs()
        assert bool((err <= 2.0 ** -17 * mag + 1e-30).all()), (name, "col_stats", i, float((err / mag.clamp_min(1e-30)).max()))
    assert X.sentinels_intact(cbuf, cs) == 0, (name, "col_stats guard band")


def _ln_case(name, dt, key, *, M, N, K, prepass, act=0, seed=0):
    from safe_denoiser_amd.unet import _interleave16
    g = torch.Generator().manual_seed(seed + (1 if dt == torch.float16 else 0))
    x = ((torch.randn(M, K, generator=g) * 1.5 + torch.randn(M, 1, generator=g) * 0.5)).to(dt).cuda()
    x = X.with_nan_tail(x, 64)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt)
    gamma = (1 + 0.2 * torch.randn(K, generator=g)).cuda(); beta = (0.3 * torch.randn(K, generator=g)).cuda()
    bias = torch.randn(N, generator=g)
    if act == 2:
        w, bias = _interleave16(w).contiguous(), _interleave16(bias).contiguous()
    w, bias = w.cuda(), bias.cuda()
    width = N // 2 if act == 2 else N
    buf, out = X.guarded(M, width, dt, "cuda", ldc=width + 8)
    fold = {}
    ops.gemm_ln(x, w, gamma, beta, bias, act=act, prepass=prepass, out=out, fold=fold)
    xd = x.to(F64)
    mu = xd.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    wf, c, d = fold["w_folded"].to(F64), fold["c"].to(F64), fold["d"].to(F64)
    y = rs * (xd @ wf.T - mu * c) + d
    s = rs * (xd.abs() @ wf.abs().T + mu.abs() * c.abs()) + d.abs()
    y, s, e = X.apply_act(y, s, act)
    y32 = None
    if act == 0:
        xf = x.float(); muf = xf.mean(1, keepdim=True); rsf = torch.rsqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5)
        y32 = rsf * (xf @ fold["w_folded"].float().T - muf * fold["c"]) + fold["d"]
    _check(name, dt, key, out, buf, y, s, e, y32, exact_fn=act == 0, direction=act != 2)
    return out


# ---------------------------------------------------------------------------------------------------------------- the matrix
D = ("dma",)
PLAIN = {
    # name: (instantiation, kwargs)
    "192 big tiles, tail 19, bias":              (D + (10, 4, 2, 0), dict(M=191 * 256 + 19, N=320, K=320)),
    "192 big tiles, GEGLU":                      (D + (10, 4, 2, 0), dict(M=191 * 256 + 37, N=640, K=320, act=2)),
    "191 big tiles -> 128-row tile":             (D + (5, 2, 2, 0), dict(M=191 * 256, N=320, K=320)),
    "256-wide big tile, tail 37, row bias 333":  (D + (8, 4, 2, 0), dict(M=192 * 256 + 37, N=256, K=320, rowbias_rpb=333)),
    "256-wide big tile, tanh-GELU":              (D + (8, 4, 2, 0), dict(M=192 * 256 + 19, N=256, K=384, act=3)),
    "256 tiles, deep ring, residual":            (D + (5, 2, 4, 0), dict(M=128 * 128, N=320, K=576, residual=True)),
    "255 tiles, 5 n-tiles (panel rest), tail 37": (D + (5, 2, 4, 0), dict(M=50 * 128 + 37, N=800, K=512, ldc_pad=8)),
    "258 tiles, SiLU":                           (D + (5, 2, 2, 0), dict(M=128 * 128 + 1, N=320, K=576, act=1)),
    "K = 64, res_pre":                           (D + (5, 2, 2, 0), dict(M=128 * 128 + 19, N=320, K=64, residual=True, res_pre=1)),
    "f32 output, n_valid < N, dual source K1":   (D + (5, 2, 2, 0), dict(M=128 * 130 + 5, N=320, K=192, K2=128, out_kind=1, n_valid=317)),
    "row gate + residual (adaLN-zero), rpb 77":  (D + (4, 2, 2, 0), dict(M=87 * 128 - 1, N=384, K=256, rowbias_rpb=77, rowgate=True, residual=True)),
    "residual_bcast, rpb 333":                   (D + (4, 2, 2, 0), dict(M=333 * 34, N=384, K=256, rowbias_rpb=333, residual=True, residual_bcast=1)),
    "M = 1":                                     (D + (2, 2, 2, 0), dict(M=1, N=320, K=640)),
    "M = 127":                                   (D + (2, 2, 2, 0), dict(M=127, N=320, K=640, ldc_pad=16)),
    "254 tiles -> 64-wide tile":                 (D + (2, 2, 2, 0), dict(M=127 * 128, N=320, K=576)),
    "GEGLU on the 128 x 128 tile, tail 19":      (D + (4, 2, 2, 0), dict(M=126 * 128 + 19, N=640, K=320, act=2)),
    "NCHW f32 output, n_valid 50":               (D + (2, 2, 2, 0), dict(M=3 * 333, N=64, K=128, out_kind=2, rowbias_rpb=333, n_valid=50)),
    "N = 96, n_valid 90, ldc > width":           (D + (1, 2, 2, 0), dict(M=1000, N=96, K=64, n_valid=90, ldc_pad=14)),
    "N = 32, M = 129, SiLU":                     (D + (1, 2, 2, 0), dict(M=129, N=32, K=128, act=1)),
    "split-K: bias + row bias + residual":       (("splitk",), dict(M=333, N=320, K=1280, rowbias_rpb=77, residual=True, split_k=4)),
    "split-K: row gate, residual_bcast":         (("splitk",), dict(M=333, N=320, K=1280, rowbias_rpb=111, rowgate=True, residual=True,
                                                                   residual_bcast=1, split_k=5)),
    "split-K: SiLU":                             (("splitk",), dict(M=64, N=640, K=2304, act=1, split_k=8)),
    "split-K: tanh-GELU":                        (("splitk",), dict(M=77, N=640, K=1536, act=3, split_k=3)),
}
FP16_RANGE = {
    "fp16 overflow + subnormal outputs":         (D + (5, 2, 2, 0), dict(M=128 * 130, N=320, K=64, bias=False, scale_rows=True, w_scale=4.0)),
    "fp16 subnormal operands":                   (D + (2, 2, 2, 0), dict(M=4 * 128 + 3, N=320, K=256, bias=False, subnormal_a=True, w_scale=16.0)),
}
CONV = {
    "slab ring W = 32, row bias":                (("slab",), dict(B=48, H=32, Cin=64, N=320, rowbias=True)),
    "slab ring W = 16, residual + col_stats":    (("slab",), dict(B=192, H=16, Cin=192, N=320, residual=True, col_stats=True)),
    "implicit conv, stride 2 + asym_pad":        (D + (2, 2, 2, 0), dict(B=2, H=16, Cin=64, N=320, stride=2, asym_pad=1)),
    "implicit conv, stride 2, symmetric":        (D + (2, 2, 2, 0), dict(B=3, H=16, Cin=128, N=128, stride=2)),
    "implicit conv, upsample":                   (D + (2, 2, 2, 0), dict(B=2, H=8, Cin=64, N=320, upsample=1)),
    "implicit conv, 4 x 4 map (Wo < 8)":         (D + (1, 2, 2, 0), dict(B=5, H=4, Cin=64, N=96)),
    "implicit conv, 6 x 6 up to 12, col_stats":  (D + (2, 2, 2, 0), dict(B=3, H=6, Cin=64, N=64, upsample=1, col_stats=True, residual=True)),
    "implicit conv 256-row tile, tail 64, col_stats": (D + (10, 4, 2, 0), dict(B=765, H=8, Cin=256, N=320, col_stats=True)),
    "conv_out: Cout 4 of 32, f32 NCHW":          (D + (1, 2, 2, 0), dict(B=2, H=16, Cin=64, N=32, n_valid=4, out_kind=2)),
}
LN = {
    "LN pre-pass, 256 x 320":                    (D + (10, 4, 2, 2), dict(M=191 * 256 + 19, N=320, K=320, prepass=True)),
    "LN pre-pass, 128 x 160":                    (D + (5, 2, 2, 2), dict(M=128 * 129 + 37, N=320, K=320, prepass=True)),
    "LN pre-pass, GEGLU 128 x 128":              (D + (4, 2, 2, 2), dict(M=13 * 128 + 19, N=2560, K=320, prepass=True, act=2)),
    "LN pre-pass, 128 x 64":                     (D + (2, 2, 2, 2), dict(M=300, N=320, K=320, prepass=True)),
    "LN fragments, 256 x 320, GEGLU":            (D + (10, 4, 2, 1), dict(M=191 * 256 + 37, N=640, K=320, prepass=False, act=2)),
    "LN fragments, 128 x 160":                   (D + (5, 2, 2, 1), dict(M=128 * 129 + 1, N=320, K=640, prepass=False)),
    "LN fragments, 128 x 64":                    (D + (2, 2, 2, 1), dict(M=129, N=320, K=320, prepass=False)),
}


@pytest.fixture(autouse=True)
def _no_tf32():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


_run_all = X.run_all


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_plain_and_split_k_forms_are_exact(dt):
    _run_all(_gemm_case, dt, dict(PLAIN, **(FP16_RANGE if dt == torch.float16 else {})))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_conv_forms_are_exact(dt):
    _run_all(_conv_case, dt, CONV)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_layernorm_folded_forms_are_exact(dt):
    _run_all(_ln_case, dt, LN)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_fused_feed_forward_is_exact(dt):
    """k_ffn320: out = x + [H | h3] . Wcat^T + bcat, H = the 16-bit GEGLU hidden (the kernel rounds it to 16 bit by design, the
    same bits as sdn_gemm_ln_*: tests/test_gpu_ops.py) -- so the exact reference takes H from the LayerNorm-folded GEGLU GEMM,
    itself checked above."""
    from safe_denoiser_amd.unet import _interleave16
    g = torch.Generator().manual_seed(5 + (1 if dt == torch.float16 else 0))
    Cc, M = 320, 128 * 5 + 37
    x = X.with_nan_tail(((torch.randn(M, Cc, generator=g) * 1.5 + torch.randn(M, 1, generator=g))).to(dt).cuda(), 64)
    w1 = _interleave16((torch.randn(8 * Cc, Cc, generator=g) * Cc ** -0.5).to(dt)).contiguous().cuda()
    b1 = _interleave16(torch.randn(8 * Cc, generator=g)).contiguous().cuda()
    gamma = (1 + 0.2 * torch.randn(Cc, generator=g)).cuda(); beta = (0.3 * torch.randn(Cc, generator=g)).cuda()
    wcat = (torch.randn(Cc, 5 * Cc, generator=g) * (5 * Cc) ** -0.5).to(dt).cuda()
    bcat = torch.randn(Cc, generator=g).cuda()
    res = X.with_nan_tail(torch.randn(M, Cc, generator=g).to(dt).cuda(), 64)
    for prepass in (True, False):
        hid = ops.gemm_ln(x, w1, gamma, beta, b1, act=2, prepass=prepass)
        nblk = (M + 127) // 128
        cbuf, cs = X.guarded_like((nblk, Cc, 2), torch.float32, "cuda")
        ops.SENTINEL = True                    # output starts as NaN: an unwritten tile fails the NaN check
        try:
            out = ops.ffn_fused(x, w1, gamma, beta, b1, wcat, bcat, res, col_stats=cs, own_stats=not prepass)
        finally:
            ops.SENTINEL = False
        y, s, e, y32 = _reference(hid, wcat, a2=x, bias=bcat, residual=res)
        _check(f"ffn320 ({'pre-pass' if prepass else 'fragment'} statistics)", dt, ("ffn",), out, None, y, s, e, y32, exact_fn=True)
        _check_col_stats("ffn320", out, cs, cbuf, M)


def test_every_instantiation_ran_in_both_dtypes():
    """The cases above covered exactly the reachable instantiations (tests_support/exact.py INSTANTIATIONS), in both dtypes."""
    want = {(str(dt), k) for dt in DTYPES for k in X.INSTANTIATIONS}
    if os.environ.get("SDN_EXACT_STATS"):                 # per-case table: rates, worst ulps, direction statistic
        with open(os.environ["SDN_EXACT_STATS"], "w") as f:
            json.dump(_STATS, f, indent=0)
    assert _SEEN == want, dict(missing=sorted(map(str, want - _SEEN)), unexpected=sorted(map(str, _SEEN - want)))
