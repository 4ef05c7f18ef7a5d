"""Every normalisation kernel -- the 16-bit GroupNorm (own statistics pass and column sums), LayerNorm, adaLN and row statistics
of sdn_norm.hip, the f32 GroupNorm / LayerNorm / adaLN forms of sdn_f32.hip -- element by element against float64 arithmetic on the
values the kernel reads (criterion: tests_support/exact.py, "Normalisation kernels"):

    |out - f(y)| <= 1/2 ulp_T(f(y)) + ARITH S + STAT Q

Each case names the kernel form it is written for and asserts it through sdn_debug_norm_last_launch; the last test asserts that
every form the launchers can reach ran in every dtype it exists in.  Outputs AND workspaces are views into NaN-sentinel buffers;
inputs carry a NaN row right behind their valid extent (k_gn_stats, k_layernorm and k_row_stats clamp tail loads to the last valid
row, so one row past it poisons a checked value).  The statistics the kernels expose (stats_ws, sdn_row_stats_*) are asserted
against the float64 ones and feed the STAT measurement; triple outputs must be, bit for bit, the split of the checked f32 output.
Shapes, inputs and launch plans live in tests_support/norm_cases.py, shared with the CPU checker tests.

Clean share: outside the named cancellation cases (GroupNorm at |mean| / std >= 30, the constant map, fp16 near 60000; LayerNorm
rows with a large common offset, where S / |y| is what is being probed) at least 98 % of a 16-bit case's elements have
ARITH S + STAT Q <= 1/4 ulp_T(y)."""
import ctypes as C
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import safe_denoiser_amd as sda
from tests_support import exact as X
from tests_support import norm_cases as NC
from tests_support import ops

pytestmark = pytest.mark.gpu
F32, F64, BF, FP16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
DT16 = pytest.mark.parametrize("dt", [BF, FP16], ids=["bf16", "f16"])
DCODE = {BF: 0, FP16: 1, F32: 2}
_SEEN = set()                 # (NORM_INSTANTIATIONS key, dtype code, triple) of every case that ran and passed
_STATS = []                   # per-case statistics (written to $SDN_EXACT_STATS when set)


def _record():
    rec = (C.c_int * len(X.NL_FIELDS))()
    sda.lib().sdn_debug_norm_last_launch(rec, len(X.NL_FIELDS))
    return list(rec)


def _expect_launch(name, key, dt, **fields):
    """The launch record must be the form (and plan) the case is written for; returns the failures."""
    rec = _record()
    got = dict(zip(X.NL_FIELDS, rec))
    bad = [f"{k} {got[k]} != {v}" for k, v in fields.items() if got[k] != v]
    if X.norm_launch_key(rec) != key or got["dtype"] != DCODE[dt]:
        bad.append(f"ran {X.norm_launch_key(rec)} dtype {got['dtype']}")
    return [f"{name}: written for {key}, " + ", ".join(bad)] if bad else []


def _tail(t, rows):
    """t (CPU) -> GPU [rows, ...] view with one NaN row behind it, reshaped back."""
    return X.with_nan_tail(t.reshape(rows, -1).cuda(), 1).view(t.shape)


def _judge(name, family, key, dt, out, buf, ref, *, triple=0, cancellation=False, ref32=None, assert_rate=False, stat=None, extra=()):
    """Bound, NaN, guard-band, clean-share, rate and direction verdict of one launch; records the case."""
    torch.cuda.synchronize()
    fails = list(extra)
    bad = X.sentinels_intact(buf, out)
    if bad:
        fails.append(f"{bad} guard-band sentinels overwritten")
    o = out.cpu().reshape(ref["y"].shape)
    st = X.analyse(o, ref["y"], ref["s"], ref["e"], dtype=dt)
    rate32 = X.ref_rate(ref32.reshape(ref["y"].shape), ref["y"], dt) if ref32 is not None else None
    fails += X.failures(st, exact_fn=assert_rate, ref_rate=rate32, direction=assert_rate)
    row = dict(case=name, family=family, inst="/".join(map(str, key)), dtype=DCODE[dt], n=st["n"], arith_log2=round(math.log2(X.NORM_ARITH[family]), 2),
               stat_log2=round(math.log2(X.NORM_STAT[X.NORM_STAT_FAMILY[family]]), 2), max_ulp=round(st["max_ulp"], 3),
               max_err_over_bound=round(st["max_err_over_tol"], 3), rate=round(st["rate"], 4), ref_rate=None if rate32 is None else round(rate32, 4),
               direction=round(st["direction"], 4), n_dir=st["n_dir"], log2_err_over_S=_log2_err_over_S(o, ref))
    if dt != F32:
        row["clean_share"] = round(X.clean_share(ref, dt), 4)
        if not cancellation and row["clean_share"] < X.CLEAN_SHARE_MIN:
            fails.append(f"clean share {row['clean_share']} < {X.CLEAN_SHARE_MIN}")
    if stat:
        row.update(stat)
    _STATS.append(row)
    print(row)
    if not fails:
        _SEEN.add((key, DCODE[dt], triple))
    return [f"{name} [{family}, {row['dtype']}]: " + "; ".join(fails)] if fails else []


def _log2_err_over_S(o, ref):
    fin = torch.isfinite(o.double())
    e = ((o.double() - ref["y"]).abs() / (X.GELU_D * ref["S"]).clamp_min(1e-300))[fin]
    return round(math.log2(max(float(e.max()) if e.numel() else 0.0, 1e-300)), 2)


def _stat_of_outputs(o, ref, family):
    """For the f32 forms, which expose no statistics: what of |out - y| is left after 1/2 ulp + ARITH S, per unit of Q."""
    y = ref["y"]
    left = (o.double().reshape(y.shape) - y).abs() - 0.5 * X.ulp(y, F32) - X.NORM_ARITH[family] * ref["S"]
    return dict(out_stat_err=float((left.clamp_min(0) / ref["Q"].clamp_min(1e-300)).max()))


def _check(errs):
    assert not errs, "\n".join(errs)


# ================================================================================================ 16-bit GroupNorm
def _gn_ref(x, G, gamma, beta, eps, silu, family, e2=True):
    B, hw, Cc = x.shape
    return X.norm_reference(x.double().view(B, hw, G, Cc // G), gamma.double().view(1, 1, G, -1), beta.double().view(1, 1, G, -1), (1, 3), eps,
                            e2=e2, family=family, act=silu)


def _gn16_run(name, dt, case, x, *, variants, cancellation=False, cols=None, plain=False, family=None, chain=None, beta0=None):
    """One 16-bit GroupNorm case over its (silu, eps) variants: x [B, hw, C] CPU in dt."""
    B, hw, Cc = x.shape
    G, c1 = case["G"], case.get("c1") or Cc
    family = family or case.get("family", "gn16")
    gamma, beta = NC.affine(Cc, beta0=case.get("beta0", 0.0) if beta0 is None else beta0)
    x1 = _tail(x[:, :, :c1].contiguous(), B * hw)
    x2 = _tail(x[:, :, c1:].contiguous(), B * hw) if c1 < Cc else None
    gg, bg = gamma.cuda(), beta.cuda()
    plan = NC.gn16_plan(hw, Cc)
    used = B * G * 2 + (0 if cols else B * plan["ntiles"] * G * 2)
    errs = []
    for silu, eps in variants:
        obuf, out = X.guarded_like((B, hw, Cc), dt, "cuda")
        wbuf, ws = X.guarded_like((B * 129 * G * 2,), F32, "cuda")
        ops.groupnorm(x1, x2, G, eps, silu, gg, bg, out=out, ws=ws, cols1=None if cols is None else cols[0], cols2=None if cols is None else cols[1])
        key = ("gn_cols", 0, 0) if cols else ("gn_stats", 0, 0)
        extra = _expect_launch(name, key, dt, stats_src=1 if cols else 0, **({} if cols else case.get("plan", {})))
        torch.cuda.synchronize()
        if X.sentinels_intact(wbuf, ws[:used]):
            extra.append(f"{X.sentinels_intact(wbuf, ws[:used])} workspace sentinels past the {used} floats in use overwritten")
        ref = _gn_ref(x, G, gamma, beta, eps, silu, family)
        sw = ws[:B * G * 2].view(B, 1, G, 1, 2).cpu()
        se = X.stat_errors(sw[..., 0], sw[..., 1], ref)
        extra += X.stat_failures(se, X.NORM_STAT[family])
        if chain is not None and max(se["mean_err"], se["rstd_err"]) > chain * 2.0 ** -24:
            extra.append(f"statistics error {max(se['mean_err'], se['rstd_err']):.3g} above the chain bound {chain} x 2^-24")
        ref32 = None
        if plain and not silu:
            ref32 = F.group_norm(x.float().permute(0, 2, 1), G, gamma, beta, eps).permute(0, 2, 1).reshape(B, hw, G, Cc // G)
        errs += _judge(f"{name}, silu {silu}, eps {eps:g}", family, key, dt, out, obuf, ref, cancellation=cancellation, ref32=ref32,
                       assert_rate=plain and not silu, extra=extra,
                       stat=dict(mean_err=se["mean_err"], rstd_err=se["rstd_err"], chain=chain))
    return errs


@DT16
@pytest.mark.parametrize("name", list(NC.GN16_CASES))
def test_groupnorm_16_own_statistics(name, dt):
    """Plain cases: N(offset_b, scale_b^2) samples, with and without SiLU, eps 1e-5 and 1e-6; the exact-rounding rate must match
    torch's fp32 group_norm rounded once, the rounding direction be unbiased, and 98 % of the elements be decided by the rounding."""
    c = NC.GN16_CASES[name]
    x = NC.gn_input(2, c["hw"], c["C"], dt, seed=len(name))
    _check(_gn16_run(name, dt, c, x, variants=NC.GN16_VARIANTS, plain=not c.get("cancel"), cancellation=bool(c.get("cancel") or c.get("no_share")),
                     chain=NC.gn16_chain(c["hw"], c["C"], c["G"])))


@DT16
def test_groupnorm_16_probe_rows_and_chunks(dt):
    """x = 0 except one row (tile edges, the partial last stride) or one 8-channel chunk (group edges, the source seam): that row /
    chunk is all the statistics have, so dropping or misplacing it moves every output of the sample far outside the bound."""
    errs = []
    for name, rows in NC.GN16_ROW_PROBES.items():
        c = NC.GN16_CASES[name]
        for p in rows:
            x = NC.gn_input(2, c["hw"], c["C"], dt, seed=p, probe_row=p)
            errs += _gn16_run(f"{name}, only row {p}", dt, c, x, variants=((0, 1e-5),))
    for name, chunks in NC.GN16_CHUNK_PROBES.items():
        c = NC.GN16_CASES[name]
        for q in chunks:
            x = NC.gn_input(2, c["hw"], c["C"], dt, seed=q, probe_chunk=q)
            errs += _gn16_run(f"{name}, only chunk {q}", dt, c, x, variants=((0, 1e-5),))
    _check(errs)


@pytest.mark.parametrize("cname,dt", [(n, d) for n in NC.GN16_CANCEL for d in (BF, FP16) if d == FP16 or "fp16" not in n],
                         ids=lambda v: {BF: "bf16", FP16: "f16"}.get(v, v))
def test_groupnorm_16_cancellation(cname, dt):
    """E[x^2] - mean^2 in fp32 and x * ca + cb without centring, per element: the bound grows with M2 / v (that is Q), and the
    kernels must stay inside it.  At |mean| / std = 3 (the UNet's figure) the clean share must hold as well: that case runs with
    beta offset by 3 and, without the share, at beta ~ 0 (norm_cases.GN16_CANCEL says why)."""
    errs = []
    for name in ("ragged tile: hw 33, C 320, cpg 10, rt 6", "tile cap: hw 4097 -> 33 rows per tile"):
        c = NC.GN16_CASES[name]
        kw = dict(NC.GN16_CANCEL[cname])
        beta0 = kw.pop("beta0", 0.0)
        x = NC.gn_input(2, c["hw"], c["C"], dt, seed=7, **kw)
        errs += _gn16_run(f"{cname}; {name}", dt, c, x, variants=((0, 1e-5), (1, 1e-5)), cancellation=cname != "|mean| / std 3", beta0=beta0)
    _check(errs)


def _column_partials(x, c_lo, c_hi):
    """[B * hw / 128, c, 2] f32: float64 (sum, sum of squares) of every 128-row block and column, rounded to f32."""
    B, hw, _ = x.shape
    blk = x[:, :, c_lo:c_hi].double().view(B * hw // 128, 128, c_hi - c_lo)
    return torch.stack([blk.sum(1), (blk * blk).sum(1)], -1).float().cuda()


@DT16
@pytest.mark.parametrize("name", list(NC.GN16_COLS_CASES))
def test_groupnorm_16_from_synthesised_column_sums(name, dt):
    """k_gn_finalize_cols in isolation: the partials are the float64 column sums rounded to f32."""
    c = NC.GN16_COLS_CASES[name]
    x = NC.gn_input(2, c["hw"], c["C"], dt, seed=len(name))
    c1 = c.get("c1") or c["C"]
    cols = (_column_partials(x, 0, c1), _column_partials(x, c1, c["C"]) if c1 < c["C"] else None)
    _check(_gn16_run(name, dt, c, x, variants=NC.GN16_VARIANTS, cols=cols, plain=True, family="gn16cols",
                     chain=NC.gn16cols_chain(c["hw"], c["C"], c["G"])))


@DT16
def test_groupnorm_16_from_a_producing_gemm(dt):
    """The same with partials a real sdn_gemm_stats_* left behind: the statistics of the 16-bit values that GEMM stored."""
    B, hw, K, N = 2, 128, 64, 320
    g = torch.Generator().manual_seed(17)
    a, w = torch.randn(B * hw, K, generator=g).to(dt).cuda(), (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).cuda()
    cols = torch.zeros(B * hw // 128, N, 2, device="cuda")
    y = ops.gemm(a, w, bias=(0.5 + torch.randn(N, generator=g)).cuda(), col_stats=cols)
    c = dict(hw=hw, C=N, G=32)
    _check(_gn16_run("column sums from sdn_gemm_stats", dt, c, y.cpu().view(B, hw, N), variants=((0, 1e-5), (1, 1e-5)), cols=(cols, None),
                     family="gn16cols", chain=NC.gn16cols_chain(hw, N, 32)))


@DT16
def test_groupnorm_16_rejects_what_it_cannot_tile(dt):
    """C = 2056: 257 chunks, a prime above the 256 threads -> no (ct, nch) split fits LDS: SDN_E_INVALID, nothing written."""
    B, hw, Cc, G = 1, 3, 2056, 8
    assert NC.gn16_plan(hw, Cc) is None
    x = NC.gn_input(B, hw, Cc, dt).cuda()
    gamma, beta = (t.cuda() for t in NC.affine(Cc))
    obuf, out = X.guarded_like((B, hw, Cc), dt, "cuda")
    wbuf, ws = X.guarded_like((B * 129 * G * 2,), F32, "cuda")
    assert ops.groupnorm(x, None, G, 1e-5, 0, gamma, beta, out=out, ws=ws, check=False) == -1
    torch.cuda.synchronize()
    assert X.sentinels_intact(obuf, out[:0]) == 0 and X.sentinels_intact(wbuf, ws[:0]) == 0


# ================================================================================================ 16-bit LayerNorm, adaLN, row statistics
def _ln_ref(x, g, b, eps, family):
    return X.norm_reference(x.double(), g.double(), b.double(), (1,), eps, e2=False, family=family)


def _ln16_run(dt, Cc, rows, *, offset=0.0, eps=1e-5, seed=0):
    """k_layernorm<T, NQ, R>, its adaLN form at rows_per_batch 3 and 5, and k_row_stats<T, NQ, R> on one input."""
    nq, r = NC.ln16_nq_r(Cc)
    x = NC.ln_input(rows, Cc, dt, seed=seed, offset=offset)
    xg = _tail(x, rows)
    gamma, beta = NC.affine(Cc, seed=1)
    tag = f"C {Cc}, rows {rows}" + (f", offset {offset:g}" if offset else "")
    cancel = offset != 0.0
    errs = []
    # row statistics first: they are the STAT measurement of the family
    sbuf, sv = X.guarded_like((rows, 2), F32, "cuda")
    ops.row_stats(xg, eps, out=sv)
    extra = _expect_launch(tag, ("row_stats", nq, r), dt)
    ref = _ln_ref(x, gamma, beta, eps, "ln16")
    torch.cuda.synchronize()
    se = X.stat_errors(sv[:, 0:1].cpu(), sv[:, 1:2].cpu(), ref)
    extra += X.stat_failures(se, X.NORM_STAT["ln16"])
    if X.sentinels_intact(sbuf, sv):
        extra.append("row_stats guard band overwritten")
    chain = NC.ln16_chain(Cc)
    if max(se["mean_err"], se["rstd_err"]) > chain * 2.0 ** -24:
        extra.append(f"statistics error {max(se['mean_err'], se['rstd_err']):.3g} above the chain bound {chain} x 2^-24")
    _STATS.append(dict(case=f"row_stats {tag}", family="ln16", inst=f"row_stats/{nq}/{r}", dtype=DCODE[dt], mean_err=se["mean_err"],
                       rstd_err=se["rstd_err"], chain=chain))
    if extra:
        errs.append(f"row_stats {tag}: " + "; ".join(extra))
    else:
        _SEEN.add((("row_stats", nq, r), DCODE[dt], 0))
    # LayerNorm
    obuf, out = X.guarded_like((rows, Cc), dt, "cuda")
    ops.layernorm(xg, gamma.cuda(), beta.cuda(), eps, out=out)
    extra = _expect_launch(tag, ("layernorm", nq, r), dt)
    ref32 = F.layer_norm(x.float(), (Cc,), gamma, beta, eps)
    errs += _judge(f"layernorm {tag}", "ln16", ("layernorm", nq, r), dt, out, obuf, ref, cancellation=cancel, ref32=ref32, assert_rate=not cancel, extra=extra)
    # adaLN: rows_per_batch 3 and 5 -> a wave's R rows and a workgroup's 4 waves straddle samples
    for rpb in (3, 5):
        nb = (rows + rpb - 1) // rpb
        mod = NC.mod_input(nb, Cc, seed=rpb)
        modg = X.with_nan_tail(mod.cuda(), 1)
        g, b = NC.mod_rows(mod, Cc, rows, rpb)
        refm = _ln_ref(x, g, b, 1e-6, "ln16mod")
        obuf, out = X.guarded_like((rows, Cc), dt, "cuda")
        ops.layernorm_mod(xg, modg[:, Cc:2 * Cc], modg[:, :Cc], rpb, 1e-6, out=out)
        extra = _expect_launch(tag, ("layernorm_mod", nq, r), dt)
        errs += _judge(f"layernorm_mod {tag}, rows_per_batch {rpb}", "ln16mod", ("layernorm_mod", nq, r), dt, out, obuf, refm, cancellation=cancel,
                       extra=extra)
    return errs


@DT16
@pytest.mark.parametrize("Cc", NC.LN16_WIDTHS)
def test_layernorm_16_adaln_and_row_stats(Cc, dt):
    errs = []
    for rows in NC.ln16_rows(Cc):
        errs += _ln16_run(dt, Cc, rows, seed=rows)
    errs += _ln16_run(dt, Cc, NC.ln16_rows(Cc)[1], offset=40.0, seed=5)          # large common offset: the centred sums' case
    _check(errs)


@DT16
def test_layernorm_16_rejects_wide_and_ragged_rows(dt):
    for Cc in (2056, 324):
        x = torch.zeros(4, Cc, dtype=dt, device="cuda")
        gamma, beta = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
        obuf, out = X.guarded_like((4, Cc), dt, "cuda")
        sbuf, sv = X.guarded_like((4, 2), F32, "cuda")
        mod = torch.zeros(2, 3 * Cc, device="cuda")
        assert ops.layernorm(x, gamma, beta, out=out, check=False) == -1
        assert ops.layernorm_mod(x, mod[:, Cc:2 * Cc], mod[:, :Cc], 2, out=out, check=False) == -1
        assert ops.row_stats(x, out=sv, check=False) == -1
        torch.cuda.synchronize()
        assert X.sentinels_intact(obuf, out[:0]) == 0 and X.sentinels_intact(sbuf, sv[:0]) == 0


# ================================================================================================ f32 forms (sdn_f32.hip)
def _gnf32_run(name, kernel, case, *, fields=None):
    """One f32 GroupNorm case, plain (with and without SiLU) and triple; kernel: the form the case is written for."""
    B, hw, Cc, G = 2, case["hw"], case["C"], case["G"]
    c1 = case.get("c1") or Cc
    x = NC.gn_input(B, hw, Cc, F32, seed=len(name))
    gamma, beta = NC.affine(Cc)
    gg, bg = gamma.cuda(), beta.cuda()
    if case.get("misalign"):
        store = torch.empty(B * hw * Cc + 4, device="cuda")
        x1 = store[1:1 + B * hw * Cc].view(B, hw, Cc).copy_(x)
        x2 = None
    else:
        x1 = _tail(x[:, :, :c1].contiguous(), B * hw)
        x2 = _tail(x[:, :, c1:].contiguous(), B * hw) if c1 < Cc else None
    with_ws = kernel == "gn_f32_rows" or case.get("ws")
    key = (kernel, 0, 0)
    errs = []
    plain = {}
    for silu in (0, 1):
        obuf, out = X.guarded_like((B, hw, Cc), F32, "cuda")
        wbuf, ws = X.guarded_like((B * 129 * G * 2,), F32, "cuda") if with_ws else (None, None)
        ops.groupnorm_f32(x1, x2, G, 1e-5, silu, gg, bg, out=out, ws=ws)
        extra = _expect_launch(name, key, F32, triple=0, **(fields or {}))
        torch.cuda.synchronize()
        if with_ws and X.sentinels_intact(wbuf, ws):
            extra.append("workspace guard band overwritten")
        ref = _gn_ref(x, G, gamma, beta, 1e-5, silu, "gnf32")
        stat = _stat_of_outputs(out.cpu(), ref, "gnf32") if not silu else None
        errs += _judge(f"{name}, silu {silu}", "gnf32", key, F32, out, obuf, ref, stat=stat, extra=extra)
        plain[silu] = out.cpu()
    tbuf, tout = X.guarded_like((B * hw, 3, Cc), BF, "cuda")
    wbuf, ws = X.guarded_like((B * 129 * G * 2,), F32, "cuda") if with_ws else (None, None)
    ops.groupnorm_f32(x1, x2, G, 1e-5, 1, gg, bg, out=tout, ws=ws, triple=True)
    extra = _expect_launch(name, key, F32, triple=1, **(fields or {}))
    torch.cuda.synchronize()
    extra += X.check_split_planes(tout.cpu(), plain[1].view(B * hw, Cc), 3)
    if X.sentinels_intact(tbuf, tout):
        extra.append("triple guard band overwritten")
    if extra:
        errs.append(f"{name}, triple: " + "; ".join(extra))
    elif not errs:
        _SEEN.add((key, 2, 1))
    return errs


def test_groupnorm_f32_row_major_form():
    errs = []
    for name, c in NC.GNF32_ROWS_CASES.items():
        rpc, nchunk = NC.gnf32_rpc(c["hw"])
        errs += _gnf32_run(name, "gn_f32_rows", c, fields=dict(rpc=rpc, nchunk=nchunk))
    _check(errs)


def test_groupnorm_f32_pairs_form():
    """k_groupnorm_f32, reached with stats_ws = NULL or C > GN_MAXC."""
    _check([e for name, c in NC.GNF32_PAIRS_CASES.items() for e in _gnf32_run(name, "gn_f32_pairs", c)])


def test_groupnorm_f32_general_form():
    """k_groupnorm_f32_any: odd channels per group, cpg > 512, an odd first source, x off 8-byte alignment."""
    _check([e for name, c in NC.GNF32_ANY_CASES.items() for e in _gnf32_run(name, "gn_f32_any", c)])


def _lnf32_run(kernel, Cc, rows=9):
    x = NC.ln_input(rows, Cc, F32, seed=Cc)
    xg = _tail(x, rows)
    gamma, beta = NC.affine(Cc, seed=2)
    key = (kernel, 0, 0)
    obuf, out = X.guarded_like((rows, Cc), F32, "cuda")
    ops.layernorm(xg, gamma.cuda(), beta.cuda(), 1e-5, out=out)
    extra = _expect_launch(f"C {Cc}", key, F32, triple=0)
    ref = _ln_ref(x, gamma, beta, 1e-5, "lnf32")
    torch.cuda.synchronize()
    errs = _judge(f"{kernel} C {Cc}, rows {rows}", "lnf32", key, F32, out, obuf, ref, stat=_stat_of_outputs(out.cpu(), ref, "lnf32"), extra=extra)
    tbuf, tout = X.guarded_like((rows, 3, Cc), BF, "cuda")
    ops.layernorm(xg, gamma.cuda(), beta.cuda(), 1e-5, out=tout, triple=True)
    extra = _expect_launch(f"C {Cc}", key, F32, triple=1)
    torch.cuda.synchronize()
    extra += X.check_split_planes(tout.cpu(), out.cpu(), 3)
    if X.sentinels_intact(tbuf, tout):
        extra.append("triple guard band overwritten")
    if extra:
        errs.append(f"{kernel} C {Cc}, triple: " + "; ".join(extra))
    elif not errs:
        _SEEN.add((key, 2, 1))
    return errs


def test_layernorm_f32_register_and_generic_forms():
    """k_layernorm_f32_regs at c = 4, 260 (first width with a second v[j]), 1280; k_layernorm_f32 at c = 77 (odd: triple through
    store_triple1), 1284 (past the registers), 1538 (even, not a multiple of 4)."""
    errs = [e for Cc in NC.LNF32_REGS_WIDTHS for rows in (1, 9) for e in _lnf32_run("ln_f32_regs", Cc, rows)]
    errs += [e for Cc in NC.LNF32_GENERIC_WIDTHS for rows in (1, 9) for e in _lnf32_run("ln_f32", Cc, rows)]
    _check(errs)


def test_layernorm_mod_f32():
    """k_layernorm_mod_f32<2 / 4 / 8> with rows_per_batch 3 and 5: the 4 rows of a workgroup straddle samples."""
    errs = []
    rows = 11
    for Cc, nv in NC.LNF32_MOD_WIDTHS.items():
        x = NC.ln_input(rows, Cc, F32, seed=Cc)
        xg = _tail(x, rows)
        for rpb in (3, 5):
            nb = (rows + rpb - 1) // rpb
            mod = NC.mod_input(nb, Cc, seed=rpb)
            modg = X.with_nan_tail(mod.cuda(), 1)
            g, b = NC.mod_rows(mod, Cc, rows, rpb)
            ref = _ln_ref(x, g, b, 1e-6, "lnf32mod")
            obuf, out = X.guarded_like((rows, Cc), F32, "cuda")
            ops.layernorm_mod(xg, modg[:, Cc:2 * Cc], modg[:, :Cc], rpb, 1e-6, out=out)
            extra = _expect_launch(f"C {Cc}", ("ln_mod_f32", nv, 0), F32)
            torch.cuda.synchronize()
            errs += _judge(f"ln_mod_f32 C {Cc}, rows_per_batch {rpb}", "lnf32mod", ("ln_mod_f32", nv, 0), F32, out, obuf, ref,
                           stat=_stat_of_outputs(out.cpu(), ref, "lnf32mod"), extra=extra)
    _check(errs)


# ================================================================================================ coverage
def test_every_norm_instantiation_ran_in_every_dtype():
    """The cases above ran (and passed on) everything the norm launchers can launch: tests_support/exact.py NORM_INSTANTIATIONS,
    16-bit kernels in bf16 and fp16, f32 ones plain and triple."""
    if os.environ.get("SDN_EXACT_STATS"):
        with open(os.environ["SDN_EXACT_STATS"], "w") as f:
            json.dump(_STATS, f, indent=0)
    want = X.norm_coverage_wanted()
    assert _SEEN == want, dict(missing=sorted(map(str, want - _SEEN)), unexpected=sorted(map(str, _SEEN - want)))
