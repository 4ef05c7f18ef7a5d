"""The LayerNorm forms for rows of 2049 .. 2560 columns (SD-3.5-large is 2432 wide) -- k_layernorm<T, 5, 1>, its adaLN form and
k_row_stats<T, 5, 1> of sdn_norm.hip in bf16 and fp16, k_layernorm_mod_f32<10> of sdn_f32.hip -- element by element against float64
arithmetic on the values the kernel reads, by the criterion of tests/test_gpu_norm_exact.py (tests_support/exact.py,
"Normalisation kernels"):

    |out - f(y)| <= 1/2 ulp_T(f(y)) + ARITH S + STAT Q

with the constants of the ln16 / ln16mod / lnf32mod families unchanged, and the statistics k_row_stats exposes inside the chain bound
of a lane's 8 x 5 elements, 6 butterfly steps and the division: 47 x 2^-24.
Widths: 2176 = 17 x 128, the first above the old limit (the fifth chunk has 16 of 64 lanes live); 2432 (48 live); 2560 (a full fifth
chunk).  Rows 1, 3, 5, 261: a lone row, partial workgroups of 4 waves, and 66 workgroups.  Outputs are views into NaN-sentinel buffers
whose bands start right behind column c of the last row (for rows = 1: right behind the one row), inputs carry a NaN row behind their
extent, the modulation rows have leading dimension 3 c with NaN behind the last sample.  Every case asserts from
sdn_debug_norm_last_launch that the wide form ran; the last test asserts that all of WIDE_INSTANTIATIONS did, in every dtype."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safe_denoiser_amd as sda
from tests_support import exact as X
from tests_support import norm_cases as NC
from tests_support import ops

pytestmark = pytest.mark.gpu
F32, BF, FP16 = torch.float32, torch.bfloat16, torch.float16
DCODE = {BF: 0, FP16: 1, F32: 2}
WIDTHS, ROWS, RPB = (2176, 2432, 2560), (1, 3, 5, 261), (3, 5)
CHAIN = 8 * 5 + 6 + 1
# (NORM_INSTANTIATIONS-style key, dtype code) of the forms this file is about -- kept apart from tests_support/exact.py's table,
# which tests/test_gpu_norm_exact.py compares with its own cases
WIDE_INSTANTIATIONS = {(("layernorm", 5, 1), 0), (("layernorm", 5, 1), 1), (("layernorm_mod", 5, 1), 0), (("layernorm_mod", 5, 1), 1),
                       (("row_stats", 5, 1), 0), (("row_stats", 5, 1), 1), (("ln_mod_f32", 10, 0), 2)}
_SEEN = set()


def _ran(key, dt):
    rec = (C.c_int * len(X.NL_FIELDS))()
    sda.lib().sdn_debug_norm_last_launch(rec, len(X.NL_FIELDS))
    rec = list(rec)
    got = (X.norm_launch_key(rec), rec[1])
    return [] if got == (key, DCODE[dt]) else [f"written for {key} dtype {DCODE[dt]}, ran {got}"]


def _ref(x, g, b, eps, family):
    return X.norm_reference(x.double(), g.double(), b.double(), (1,), eps, e2=False, family=family)


def _judge(name, family, key, dt, out, buf, ref, *, cancellation=False, ref32=None, extra=()):
    torch.cuda.synchronize()
    fails = list(extra)
    bad = X.sentinels_intact(buf, out)
    if bad:
        fails.append(f"{bad} guard-band sentinels overwritten")
    o = out.cpu()
    st = X.analyse(o, ref["y"], ref["s"], ref["e"], dtype=dt)
    rate32 = X.ref_rate(ref32, ref["y"], dt) if ref32 is not None else None
    fails += X.failures(st, exact_fn=ref32 is not None, ref_rate=rate32, direction=ref32 is not None)
    share = X.clean_share(ref, dt) if dt != F32 else None
    print(dict(case=name, inst="/".join(map(str, key)), dtype=DCODE[dt], n=st["n"], max_ulp=round(st["max_ulp"], 3),
               max_err_over_bound=round(st["max_err_over_tol"], 3), rate=round(st["rate"], 4), clean_share=share))
    if share is not None and not cancellation and share < X.CLEAN_SHARE_MIN:
        fails.append(f"clean share {share:.4f} < {X.CLEAN_SHARE_MIN}")
    if not fails:
        _SEEN.add((key, DCODE[dt]))
    return [f"{name} [{family}]: " + "; ".join(fails)] if fails else []


def _tail(x):
    return X.with_nan_tail(x.cuda(), 1)


def _mod_case(x, Cc, rows, rpb):
    """Stacked modulation [nb, 3 c] (ld_mod = 3 c > c) with a NaN row behind the last sample, and its float64 (1 + scale, shift) rows."""
    nb = (rows + rpb - 1) // rpb
    mod = NC.mod_input(nb, Cc, seed=rpb)
    g, b = NC.mod_rows(mod, Cc, rows, rpb)
    return X.with_nan_tail(mod.cuda(), 1), g, b


def _run16(dt, Cc, rows, *, offset=0.0, seed=0):
    x = NC.ln_input(rows, Cc, dt, seed=seed, offset=offset)
    xg = _tail(x)
    gamma, beta = NC.affine(Cc, seed=1)
    tag = f"C {Cc}, rows {rows}" + (f", offset {offset:g}" if offset else "")
    cancel = offset != 0.0
    errs = []
    # row statistics: the family's STAT constant and the chain bound of the NQ = 5 form
    sbuf, sv = X.guarded_like((rows, 2), F32, "cuda")
    ops.row_stats(xg, 1e-5, out=sv)
    extra = _ran(("row_stats", 5, 1), dt)
    ref = _ref(x, gamma, beta, 1e-5, "ln16")
    torch.cuda.synchronize()
    se = X.stat_errors(sv[:, 0:1].cpu(), sv[:, 1:2].cpu(), ref)
    extra += X.stat_failures(se, X.NORM_STAT["ln16"])
    if X.sentinels_intact(sbuf, sv):
        extra.append("row_stats guard band overwritten")
    worst = max(se["mean_err"], se["rstd_err"])
    print(dict(case=f"row_stats {tag}", dtype=DCODE[dt], mean_err_x2p24=round(se["mean_err"] * 2 ** 24, 3),
               rstd_err_x2p24=round(se["rstd_err"] * 2 ** 24, 3), chain=CHAIN))
    if worst > CHAIN * 2.0 ** -24:
        extra.append(f"statistics error {worst:.3g} above the chain bound {CHAIN} x 2^-24")
    if extra:
        errs.append(f"row_stats {tag}: " + "; ".join(extra))
    else:
        _SEEN.add((("row_stats", 5, 1), DCODE[dt]))
    # LayerNorm
    obuf, out = X.guarded_like((rows, Cc), dt, "cuda")
    ops.layernorm(xg, gamma.cuda(), beta.cuda(), 1e-5, out=out)
    ref32 = None if cancel else F.layer_norm(x.float(), (Cc,), gamma, beta, 1e-5)
    errs += _judge(f"layernorm {tag}", "ln16", ("layernorm", 5, 1), dt, out, obuf, ref, cancellation=cancel, ref32=ref32,
                   extra=_ran(("layernorm", 5, 1), dt))
    # adaLN, rows_per_batch 3 and 5: a workgroup's 4 waves straddle samples
    for rpb in RPB:
        modg, g, b = _mod_case(x, Cc, rows, rpb)
        refm = _ref(x, g, b, 1e-6, "ln16mod")
        obuf, out = X.guarded_like((rows, Cc), dt, "cuda")
        ops.layernorm_mod(xg, modg[:, Cc:2 * Cc], modg[:, :Cc], rpb, 1e-6, out=out)
        errs += _judge(f"layernorm_mod {tag}, rows_per_batch {rpb}", "ln16mod", ("layernorm_mod", 5, 1), dt, out, obuf, refm,
                       cancellation=cancel, extra=_ran(("layernorm_mod", 5, 1), dt))
    return errs


@pytest.mark.parametrize("dt", [BF, FP16], ids=["bf16", "f16"])
@pytest.mark.parametrize("Cc", WIDTHS)
def test_layernorm_16_adaln_and_row_stats_wide(Cc, dt):
    errs = []
    for rows in ROWS:
        errs += _run16(dt, Cc, rows, seed=rows)
    errs += _run16(dt, Cc, 5, offset=40.0, seed=5)                    # large common offset: the centred sums' case
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("Cc", WIDTHS)
def test_layernorm_mod_f32_wide(Cc):
    """k_layernorm_mod_f32<10>: 40 f32 per lane; at 2176 the last two float4 of a lane are dead in every lane but 32 of j = 8."""
    errs = []
    for rows, offset in [(r, 0.0) for r in ROWS] + [(5, 40.0)]:
        x = NC.ln_input(rows, Cc, F32, seed=Cc + rows, offset=offset)
        xg = _tail(x)
        for rpb in RPB:
            modg, g, b = _mod_case(x, Cc, rows, rpb)
            ref = _ref(x, g, b, 1e-6, "lnf32mod")
            obuf, out = X.guarded_like((rows, Cc), F32, "cuda")
            ops.layernorm_mod(xg, modg[:, Cc:2 * Cc], modg[:, :Cc], rpb, 1e-6, out=out)
            errs += _judge(f"ln_mod_f32 C {Cc}, rows {rows}, rows_per_batch {rpb}" + (f", offset {offset:g}" if offset else ""), "lnf32mod",
                           ("ln_mod_f32", 10, 0), F32, out, obuf, ref, extra=_ran(("ln_mod_f32", 10, 0), F32))
    assert not errs, "\n".join(errs)


def test_rows_of_at_most_2048_keep_their_instantiation():
    for dt in (BF, FP16):
        x = torch.zeros(4, 2048, dtype=dt, device="cuda")
        ops.layernorm(x, torch.ones(2048, device="cuda"), torch.zeros(2048, device="cuda"))
        assert not _ran(("layernorm", 4, 1), dt)
        ops.row_stats(x)
        assert not _ran(("row_stats", 4, 1), dt)
    x = torch.zeros(4, 2048, device="cuda")
    mod = torch.zeros(1, 3 * 2048, device="cuda")
    ops.layernorm_mod(x, mod[:, 2048:4096], mod[:, :2048], 4)
    assert not _ran(("ln_mod_f32", 8, 0), F32)


def test_every_wide_form_ran_in_every_dtype():
    """Reads the module-level _SEEN the tests above fill, as tests/test_gpu_norm_exact.py's coverage test does: it is meant for a
    run of the whole file in order and fails under -k, -x after a failure, or a reordering."""
    assert _SEEN == WIDE_INSTANTIATIONS, dict(missing=sorted(map(str, WIDE_INSTANTIATIONS - _SEEN)), unexpected=sorted(map(str, _SEEN - WIDE_INSTANTIATIONS)))
