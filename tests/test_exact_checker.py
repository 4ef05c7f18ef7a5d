"""The element-exact GEMM criterion (tests_support/exact.py) on the CPU: round-to-nearest outputs built from float64 references
pass; the defects it exists to catch -- round toward zero, a double-rounded epilogue, one element 2 ulps off, an overwritten
guard band, an unwritten (NaN) tile -- are each rejected.  And the instantiation list the GPU matrix covers is the one
dispatch_dma can launch."""
import os
import re

import pytest
import torch

from tests_support import exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]


def _case(dt, M=512, N=256, K=128, seed=0):
    """Exact y and S of a bias GEMM on 16-bit operands (float64 arithmetic), and the pieces it was made of."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dt).double()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).double()
    bias = torch.randn(N, generator=g).to(dt).double()          # 16-bit-representable, so a 16-bit re-add keeps y the reference
    return a @ w.T, bias, a @ w.T + bias, a.abs() @ w.abs().T + bias.abs()


def _verdict(out, y, s, dt):
    return X.failures(X.analyse(out, y, s), exact_fn=True, ref_rate=X.ref_rate(y.float(), y, dt))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_round_to_nearest_passes(dt):
    _, _, y, s = _case(dt)
    out = X.round_to(y, dt).to(dt)
    assert _verdict(out, y, s, dt) == []
    st = X.analyse(out, y, s)
    assert st["rate"] == 1.0 and st["max_ulp"] <= 0.5 and abs(st["direction"]) < 0.01 and st["n_dir"] >= X.MIN_DIRECTION_ELEMS


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_round_toward_zero_fails(dt):
    _, _, y, s = _case(dt)
    rn, u = X.round_to(y, dt), X.ulp(y, dt)
    out = torch.where(rn.abs() > y.abs(), rn - torch.sign(y) * u, rn).to(dt)      # truncation: never away from zero
    f = _verdict(out, y, s, dt)
    assert any("outside the bound" in m for m in f), f
    assert any("direction" in m for m in f), f
    assert any("rate" in m for m in f), f


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_double_rounded_bias_fails(dt):
    """The epilogue rounds the GEMM to 16 bit, then adds the bias and rounds again."""
    ab, bias, y, s = _case(dt)
    out = X.round_to(X.round_to(ab, dt) + bias, dt).to(dt)
    f = _verdict(out, y, s, dt)
    assert any("outside the bound" in m for m in f), f
    assert any("rate" in m for m in f), f


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_one_element_two_ulps_off_fails(dt):
    _, _, y, s = _case(dt)
    out = X.round_to(y, dt)
    i = int((y[7].abs() - 0.3).abs().argmin())      # a small element (|y| ~ 0.3, a few times below the column scale)
    out[7, i] += 2 * X.ulp(y[7, i], dt)
    f = _verdict(out.to(dt), y, s, dt)
    assert len(f) == 1 and f[0].startswith("1 elements outside the bound"), f


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_unwritten_tile_fails(dt):
    _, _, y, s = _case(dt)
    buf, view = X.guarded(512, 256, dt, "cpu", ldc=264)
    view[:384] = X.round_to(y, dt).to(dt)[:384]
    view[384:, :128] = X.round_to(y, dt).to(dt)[384:, :128]  # the tile [384:, 128:] is never stored: it keeps the sentinel
    assert X.sentinels_intact(buf, view) == 0
    f = _verdict(view, y, s, dt)
    assert any(m.startswith(f"{128 * 128} NaN") for m in f), f


@pytest.mark.parametrize("dt", DTYPES + [torch.float32], ids=["bf16", "f16", "f32"])
def test_overwritten_sentinel_is_found(dt):
    buf, view = X.guarded(100, 40, dt, "cpu", ldc=48)
    view.fill_(1.0)
    assert X.sentinels_intact(buf, view) == 0
    base = view.storage_offset() - buf.storage_offset()
    for pos in (0, base - 1, base + 40, base + 47, base + 99 * 48 + 40, buf.numel() - 1):   # before, ldc gaps, after
        b2 = buf.clone()
        b2[pos] = 0.0
        assert X.sentinels_intact(b2, b2[base:base + 100 * 48].view(100, 48)[:, :40]) == 1, pos
    # a canonical NaN written over the sentinel is a change too (the pattern is compared bit for bit)
    assert torch.isnan(buf[0].float())
    b3 = buf.clone()
    b3[0] = float("nan")
    assert X.sentinels_intact(b3, b3[base:base + 100 * 48].view(100, 48)[:, :40]) == 1


def test_fp16_overflow_and_subnormals():
    dt = torch.float16
    y = torch.tensor([65519.0, 65520.0, -70000.0, 2.0 ** -25, 3 * 2.0 ** -25, 1e-9, 65504.0], dtype=torch.float64)
    z = torch.zeros_like(y)
    rn = X.round_to(y, dt)
    assert rn.tolist() == [65504.0, float("inf"), float("-inf"), 0.0, 2 * 2.0 ** -24, 0.0, 65504.0]
    assert X.failures(X.analyse(rn.to(dt), y, z), exact_fn=False) == []
    for i, v, what in ((1, 65504.0, "overflow"), (0, float("inf"), "overflow"), (4, 2.0 ** -22, "outside")):
        bad = rn.clone()
        bad[i] = v                                   # finite where RN is inf / inf where RN is finite / subnormal 2.5 ulps off
        assert any(what in m for m in X.failures(X.analyse(bad.to(dt), y, z), exact_fn=False)), (i, v)


def test_dispatch_instantiations_match_the_gpu_matrix():
    """Parses the launch_dma<T, ...> instantiations of dispatch_dma (csrc/sdn_gemm.hip): a new one without a case in the GPU
    matrix (tests_support/exact.py INSTANTIATIONS) fails here, on the CPU."""
    src = open(os.path.join(ROOT, "safe_denoiser_amd", "csrc", "sdn_gemm.hip")).read()
    body = re.search(r"\nint dispatch_dma\(.*?\n}\n", src, re.S).group(0)
    found = set()
    for args in re.findall(r"launch_dma<T,\s*([0-9,\s]+)>", body):
        v = [int(x) for x in args.split(",")]
        v += [2, 0][len(v) - 2:]                       # template defaults: NSTAGE = 2, LNF = 0
        found.add(("dma",) + tuple(v))
    assert len(found) >= 10, found
    want = {k for k in X.INSTANTIATIONS if k[0] == "dma"}
    assert found == want, dict(missing_from_matrix=sorted(found - want), not_in_dispatch=sorted(want - found))
    assert {k for k in X.INSTANTIATIONS if k[0] != "dma"} == {("slab",), ("splitk",), ("ffn",)}


# ---- the fp32-storage GEMM forms (bf16x3 and f32): the scheme's own bound, and the faults a whole-matrix norm cannot see ----------
def test_bf16x3_scheme_is_within_three_residuals_of_the_f32_product():
    """|y3 - y| <= 3 * 2^-16 S for y3 = Ahi Whi^T + Alo Whi^T + Ahi Wlo^T against the exact product y of the f32 operands,
    S = |A| |W|^T.  With u = 2^-8 per bf16 rounding: a = hi + lo + r, |lo| <= u |a|, |r| <= u |lo| <= u^2 |a|, so
    a w - (ah wh + al wh + ah wl) = al wl + ra w + (ah + al) rw, each term <= u^2 |a| |w| = 2^-16 |a| |w|.  The operator-level
    3e-5 rel-L2 bounds of tests/test_gpu_f32.py / test_gpu_x3t.py (= 2^-15.0) rest on this property; the kernels themselves are
    held to accumulation error against y3 (tests/test_gpu_x3_exact.py)."""
    g = torch.Generator().manual_seed(3)
    M, N, K = 400, 96, 192
    a = torch.randn(M, K, generator=g) * torch.exp2(torch.arange(M, dtype=torch.float32) % 40 - 26.0)[:, None]   # 2^-26 ... 2^13
    a[::7] = torch.randn(M, K, generator=g)[::7]                                                                  # and unscaled rows
    w = torch.randn(N, K, generator=g) * K ** -0.5
    A, W = a.double(), w.double()
    A3, W3 = X.x3_operands(A, W)
    assert A3.shape == (M, 3 * K) and torch.equal(A3[:, :K], A3[:, 2 * K:]) and torch.equal(W3[:, :K], W3[:, K:2 * K])
    y, y3, s = A @ W.T, A3 @ W3.T, A.abs() @ W.abs().T
    ratio = float(((y3 - y).abs() / s).max())
    assert 2.0 ** -22 < ratio <= X.SCHEME_REL, ratio          # (and not vacuous: the scheme's error is really there)
    # exactly representable operands have no lo: the scheme is then exact
    A3b, W3b = X.x3_operands(a.bfloat16().double(), w.bfloat16().double())
    assert not bool(A3b[:, K:2 * K].any()) and torch.equal(A3b @ W3b.T, a.bfloat16().double() @ w.bfloat16().double().T)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def x3_emulation():
    """One bf16x3 GEMM as the kernels run it, emulated on the CPU: out = RN_f32(y3 + bias + residual) over n_valid = N - 28 columns
    of a 4113 x 320 problem (ragged last row tile: 17 rows).  The residual of the three samples differs by ~1e-4 between samples
    and the weight row of the last (padding) column by ~1e-4 from the last valid one: the small differences a real plan has
    between neighbouring samples / a clamped neighbour.  Shared by the planted-fault tests, never modified."""
    g = torch.Generator().manual_seed(11)
    M, N, K, nv, rpb = 4113, 320, 192, 292, 1371
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w[N - 1] = w[nv - 1] * (1 + 1e-4 * torch.randn(K, generator=g))
    bias = torch.randn(N, generator=g).double()
    res = (torch.randn(rpb, nv, generator=g).repeat(3, 1) * (1 + 1e-4 * torch.randn(M, nv, generator=g))).double()
    A, W = a.double(), w.double()
    A3, W3 = X.x3_operands(A, W)
    y3 = (A3 @ W3.T + bias)[:, :nv] + res
    s3 = (A3.abs() @ W3.abs().T + bias.abs())[:, :nv] + res.abs()
    ref = (A @ W.T + bias)[:, :nv] + res                        # what the old whole-matrix tests compare with
    return dict(M=M, N=N, K=K, nv=nv, rpb=rpb, A3=A3, W3=W3, res=res, y3=y3, s3=s3, ref=ref, out=y3.float())


def _x3_verdict(out, em):
    return X.failures(X.analyse(out, em["y3"], em["s3"], dtype=torch.float32, acc=max(X.X3_ACC.values())), exact_fn=False, direction=False)


def test_x3_emulated_kernel_passes_both_criteria(x3_emulation):
    em = x3_emulation
    assert _x3_verdict(em["out"], em) == []
    assert _rel_l2(em["out"], em["ref"]) <= 3e-5


def test_x3_dropped_lo_term_in_one_fragment_is_found_where_the_norm_is_blind(x3_emulation):
    em = x3_emulation
    K, r, c = em["K"], slice(4096, 4112), slice(32, 48)         # one 16 x 16 fragment of the ragged row tile
    out = em["out"].clone()
    out[r, c] = (em["y3"][r, c] - em["A3"][r, K:2 * K] @ em["W3"][c, K:2 * K].T).float()      # a_lo . w_hi never accumulated
    f = _x3_verdict(out, em)
    assert len(f) == 1 and "outside the bound" in f[0] and int(f[0].split()[0]) > 200, f
    assert _rel_l2(out, em["ref"]) <= 3e-5


def test_x3_tail_column_from_the_clamped_neighbour_is_found_where_the_norm_is_blind(x3_emulation):
    em = x3_emulation
    N, nv = em["N"], em["nv"]
    out = em["out"].clone()
    out[:, nv - 1] = (em["y3"][:, nv - 1] + em["A3"] @ (em["W3"][N - 1] - em["W3"][nv - 1])).float()  # column N - 1's weight row
    f = _x3_verdict(out, em)
    assert len(f) == 1 and "outside the bound" in f[0] and int(f[0].split()[0]) > em["M"] // 2, f
    assert _rel_l2(out, em["ref"]) <= 3e-5


def test_x3_residual_row_of_the_next_sample_is_found_where_the_norm_is_blind(x3_emulation):
    em = x3_emulation
    m = 700
    out = em["out"].clone()
    out[m] = (em["y3"][m] - em["res"][m] + em["res"][m + em["rpb"]]).float()
    f = _x3_verdict(out, em)
    assert len(f) == 1 and "outside the bound" in f[0] and int(f[0].split()[0]) > em["nv"] // 2, f
    assert _rel_l2(out, em["ref"]) <= 3e-5


def test_x3_unwritten_fragment_and_ldc_gap_store_are_found_where_the_old_harness_is_blind(x3_emulation):
    em = x3_emulation
    M, nv = em["M"], em["nv"]
    r, c = slice(4096, 4112), slice(32, 48)
    # the old harness: torch.empty hands back the previous call's identical result, a contiguous [M, n_valid] view has no gap
    old = em["out"].clone()                                      # (allocator reuse: the buffer still holds a correct result)
    written = torch.ones(M, nv, dtype=torch.bool); written[r, c] = False
    old[written] = em["out"][written]
    assert _rel_l2(old, em["ref"]) <= 3e-5
    # the new one: a sentinel-NaN f32 buffer with an ldc gap
    buf, view = X.guarded(M, nv, torch.float32, "cpu", ldc=nv + 4)
    view[written] = em["out"][written]
    assert X.sentinels_intact(buf, view) == 0
    f = _x3_verdict(view, em)
    assert any(m.startswith("256 NaN") for m in f), f
    view[r, c] = em["out"][r, c]
    assert _x3_verdict(view, em) == [] and X.sentinels_intact(buf, view) == 0
    buf[view.storage_offset() + 5 * (nv + 4) + nv] = 0.25        # one element stored into the ldc gap of row 5
    assert X.sentinels_intact(buf, view) == 1
    assert _rel_l2(view, em["ref"]) <= 3e-5                      # the values themselves are all right: the norm has nothing to see


def test_split_planes_check_and_plane_guards():
    """check_split_planes accepts the split of an f32 result and names the plane that is off; guarded_planes guards every gap."""
    g = torch.Generator().manual_seed(5)
    f = torch.randn(40, 24, generator=g) * torch.exp2(torch.arange(40, dtype=torch.float32) % 40 - 26.0)[:, None]
    hi = f.bfloat16(); lo = (f - hi.float()).bfloat16()
    for planes in (2, 3):
        buf, view = X.guarded_planes(40, planes, 24, torch.bfloat16, "cpu", ldc=28)
        view[:, 0], view[:, 1] = hi, lo
        if planes == 3:
            view[:, 2] = hi
        assert X.check_split_planes(view, f, planes) == [] and X.sentinels_intact(buf, view) == 0
        v2 = view.clone(); v2[3, 1, 4] = (f[3, 4] - hi[3, 4].float()).bfloat16() * 1.01 + 1e-30
        assert any("lo plane" in m for m in X.check_split_planes(v2, f, planes))
        v3 = view.clone(); v3[7, 0, 2] = hi[7, 2] * 1.01
        assert any("hi plane" in m for m in X.check_split_planes(v3, f, planes))
        base = view.storage_offset()
        for pos in (base - 1, base + 24, base + 28 + 27, base + 40 * planes * 28):       # before, both kinds of gap, after
            b2 = buf.clone(); b2[pos] = 0.0
            assert X.sentinels_intact(b2, b2[base:base + 40 * planes * 28].view(40, planes, 28)[:, :, :24]) == 1, pos


def test_x3t_instantiation_list_is_the_plain_part_of_the_16_bit_one():
    """The triple-operand path reaches the plain k_gemm_dma tiles and the slab ring, nothing else (exact.py says why)."""
    assert set(X.X3T_INSTANTIATIONS) == {k for k in X.INSTANTIATIONS if k[0] == "dma" and k[4] == 0} | {("slab",)}


# ---- the normalisation kernels: the dispatch lists, the constants' hard bounds, emulations and planted faults --------------------
from tests_support import norm_cases as NC  # noqa: E402


def _src(name):
    return open(os.path.join(ROOT, "safe_denoiser_amd", "csrc", name)).read()


def _body(src, head):
    """The function whose definition starts with `head`, up to the first line that is a lone closing brace."""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_norm_dispatch_matches_the_instantiation_list():
    """Parses the launchers of sdn_norm.hip and sdn_f32.hip: the template instantiations and kernel forms they can launch are the
    NORM_INSTANTIATIONS the GPU matrix covers, every launch site leaves a record, and no normalisation kernel exists outside them."""
    norm, f32 = _src("sdn_norm.hip"), _src("sdn_f32.hip")
    pairs = lambda body, macro: {(int(a), int(b)) for a, b in re.findall(macro + r"\((\d+),\s*(\d+)\);", body)}
    launched = lambda body: set(re.findall(r"hipLaunchKernelGGL\(\(?(k_\w+)", body))
    found = set()
    ln = _body(norm, "int layernorm_impl(")
    assert "record_norm_launch({mod ? 4 : 3, T::kDtype, NQ, R," in ln and launched(ln) == {"k_layernorm"}
    found |= {(k, nq, r) for k in ("layernorm", "layernorm_mod") for nq, r in pairs(ln, "SDN_LN_LAUNCH")}
    assert "layernorm_impl<T>(x, rows, c, eps, scale, shift, out, stream, 1, rows_per_batch, ld_mod)" in norm      # adaLN = mod 1
    rs = _body(norm, "int row_stats_impl(")
    assert "record_norm_launch({5, T::kDtype, NQ, R," in rs and launched(rs) == {"k_row_stats"}
    found |= {("row_stats", nq, r) for nq, r in pairs(rs, "SDN_RS_LAUNCH")}
    gn = _body(norm, "int groupnorm_impl(")
    assert launched(gn) == {"k_gn_finalize_cols", "k_gn_stats", "k_gn_finalize", "k_gn_apply"}
    assert "record_norm_launch({2, T::kDtype," in gn and "record_norm_launch({1, T::kDtype, 0, 0, nch, ct, ntiles, rows_per_tile," in gn
    found |= {("gn_stats", 0, 0), ("gn_cols", 0, 0)}
    gf = _body(f32, "static int groupnorm_f32_impl(")
    assert launched(gf) == {"k_gn_rows_stats", "k_gn_rows_apply", "k_groupnorm_f32", "k_groupnorm_f32_any"}
    assert "record_norm_launch({6, 2, 0, 0, 0, 0, 0, 0, rpc, nchunk, 0, triple})" in gf and "record_norm_launch({pairs ? 7 : 8, 2," in gf
    found |= {("gn_f32_rows", 0, 0), ("gn_f32_pairs", 0, 0), ("gn_f32_any", 0, 0)}
    lf = _body(f32, "static int layernorm_f32_impl(")
    assert launched(lf) == {"k_layernorm_f32_regs", "k_layernorm_f32"} and "record_norm_launch({regs ? 9 : 10, 2," in lf
    found |= {("ln_f32_regs", 0, 0), ("ln_f32", 0, 0)}
    lm = _body(f32, 'extern "C" int sdn_layernorm_mod_f32(')
    assert launched(lm) == {"k_layernorm_mod_f32<NV>"} or launched(lm) == {"k_layernorm_mod_f32"}
    assert "record_norm_launch({11, 2, NV," in lm
    found |= {("ln_mod_f32", int(nv), 0) for nv in re.findall(r"SDN_LNM_F32\((\d+)\);", lm)}
    assert found == set(X.NORM_INSTANTIATIONS), dict(missing_from_matrix=sorted(found - set(X.NORM_INSTANTIATIONS)),
                                                     not_in_dispatch=sorted(set(X.NORM_INSTANTIATIONS) - found))
    # the widths at which the GPU cases switch instantiation are the launchers' thresholds
    assert "if (c <= 512) SDN_LN_LAUNCH(1, 4);" in ln and "else if (c <= 1024) SDN_LN_LAUNCH(2, 2);" in ln
    assert [NC.ln16_nq_r(c) for c in (512, 520, 1024, 1032)] == [(1, 4), (2, 2), (2, 2), (4, 1)]
    # every normalisation kernel of the two files is launched by one of the launchers above
    kernels = {k for src in (norm, f32) for k in re.findall(r"\n(k_\w+)\(", src) if re.search(r"norm|k_gn_|row_stats", k)}
    assert kernels == {"k_gn_stats", "k_gn_finalize", "k_gn_finalize_cols", "k_gn_apply", "k_layernorm", "k_row_stats", "k_groupnorm_f32",
                       "k_groupnorm_f32_any", "k_gn_rows_stats", "k_gn_rows_apply", "k_layernorm_f32", "k_layernorm_f32_regs",
                       "k_layernorm_mod_f32"}, kernels
    assert sorted(X.NORM_KERNEL) == list(range(1, 12)) and X.norm_coverage_wanted() and len(X.NL_FIELDS) == 12
    assert "enum { SDN_NL_KERNEL, SDN_NL_DTYPE, SDN_NL_NQ, SDN_NL_R, SDN_NL_NCH, SDN_NL_CT, SDN_NL_NTILES, SDN_NL_ROWS_PER_TILE, SDN_NL_RPC," in _src("sdn_ops.h")
    assert "sdn_debug_norm_last_launch" not in open(os.path.join(ROOT, "include", "sdn.h")).read()


def test_norm_launch_plans_restate_the_launcher():
    """norm_cases.gn16_plan against the arithmetic of groupnorm_impl as written, and the shapes the issue names."""
    gn = _body(_src("sdn_norm.hip"), "int groupnorm_impl(")
    for line in ("int nch = (cch + THREADS - 1) / THREADS;", "while (cch % nch != 0) ++nch;", "if (ct > THREADS) return SDN_E_INVALID;",
                 "int ntiles = (hw + 31) / 32;", "if (ntiles > GN_MAX_TILES) ntiles = GN_MAX_TILES;",
                 "const int rows_per_tile = (hw + ntiles - 1) / ntiles;", "if (lds > 64 * 1024) return SDN_E_INVALID;"):
        assert line in gn, line
    for c in NC.GN16_CASES.values():
        p = NC.gn16_plan(c["hw"], c["C"])
        assert all(p[k] == v for k, v in c["plan"].items()), (c, p)
    assert NC.gn16_plan(33, 2056) is None and NC.gn16_plan(33, 320)["rt"] == 6 and NC.gn16_plan(33, 4096)["rt"] == 1
    assert NC.gnf32_rpc(1025) == (32, 33) and NC.gnf32_rpc(2049) == (64, 33) and NC.gnf32_rpc(17) == (16, 2)


def test_norm_constants_stay_below_their_hard_bounds():
    """ARITH <= 8 roundings; every family's STAT below (longest serial fp32 chain of its statistics) x 2^-24, and not below the
    2^-24 of a single rounding."""
    assert all(v <= 8 * 2.0 ** -24 for v in X.NORM_ARITH.values())
    chains = NC.stat_chains()
    assert set(chains) == set(X.NORM_STAT)
    for fam, stat in X.NORM_STAT.items():
        assert 2.0 ** -24 <= stat < chains[fam] * 2.0 ** -24, (fam, stat, chains[fam])


def _gn_ref(x, G, gamma, beta, eps, silu, family="gn16"):
    B, hw, Cc = x.shape
    return X.norm_reference(x.double().view(B, hw, G, Cc // G), gamma.double().view(1, 1, G, -1), beta.double().view(1, 1, G, -1), (1, 3), eps,
                            e2=True, family=family, act=silu)


def _norm_verdict(out, ref, dt, *, mean=None, rstd=None, family=None, ref32=None):
    st = X.analyse(out.reshape(ref["y"].shape), ref["y"], ref["s"], ref["e"], dtype=dt)
    f = X.failures(st, exact_fn=ref32 is not None, ref_rate=None if ref32 is None else X.ref_rate(ref32.reshape(ref["y"].shape), ref["y"], dt))
    if mean is not None:
        f += X.stat_failures(X.stat_errors(mean.reshape(ref["mu"].shape), rstd.reshape(ref["mu"].shape), ref), X.NORM_STAT[family])
    return f


GN_EMU_CASES = ["ragged tile: hw 33, C 320, cpg 10, rt 6", "tile cap: hw 4097 -> 33 rows per tile", "uneven tiles: hw 100, G 1",
                "two sources 320 + 640, seam inside group 10", "prime chunk count: C 1928 (241 chunks), G 8"]


@pytest.fixture(scope="module")
def gn_emulation_inputs():
    """The GPU tests' own inputs and float64 references of the emulated GroupNorm cases, per (case, dtype); never modified."""
    made = {}
    for name in GN_EMU_CASES:
        c = NC.GN16_CASES[name]
        for dt in DTYPES:
            x = NC.gn_input(2, c["hw"], c["C"], dt, seed=len(name))
            gamma, beta = NC.affine(c["C"], beta0=c.get("beta0", 0.0))
            fam = c.get("family", "gn16")
            made[name, dt] = dict(x=x, gamma=gamma, beta=beta, G=c["G"], family=fam,
                                  ref={s: _gn_ref(x, c["G"], gamma, beta, 1e-5, s, family=fam) for s in (0, 1)})
    return made


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", GN_EMU_CASES)
def test_groupnorm_emulation_passes_the_criterion(gn_emulation_inputs, name, dt):
    """fp32 arithmetic with the kernel's summation structure (per-tile partials, serial group reduction, 8-share finalize,
    E[x^2] - mean^2, x * ca + cb) on the GPU cases' inputs: inside the bound, statistics inside theirs, clean share >= 98 %."""
    em = gn_emulation_inputs[name, dt]
    for silu in (0, 1):
        out, mean, rstd = NC.emulate_gn16(em["x"], em["G"], 1e-5, em["gamma"], em["beta"], silu, dt)
        assert _norm_verdict(out, em["ref"][silu], dt, mean=mean, rstd=rstd, family=em["family"]) == [], (name, silu)
        assert X.clean_share(em["ref"][silu], dt) >= X.CLEAN_SHARE_MIN


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("fault", ["drop_row", "next_group_chunk", "n_minus_1", "eps_outside", "affine_shift", "rtz"])
def test_groupnorm_planted_fault_is_found(gn_emulation_inputs, fault, dt):
    """Each fault the relative-L2 tests cannot see must be rejected, at the ragged-tile shape and at the hw = 4097 one."""
    for name in GN_EMU_CASES[:2]:
        em = gn_emulation_inputs[name, dt]
        out, mean, rstd = NC.emulate_gn16(em["x"], em["G"], 1e-5, em["gamma"], em["beta"], 0, dt, fault=fault)
        f = _norm_verdict(out, em["ref"][0], dt, mean=mean, rstd=rstd, family="gn16")
        assert f, (fault, name)
        if fault in ("drop_row", "next_group_chunk", "affine_shift", "rtz"):
            assert any("outside the bound" in m for m in f), f
        if fault in ("drop_row", "n_minus_1", "eps_outside"):
            assert any("outside the bound (worst" in m and ("means" in m or "rstd" in m) for m in f), f
        if fault == "rtz" and em["x"].numel() >= 5 * X.MIN_DIRECTION_ELEMS:
            assert any("direction" in m for m in f), f
        if fault == "drop_row" and "4097" in name:          # ... where the old criterion has nothing to see
            assert _rel_l2(out, em["ref"][0]["y"].reshape(out.shape)) <= (4e-3 if dt == torch.bfloat16 else 5e-4)      # test_gpu_ops.py's bounds


LN_EMU = [(320, 33), (768, 17), (2048, 9)]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_layernorm_emulation_passes_and_planted_faults_are_found(dt):
    """k_layernorm / adaLN / k_row_stats in fp32 with the lane-strided sums and the butterfly: inside the bound; the n - 1 variance,
    eps outside the root, gamma / beta one channel off, the next sample's scale on a sample's last row and truncating stores are not."""
    for Cc, rows in LN_EMU:
        x = NC.ln_input(rows, Cc, dt, seed=rows)
        gamma, beta = NC.affine(Cc, seed=1)
        ref = X.norm_reference(x.double(), gamma.double(), beta.double(), (1,), 1e-5, e2=False, family="ln16")
        ref32 = torch.nn.functional.layer_norm(x.float(), (Cc,), gamma, beta, 1e-5)
        out, mean, rstd = NC.emulate_ln16(x, gamma, beta, 1e-5, dt)
        assert _norm_verdict(out, ref, dt, mean=mean, rstd=rstd, family="ln16", ref32=ref32) == [], Cc
        assert X.clean_share(ref, dt) >= X.CLEAN_SHARE_MIN
        for fault in ("n_minus_1", "eps_outside", "affine_shift", "rtz"):
            out, mean, rstd = NC.emulate_ln16(x, gamma, beta, 1e-5, dt, fault=fault)
            assert _norm_verdict(out, ref, dt, mean=mean, rstd=rstd, family="ln16", ref32=ref32), (Cc, fault)
        rpb = 5
        mod = NC.mod_input((rows + rpb - 1) // rpb, Cc, seed=rpb)
        g, b = NC.mod_rows(mod, Cc, rows, rpb)
        refm = X.norm_reference(x.double(), g, b, (1,), 1e-6, e2=False, family="ln16mod")
        b_of = torch.arange(rows) // rpb
        scale, shift = mod[b_of, Cc:2 * Cc], mod[b_of, :Cc]
        assert _norm_verdict(NC.emulate_ln16(x, scale, shift, 1e-6, dt, mod=True)[0], refm, dt) == [], Cc
        if rows > rpb:
            bad = NC.emulate_ln16(x, scale, shift, 1e-6, dt, mod=True, fault="next_sample_scale", rows_per_batch=rpb)[0]
            f = _norm_verdict(bad, refm, dt)
            assert len(f) == 1 and "outside the bound" in f[0], f


def test_f32_form_emulations_pass_the_criterion():
    """The f32 forms: double statistics rounded once (GroupNorm), lane-strided f32 sums (LayerNorm, adaLN); f32 outputs have no
    16-bit rounding to hide behind, so the bound is 1/2 ulp_f32 + ARITH S + STAT Q alone."""
    c = NC.GNF32_ROWS_CASES["rows: hw 17, 320 + 640"]
    x = NC.gn_input(2, c["hw"], c["C"], torch.float32, seed=4)
    gamma, beta = NC.affine(c["C"])
    for silu in (0, 1):
        ref = _gn_ref(x, c["G"], gamma, beta, 1e-5, silu, family="gnf32")
        assert _norm_verdict(NC.emulate_gnf32(x, c["G"], 1e-5, gamma, beta, silu), ref, torch.float32) == []
    for Cc in (77, 260, 1538):
        x = NC.ln_input(9, Cc, torch.float32, seed=Cc)
        gamma, beta = NC.affine(Cc, seed=2)
        ref = X.norm_reference(x.double(), gamma.double(), beta.double(), (1,), 1e-5, e2=False, family="lnf32")
        assert _norm_verdict(NC.emulate_lnf32(x, gamma, beta, 1e-5), ref, torch.float32) == [], Cc
        bad = NC.emulate_lnf32(x, torch.roll(gamma, 1), beta, 1e-5)
        assert _norm_verdict(bad, ref, torch.float32), Cc
