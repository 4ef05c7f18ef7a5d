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
