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
