"""k_ffn320 (csrc/sdn_ffn.hip) streams its weights through a 4-stage LDS ring, three slots ahead: five W1 k-tiles and three
column slices of the contraction k-tile per 64-hidden-unit chunk.  Its arithmetic is the two-launch path's (sdn_gemm_ln_* with
the GEGLU epilogue + the two-source K = 5C GEMM), so every comparison here is equality of bits: the 16-bit output and the fp32
GroupNorm column sums.  Shapes are the smallest at which the ring can go wrong: one 128-row workgroup already runs all 160 slots
(every stage index, every wrap, the drain before the trailing k-tiles); 384 rows add two more workgroups and column-sum row
groups; 200 rows leave a ragged second tile whose rows past M are zero-filled by the buffer range check."""
import functools

import pytest
import torch

from safe_denoiser_amd.unet import _interleave16
from tests_support import ops

pytestmark = pytest.mark.gpu
C = 320
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _sentinel_outputs():
    """Outputs start as a NaN pattern, so a tile that a kernel never writes cannot compare equal by allocator reuse."""
    ops.SENTINEL = True
    yield
    ops.SENTINEL = False


def _operands(dt, M, adversarial):
    g = torch.Generator().manual_seed(17 + M)
    x = torch.randn(M, C, generator=g) * 1.5 + torch.randn(M, 1, generator=g) * 2.0
    w1 = torch.randn(8 * C, C, generator=g) * C ** -0.5
    wcat = torch.randn(C, 5 * C, generator=g) * (5 * C) ** -0.5
    if adversarial:
        # every k-tile of X at a magnitude of its own (alternating sign, so LayerNorm keeps it), chunk j of W1 (value and gate
        # rows) and of Wcat (its 64 k columns) scaled by 2^(j mod 5): a k-tile or slice that lands in the wrong stage, or is
        # read one slot early, differs from the right one in its exponent, not in its last bits
        kt = torch.arange(C) // 64
        x = (torch.randn(M, C, generator=g) + (kt + 1) * 3.0 * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)) * 2.0 ** kt
        sc = 2.0 ** ((torch.arange(4 * C) // 64) % 5)
        w1 = w1 * torch.cat([sc, sc])[:, None]
        wcat[:, :4 * C] *= sc[None, :]
    b1 = torch.randn(8 * C, generator=g)
    gamma = 1 + 0.2 * torch.randn(C, generator=g); beta = 0.3 * torch.randn(C, generator=g)
    bcat = torch.randn(C, generator=g)
    res = torch.randn(M, C, generator=g)
    return dict(x=x.to(dt).cuda(), w1=_interleave16(w1.to(dt)).contiguous().cuda(), b1=_interleave16(b1).contiguous().cuda(),
                gamma=gamma.cuda(), beta=beta.cuda(), wcat=wcat.to(dt).cuda(), bcat=bcat.cuda(), res=res.to(dt).cuda())


@functools.lru_cache(maxsize=None)
def _case(dt, M, adversarial=False):
    """Operands + the two-launch results (pre-pass / fragment statistics), computed once and left unchanged."""
    o = _operands(dt, M, adversarial)
    want = {}
    for own in (False, True):
        cs = torch.zeros((M + 127) // 128, C, 2, device="cuda")
        ff = ops.gemm_ln(o["x"], o["w1"], o["gamma"], o["beta"], o["b1"], act=2, prepass=not own)
        out = ops.gemm(ff, o["wcat"], a2=o["x"], bias=o["bcat"], residual=o["res"], col_stats=cs)
        want[own] = (out, cs)
    torch.cuda.synchronize()
    return o, want


def _check(dt, M, own, with_cols, adversarial=False):
    o, want = _case(dt, M, adversarial)
    out_w, cs_w = want[own]
    cs = torch.zeros_like(cs_w) if with_cols else None
    got = ops.ffn_fused(o["x"], o["w1"], o["gamma"], o["beta"], o["b1"], o["wcat"], o["bcat"], o["res"], col_stats=cs, own_stats=own)
    torch.cuda.synchronize()
    assert got.shape == (M, C) and torch.isfinite(out_w.float()).all()
    assert torch.equal(got.view(torch.int16), out_w.view(torch.int16)), float((got.float() - out_w.float()).abs().max())
    if with_cols:
        assert torch.equal(cs, cs_w)


@pytest.mark.parametrize("with_cols", [True, False], ids=["cols", "nocols"])
@pytest.mark.parametrize("own", [False, True], ids=["prepass", "own"])
@pytest.mark.parametrize("M", [128, 384, 200])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_ring_fed_feed_forward_gives_the_two_launch_bits(dt, M, own, with_cols):
    """One workgroup / three workgroups / a ragged second tile.  sdn_ffn_geglu_fused takes any M >= 0 (the grid is ceil(M / 128)
    and rows past M are zero-filled), so M = 200 is compared like the others: its column sums equal the partner's only if the
    rows past M contribute nothing."""
    _check(dt, M, own, with_cols)


@pytest.mark.parametrize("own", [False, True], ids=["prepass", "own"])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_ring_stage_mix_up_would_change_high_bits(dt, own):
    """Operands whose k-tiles and chunks differ by powers of two (see _operands): plain Gaussian tiles are alike enough that a
    stale tile moves only low bits of a few outputs."""
    _check(dt, 128, own, True, adversarial=True)
