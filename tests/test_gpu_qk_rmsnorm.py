"""sdn_qk_rmsnorm (the SD-3.5 q/k RMS norm, in place on the q and k thirds of stacked [q | k | v] rows), element by element against
float64 on the values the kernel reads:

    y = x * (mean(x^2 over the 64 of a head) + eps)^-1/2 * w          |out - y| <= 1/2 ulp_T(y) + 39 * 2^-24 |y|

39, worst case: a 64-term positive f32 sum in any order is within 64 * 2^-24 relative, 32 * 2^-24 after the inverse square root; the
1/64 scaling (exact) and `+ eps` 1; rsqrtf 4 (exact.RSQRT_REL = 2^-22); the two multiplies 2.
The v third, the pad columns of a wider leading dimension, a NaN row behind the last one and the guard bands around the buffer must
come back bit for bit.  heads 24 gives 48 groups per row (six waves of eight heads in 16-bit storage, twelve of four in f32), heads 4
one wave (two in f32), heads 5 ten groups -- a last wave whose idle lanes would land in v; rows 1, 7, 90 and 2048 run from one partly
filled block to the grid cap's stride loop (2048 x 6 wave items = 3072 blocks of four waves > 2048)."""
import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from tests_support import exact

pytestmark = pytest.mark.gpu
F64 = torch.float64
CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
EPS = 1e-6
REL = 39 * 2.0 ** -24


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _gains():
    i = torch.arange(64, dtype=torch.float32, device="cuda")
    return 0.5 + i / 64, -(1.5 + i / 32)            # wq != wk, every element distinct: a swapped or mis-indexed gain fails


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("heads", [4, 24, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_qk_rmsnorm_against_float64(dtype, heads, pad):
    lib = sda.lib()
    C_ = heads * 64
    ld = 3 * C_ + pad
    wq, wk = _gains()
    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    for rows in (1, 7, 90, 2048):
        g = torch.Generator(device="cuda").manual_seed(1000 * heads + rows + pad)
        buf, view = exact.guarded(rows + 1, ld, dtype, "cuda")
        x = (torch.randn(rows, ld, generator=g, device="cuda") * 1.7 + 0.2)
        x[0, 64:128] = 0.0                                                       # an all-zero q head: exactly 0 out, no NaN
        x[0, 128:192] = 6e4 * (1 - 2 * (torch.arange(64, device="cuda") % 2))    # +-6e4: the squares must not overflow the f32 sum
        x[0, C_:C_ + 64] = 1e-3                                                  # a k head with one large element and 63 tiny ones
        x[0, C_ + 17] = 100.0
        view[:rows] = x.to(dtype)
        view[rows] = float("nan")                                                # one NaN row behind the last
        before = view.clone()
        rc = lib.sdn_qk_rmsnorm(CODE[dtype], view.data_ptr(), rows, heads, ld, wq.data_ptr(), wk.data_ptr(), EPS, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        xin = before[:rows, :2 * C_].to(F64).view(rows, 2 * heads, 64)
        w = torch.stack([wq] * heads + [wk] * heads).to(F64)                     # [2 heads, 64]
        y = xin * (xin.pow(2).mean(-1, keepdim=True) + eps32).pow(-0.5) * w
        out = view[:rows, :2 * C_].to(F64).view(rows, 2 * heads, 64)
        tol = 0.5 * exact.ulp(y, dtype) + REL * y.abs()
        err = (out - y).abs()
        worst = float((err / tol).max())
        print(f"qk_rmsnorm {dtype} heads {heads} ld {ld} rows {rows}: worst |out - y| / bound {worst:.3f}")
        assert not torch.isnan(out).any() and not torch.isinf(out).any()
        assert bool((err <= tol).all()), f"rows {rows}: {int((err > tol).sum())} elements outside the bound (worst {worst:.3f} x)"
        assert bool((out[0, 1] == 0).all())
        # v, the pad columns and the NaN row: bit for bit; guard bands intact
        assert torch.equal(_bits(view[:rows, 2 * C_:]), _bits(before[:rows, 2 * C_:]))
        assert torch.equal(_bits(view[rows]), _bits(before[rows]))
        assert exact.sentinels_intact(buf, view) == 0
