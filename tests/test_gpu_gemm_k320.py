"""k_gemm_k320 (csrc/sdn_gemm_k320.hip: the K = 320 linears with register-resident weights and streamed row panels) against the
generic sdn_gemm_* / sdn_gemm_ln_* entries on the same operands: the two must return the same BITS for every form the new entry
takes.  Equality with a partner could hide a shared mistake, so one case per dtype is also held to the float64 criterion of
tests_support/exact.py.

Outputs are views into NaN-sentinel buffers (before, after, ldc gap); A rows and residual rows past M are NaN in the same
allocation: a stray store or a stray read cannot pass.  The launch record (sdn_debug_k320_last_launch) shows that the new kernel
ran, on how many workgroups and row streams."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from tests_support import exact as X
from tests_support import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
VARIANTS = ["plain", "bias", "res", "ln", "ln_bias"]
CAPPED_M = [1, 63, 64, 65, 529]              # 529 rows = 9 panels of 64 (17 of 32 with a residual): the 3-slot ring wraps, last panel ragged


def _k320_record():
    rec = (C.c_int * 8)()
    sda.lib().sdn_debug_k320_last_launch(rec, 8)
    return list(rec)


def _gemm_record():
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    return list(rec)


@pytest.fixture
def capped():
    sda.lib().sdn_debug_set_k320_max_wgs(2)
    yield
    sda.lib().sdn_debug_set_k320_max_wgs(0)


def _operands(variant, dt, M, N, seed):
    g = torch.Generator().manual_seed(seed + (1 if dt == torch.float16 else 0))
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dt).cuda()
    a = X.with_nan_tail(rnd(M, 320), 64)
    w = rnd(N, 320, scale=320 ** -0.5)
    bias = torch.randn(N, generator=g).cuda() if variant in ("bias", "res", "ln_bias") else None
    res = X.nan_strided(rnd(M, N), N + 8) if variant == "res" else None          # (the residual shares the output's ldc)
    gamma = beta = None
    if variant.startswith("ln"):
        gamma = (1.0 + 0.2 * torch.randn(320, generator=g)).cuda()
        beta = (0.2 * torch.randn(320, generator=g)).cuda()
    return a, w, bias, res, gamma, beta


def _partner(variant, a, w, bias, res, gamma, beta, out):
    """The generic entry on the same operands -> the folded operands of the LayerNorm forms (None otherwise)."""
    if variant.startswith("ln"):
        fold = {}
        ops.gemm_ln(a, w, gamma, beta, bias=bias, out=out, fold=fold)
        return fold
    ops.gemm(a, w, bias=bias, residual=res, res_pre=1 if res is not None else 0, out=out)
    return None


def _k320(a, w, bias, res, fold, out, eps=1e-5):
    M, N = a.shape[0], w.shape[0]
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.ldc = M, N, 320, out.stride(0)
    d.res_pre = 1 if res is not None else 0
    p = lambda t: None if t is None else t.data_ptr()
    code = 1 if a.dtype == torch.float16 else 0
    if fold:
        return sda.lib().sdn_gemm_k320(code, C.byref(d), p(a), p(fold["w_folded"]), None, p(fold["c"]), p(fold["d"]), eps, None, p(out),
                                       _lib.stream_ptr())
    return sda.lib().sdn_gemm_k320(code, C.byref(d), p(a), p(w), p(bias), None, None, 0.0, p(res), p(out), _lib.stream_ptr())


def _compare(variant, dt, M, N, seed):
    a, w, bias, res, gamma, beta = _operands(variant, dt, M, N, seed)
    buf0, ref = X.guarded(M, N, dt, "cuda", ldc=N + 8)
    fold = _partner(variant, a, w, bias, res, gamma, beta, ref)
    before = _gemm_record()
    sda.lib().sdn_debug_k320_reset_launch()
    buf1, out = X.guarded(M, N, dt, "cuda", ldc=N + 8)
    assert _k320(a, w, bias, res, fold, out) == 0
    torch.cuda.synchronize()
    rec = _k320_record()
    assert rec[0] == 6 and rec[1] == (1 if dt == torch.float16 else 0), f"k_gemm_k320 did not run: record {rec}"
    assert rec[2] == (1 if fold else 0) and rec[3] == (1 if res is not None else 0) and rec[5] == N // 320, rec
    assert _gemm_record() == before, "sdn_gemm_k320 must keep its own launch record"
    assert X.sentinels_intact(buf1, out) == 0 and X.sentinels_intact(buf0, ref) == 0
    assert not torch.isnan(out.float()).any(), f"{variant} M={M} N={N}: unwritten or poisoned outputs"
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (
        f"{variant} [{dt}] M={M} N={N}: {int((out.view(torch.int16) != ref.view(torch.int16)).sum())} elements differ from the generic entry")
    return a, w, bias, res, out, buf1, rec


@pytest.mark.parametrize("N", [320, 960])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_equals_generic_entry_on_a_capped_grid(variant, dt, N, capped):
    for M in CAPPED_M:
        rec = _compare(variant, dt, M, N, seed=M)[-1]
        assert rec[6] == (2 if N == 320 else 1), f"capped launch should run {2 if N == 320 else 1} row stream(s): {rec}"


@pytest.mark.parametrize("variant,dt,N", [("bias", torch.bfloat16, 960), ("res", torch.float16, 320), ("ln", torch.bfloat16, 320),
                                          ("plain", torch.float16, 960), ("res", torch.bfloat16, 320), ("ln_bias", torch.float16, 960)])
def test_equals_generic_entry_on_the_full_grid(variant, dt, N):
    """One workgroup per CU: every row stream gets at least one panel, some two, the last panel is ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 64 * (cus + 1) + 7
    rec = _compare(variant, dt, M, N, seed=11)[-1]
    assert rec[4] == max(cus, N // 320) and rec[6] >= (cus // 8 // (N // 320)) * 8, rec


@pytest.mark.parametrize("dt", DTYPES)
def test_float64_criterion(dt, capped):
    """Bias + pre-added residual over a wrapping ring, element by element against float64 arithmetic on the same operands."""
    M, N = 529, 320
    a, w, bias, res, out, buf, _ = _compare("res", dt, M, N, seed=5)
    y, s, e, y32 = X.reference(a, w, bias=bias, residual=res)
    st = X.analyse(out, y, s, e, dtype=dt)
    fails = X.failures(st, exact_fn=True, ref_rate=X.ref_rate(y32, y, dt))
    print(f"k320 res [{dt}]: exact-rounding rate {st['rate']:.4f}, max ulp {st['max_ulp']:.3f}, worst err / bound {st['max_err_over_tol']:.3f}")
    assert not fails, "; ".join(fails)


def test_refused_forms():
    lib = sda.lib()
    a = torch.zeros(64, 384, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(640, 384, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(64, 640, dtype=torch.float32, device="cuda")
    vec = torch.zeros(640, device="cuda")

    def call(N=320, K=320, act=0, out_kind=0, n_valid=0, ldc=0, ln=(None, None), bias=None, res=None, dtype=0):
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.act, d.out_kind, d.n_valid, d.ldc = 64, N, K, act, out_kind, n_valid, ldc
        return lib.sdn_gemm_k320(dtype, C.byref(d), a.data_ptr(), w.data_ptr(), bias, ln[0], ln[1], 1e-5, res, out.data_ptr(), None)

    assert call(K=384) == -1 and call(K=256) == -1                       # K != 320
    assert call(N=352) == -1 and call(N=160) == -1                       # N % 320 != 0
    assert call(act=1) == -1 and call(act=2, N=640) == -1                # an activation
    assert call(out_kind=1) == -1 and call(out_kind=2) == -1             # f32 outputs
    assert call(n_valid=300) == -1                                       # ragged width
    assert call(ldc=324) == -1 and call(N=640, ldc=320) == -1            # ldc not a multiple of 8 / below N
    assert call(ln=(vec.data_ptr(), None)) == -1                         # half a LayerNorm fold
    assert call(ln=(vec.data_ptr(), vec.data_ptr()), bias=vec.data_ptr()) == -1
    assert call(ln=(vec.data_ptr(), vec.data_ptr()), res=a.data_ptr()) == -1
    assert call(dtype=2) == -1
    assert call() == 0                                                   # (the same call in an accepted form)
    torch.cuda.synchronize()


# ---- plan level ------------------------------------------------------------------------------------------------------------------
SMALL = dict(block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
             layers_per_block=1, attention_head_dim=8, cross_attention_dim=768, sample_size=16)


@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("dt", DTYPES)
def test_plan_switch_gives_the_same_bits(dt, rep):
    """sdn_debug_set_gemm_k320: the five K = 320 linears of the C = 320 block on k_gemm_k320 (default) or on k_gemm_dma."""
    from safe_denoiser_amd.unet import UNet2DConditionModel
    u = UNet2DConditionModel(text_len=77, dtype=dt, latent_repeat=rep, **SMALL)
    u.load_state_dict(u.synthetic_state_dict(7))
    g = torch.Generator().manual_seed(3)
    B = 6
    x = torch.randn(B // rep, 4, 16, 16, generator=g).cuda()
    e = torch.randn(B, 77, 768, generator=g).cuda()
    outs, kernels = [], []
    for on in (1, 0, 1):
        sda.lib().sdn_debug_set_gemm_k320(u._h, on)
        u._ws = {}
        u.profile_next()
        outs.append(u(x, 781.0, encoder_hidden_states=e).sample.clone())
        torch.cuda.synchronize()
        kernels.append({r["kernel"] for r in u.profile_read()})
    new = {"k_gemm_k320", "k_gemm_k320/rp", "k_gemm_k320/ln1"}
    assert kernels[0] & new and not (kernels[1] & new), (kernels[0], kernels[1])     # the switch really selects the plan form
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
