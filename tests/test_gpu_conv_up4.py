"""Upsampler convs in phase form (sdn_gemm_desc.upsample = 2 over the weights of sdn_conv_up4_weights), both 16-bit dtypes.

Derivation   the entry point's output equals, bit for bit, the same fp32 sums (ty-major, tx-minor) formed with torch and rounded once.
Operator     element by element against float64 arithmetic on the SAME stored operands -- the input map and the derived phase
             weights -- by the criterion of tests_support/exact.py; outputs are views into NaN-sentinel buffers, the map carries NaN
             rows behind its last sample, and the launch record must name the k_gemm_up4 instantiation the case is written for.
Agreement    with the nine-tap op on one case: both against float64 conv2d(interpolate(x, 2)) on the stored nine-tap weights.  The
             phase weights carry one more rounding to the storage type than the nine-tap ones, an error of the size of the output's
             own rounding and independent of it, so the phase op's rel L2 is expected at sqrt(2) x the nine-tap op's; the bound is
             2 x (sqrt(2) plus sampling margin), on values measured in the same test.
"""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from tests_support import exact as X
from tests_support import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
F64 = torch.float64
UP4_FAMILY = 5                 # sdn_gemm_common.h: launch-record family of k_gemm_up4

# rows ty (tx) of the nine-tap kernel that read stored row y + a - 1 + py (column x + b - 1 + px): TAPS[parity][a or b]
TAPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}


def _t(g, *shape, scale=1.0, dt=torch.bfloat16):
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def _last_launch():
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    return list(rec)


def derive(w9, N, Cin):
    """sdn_conv_up4_weights: [N, 9 Cin] -> [4, N, 4 Cin]."""
    out = torch.empty(4, N, 4 * Cin, dtype=w9.dtype, device=w9.device)
    _lib.check(sda.lib().sdn_conv_up4_weights(1 if w9.dtype == torch.float16 else 0, w9.data_ptr(), N, Cin, out.data_ptr(),
                                              _lib.stream_ptr()), "sdn_conv_up4_weights")
    return out


def derive_torch(w9, N, Cin):
    """The same sums in fp32 with torch, in the same order, rounded once to the storage type."""
    w = w9.float().view(N, 3, 3, Cin)
    out = torch.empty(4, N, 2, 2, Cin, dtype=torch.float32, device=w9.device)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    acc = None
                    for ty in TAPS[py][a]:
                        for tx in TAPS[px][b]:
                            acc = w[:, ty, tx] if acc is None else acc + w[:, ty, tx]
                    out[2 * py + px, :, a, b] = acc
    return out.to(w9.dtype).view(4, N, 4 * Cin)


def conv_up4(x, w4, bias, out, col_stats=None):
    """x [B, Hs, Ws, Cin], w4 [4, N, 4 Cin] -> out [B * 4 Hs Ws, N] (a caller-owned view: its row stride becomes ldc)."""
    B, Hs, Ws, Cin = x.shape
    N = w4.shape[1]
    d = _lib.GemmDesc()
    d.a_mode, d.Hs, d.Ws, d.Cin, d.Ho, d.Wo, d.stride, d.upsample = 1, Hs, Ws, Cin, 2 * Hs, 2 * Ws, 1, 2
    d.M, d.N, d.K, d.rows_per_batch, d.ldc = B * 4 * Hs * Ws, N, 4 * Cin, 4 * Hs * Ws, out.stride(0)
    p = lambda t: None if t is None else t.data_ptr()
    sfx = "f16" if x.dtype == torch.float16 else "bf16"
    if col_stats is not None:
        rc = getattr(sda.lib(), f"sdn_gemm_stats_{sfx}")(C.byref(d), p(x), None, p(w4), p(bias), None, None, p(out), p(col_stats),
                                                        _lib.stream_ptr())
    else:
        rc = getattr(sda.lib(), f"sdn_gemm_{sfx}")(C.byref(d), p(x), None, p(w4), p(bias), None, None, None, p(out), _lib.stream_ptr())
    return rc, d


def phase_reference(x, w4, bias):
    """(y, S', E_epi, y32), rows in OUTPUT order [B * 2Hs * 2Ws, N]: per phase a 2x2 conv over the zero-padded stored map."""
    B, Hs, Ws, Cin = x.shape
    N = w4.shape[1]
    xp = F.pad(x.to(F64), (0, 0, 1, 1, 1, 1))                         # [B, Hs + 2, Ws + 2, Cin]
    res = [torch.empty(B, Hs, 2, Ws, 2, N, dtype=F64, device=x.device) for _ in range(3)]
    y32 = torch.empty(B, Hs, 2, Ws, 2, N, dtype=torch.float32, device=x.device)
    for py in (0, 1):
        for px in (0, 1):
            A = torch.cat([xp[:, py + a:py + a + Hs, px + b:px + b + Ws] for a in (0, 1) for b in (0, 1)], dim=3).reshape(-1, 4 * Cin)
            y, s, e, y3 = X.reference_aw(A, w4[2 * py + px].to(F64), x.dtype, bias=bias)
            for dst, src in zip(res, (y, s, e)):
                dst[:, :, py, :, px] = src.view(B, Hs, Ws, N)
            y32[:, :, py, :, px] = y3.view(B, Hs, Ws, N)
    return [t.view(-1, N) for t in res] + [y32.view(-1, N)]


def _gemm_order(out, B, Hs, Ws):
    """Output rows [B * 2Hs * 2Ws, N] -> the GEMM's row order (sample, phase, low-res pixel)."""
    N = out.shape[1]
    return out.reshape(B, Hs, 2, Ws, 2, N).permute(0, 2, 4, 1, 3, 5).reshape(-1, N)


def _make(dt, seed, B, H, Cin, N):
    g = torch.Generator().manual_seed(seed + (1 if dt == torch.float16 else 0))
    x = X.with_nan_tail(_t(g, B * H * H, Cin, dt=dt), 64).view(B, H, H, Cin)           # NaN behind the last sample's map
    w9 = _t(g, N, 9 * Cin, scale=(9 * Cin) ** -0.5, dt=dt)
    bias = torch.randn(N, generator=g).cuda()
    return x, w9, bias


# name: (NREP of the pinned 256-row tile, shape, col_stats)
CASES = {
    "16^2, B 2, Cin 128, N 320":          (10, dict(B=2, H=16, Cin=128, N=320), False),
    "16^2, B 2, Cin 128, N 256":          (8, dict(B=2, H=16, Cin=128, N=256), False),
    "32^2, B 3, Cin 64, N 320, col_stats": (10, dict(B=3, H=32, Cin=64, N=320), True),
    "16^2, B 1, Cin 64, N 640":           (10, dict(B=1, H=16, Cin=64, N=640), False),
}


def _op_case(name, dt, nrep, shape, col_stats):
    B, H, Cin, N = shape["B"], shape["H"], shape["Cin"], shape["N"]
    x, w9, bias = _make(dt, 11, B, H, Cin, N)
    w4 = derive(w9, N, Cin)
    M = B * 4 * H * H
    buf, out = X.guarded(M, N, dt, "cuda", ldc=N + 8)
    cbuf = cs = None
    if col_stats:
        cbuf, cs = X.guarded_like((M // 128, N, 2), torch.float32, "cuda")
    rc, _ = conv_up4(x, w4, bias, out, cs)
    assert rc == 0, f"{name}: status {rc}"
    rec = _last_launch()
    assert rec[:6] == [UP4_FAMILY, 1 if dt == torch.float16 else 0, nrep, 4, 2, 0] and rec[6:9] == [M // 256, N // (32 * nrep), 1], \
        f"{name}: launch record {rec}"
    torch.cuda.synchronize()
    y, s, e, y32 = phase_reference(x, w4, bias)
    st = X.analyse(out, y, s, e, dtype=dt)
    rr = X.ref_rate(y32, y, dt)
    print(f"{name} [{dt}]: n {st['n']} exact-rounding rate {st['rate']:.4f} (torch fp32 {rr:.4f}) max ulp {st['max_ulp']:.3f} "
          f"max err / bound {st['max_err_over_tol']:.3f} direction {st['direction']:+.4f} over {st['n_dir']}")
    fails = X.failures(st, exact_fn=True, ref_rate=rr, direction=True)
    bad = X.sentinels_intact(buf, out)
    if bad:
        fails.append(f"{bad} guard-band sentinels overwritten")
    assert not fails, f"{name} [{dt}]: " + "; ".join(fails)
    if col_stats:
        # [M / 128][N][2] = fp32 (sum, sum of squares) of the STORED values of each 128-row block, blocks in the GEMM's row order
        v = _gemm_order(out, B, H, H).to(F64).view(-1, 128, N)
        for i, ref, mag in ((0, v.sum(1), v.abs().sum(1)), (1, (v * v).sum(1), (v * v).sum(1))):
            err = (cs[..., i].to(F64) - ref).abs()
            assert bool((err <= 2.0 ** -17 * mag + 1e-30).all()), (name, "col_stats", i, float((err / mag.clamp_min(1e-30)).max()))
        assert X.sentinels_intact(cbuf, cs) == 0, (name, "col_stats guard band")


@pytest.fixture(autouse=True)
def _no_tf32():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("Cin", [64, 128])
def test_phase_weights_are_the_fp32_tap_sums_rounded_once(dt, Cin):
    g = torch.Generator().manual_seed(3 + Cin)
    N = 64
    w9 = _t(g, N, 9 * Cin, scale=(9 * Cin) ** -0.5, dt=dt)
    got, want = derive(w9, N, Cin), derive_torch(w9, N, Cin)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the float64 identity the form rests on, on a small map: conv3x3(nearest-2x(x)) == the four 2x2 phase convs (unrounded sums)
    x = torch.randn(2, 6, 4, 7, generator=g, dtype=F64)
    w = w9[:5, :].to(F64).cpu().view(5, 3, 3, Cin)[..., :6].permute(0, 3, 1, 2).contiguous()
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros_like(ref)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    wk = sum(w[:, :, ty, tx] for ty in TAPS[py][a] for tx in TAPS[px][b])
                    out[:, :, py::2, px::2] += torch.einsum("bchw,nc->bnhw", xp[:, :, py + a:py + a + 4, px + b:px + b + 7], wk)
    assert float((out - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_phase_op_is_exact_on_its_stored_operands(dt, name):
    nrep, shape, col_stats = CASES[name]
    _op_case(name, dt, nrep, shape, col_stats)


def test_forms_outside_the_phase_mode_are_refused():
    dt = torch.bfloat16
    x, w9, bias = _make(dt, 5, 1, 16, 64, 320)
    w4 = derive(w9, 320, 64)
    out = torch.empty(4 * 256, 320, dtype=dt, device="cuda")
    lib = sda.lib()
    p = lambda t: t.data_ptr()
    rc, d = conv_up4(x, w4, bias, out)
    assert rc == 0
    res, rowv = torch.zeros_like(out), torch.zeros(1, 320, device="cuda")
    part = torch.empty(2 * out.numel(), dtype=torch.float32, device="cuda")
    call = lambda **kw: lib.sdn_gemm_bf16(C.byref(d), p(x), None, p(w4), p(bias), kw.get("rowbias"), kw.get("rowgate"), kw.get("residual"),
                                          p(out), _lib.stream_ptr())
    assert call(residual=p(res)) != 0 and call(rowbias=p(rowv)) != 0 and call(rowgate=p(rowv)) != 0
    for field, value in (("act", 1), ("n_valid", 300), ("out_kind", 1), ("out_kind", 2), ("x3_out", 1), ("stride", 2), ("K", 9 * 64)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert call() != 0, field
        setattr(d, field, keep)
    d.split_k = 2
    assert lib.sdn_gemm_splitk_bf16(C.byref(d), p(x), None, p(w4), p(bias), None, None, None, p(out), p(part), part.numel() * 4,
                                    _lib.stream_ptr()) != 0
    d.split_k = 0
    # shapes that do not qualify: a stored map that is not whole 256-row tiles, an N no 256-row tile serves
    x8 = torch.zeros(1, 8, 8, 64, dtype=dt, device="cuda")
    d.Hs = d.Ws = 8; d.Ho = d.Wo = 16; d.M = 256
    assert lib.sdn_gemm_bf16(C.byref(d), p(x8), None, p(w4), p(bias), None, None, None, p(out), _lib.stream_ptr()) != 0
    d.Hs = d.Ws = 16; d.Ho = d.Wo = 32; d.M = 4 * 256
    assert call() == 0
    d.N = 192
    assert call() != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_phase_op_agrees_with_the_nine_tap_op(dt):
    """Case 1: rel L2 of both ops against float64 conv2d(interpolate(x, 2)) on the stored nine-tap weights; phase <= 2 x nine-tap.
    (Measured on MI355X, profiles/up4_op_error.json.)"""
    B, H, Cin, N = 2, 16, 128, 320
    x, w9, bias = _make(dt, 11, B, H, Cin, N)
    w4 = derive(w9, N, Cin)
    M = B * 4 * H * H
    buf, out4 = X.guarded(M, N, dt, "cuda", ldc=N + 8)
    rc, _ = conv_up4(x, w4, bias, out4)
    assert rc == 0 and _last_launch()[0] == UP4_FAMILY
    out9 = ops.gemm(x, w9, bias=bias, conv=dict(Hs=H, Ws=H, Cin=Cin, Ho=2 * H, Wo=2 * H, stride=1, upsample=1))
    assert _last_launch()[0] != UP4_FAMILY
    torch.cuda.synchronize()
    wk = w9.to(F64).view(N, 3, 3, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(F.interpolate(x.to(F64).permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), wk, bias.to(F64), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(M, N)
    rel = lambda o: float((o.to(F64) - ref).norm() / ref.norm())
    r9, r4 = rel(out9), rel(out4)
    print(f"up4 op error [{dt}]: nine-tap rel L2 {r9:.4e}, phase form {r4:.4e}, ratio {r4 / r9:.3f}")
    if os.environ.get("SDN_UP4_STATS"):
        path = os.environ["SDN_UP4_STATS"]
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[str(dt).split(".")[-1]] = dict(shape=dict(B=B, Hs=H, Cin=Cin, N=N), nine_tap_rel_l2=r9, phase_rel_l2=r4, ratio=r4 / r9)
        json.dump(rec, open(path, "w"), indent=1)
    assert X.sentinels_intact(buf, out4) == 0
    assert r4 <= 2.0 * r9, (r4, r9)
