"""Host-side checks of the Inception-v3 pool3 tower and of the FID / KID bookkeeping (no GPU): the oracle's parameter count, the
manifest against the oracle's state dict, the BatchNorm fold of the packed weights, the plan's FLOPs against the oracle's shape
walk, argument validation of the new entry points, and frechet_distance / FrechetInceptionDistance / KernelInceptionDistance
against independent float64 restatements (scipy's sqrtm, numpy's mean / cov, the MMD formula written out)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from safe_denoiser_amd.inception import BN_EPS, InceptionV3
from safe_denoiser_amd.metrics import FrechetInceptionDistance, KernelInceptionDistance, frechet_distance, poly_mmd2
from tests_support import inception_oracle as oracle


@pytest.fixture(scope="module")
def tower():
    return InceptionV3()


# ---- architecture ------------------------------------------------------------------------------------------------------------------
def test_oracle_parameter_count():
    assert oracle.parameter_count() == 21_785_568 == oracle.TRUNK_PARAMETERS
    assert oracle.parameter_count() + oracle.AUX_AND_FC_PARAMETERS == 27_161_264          # torchvision's figure for inception_v3
    assert len(oracle.conv_table()) == 94


def test_manifest_equals_oracle_state_dict(tower):
    assert tower.state_dict_shapes() == oracle.state_dict_shapes()
    assert [c["name"] for c in tower.convs] == [c[0] for c in oracle.conv_table()]
    for c, (name, cin, cout, k, stride, pad, _) in zip(tower.convs, oracle.conv_table()):
        assert (c["cin"], c["cout"], (c["kh"], c["kw"]), c["stride"], (c["pad_h"], c["pad_w"])) == (cin, cout, k, stride, pad), name
        assert c["kpad"] == -(-cin * k[0] * k[1] // 64) * 64 and c["n_padded"] == -(-cout // 32) * 32, name


def test_plan_flops_equal_the_oracle_shape_walk(tower):
    assert _lib.lib().sdn_inception_conv_count(tower._h) == 94
    assert tower.flops(1)[0] == oracle.flops(299)
    assert tower.flops(5)[0] == oracle.flops(299, 5)
    small = InceptionV3(resize_input=False, image_size=139)
    assert small.flops(3)[0] == oracle.flops(139, 3)
    assert tower.flops(1)[1] == 0.0                                                         # no attention


def test_folded_weights_equal_a_float64_fold_rounded_once(tower):
    sd = tower.synthetic_state_dict(7)
    sd["fc.weight"] = torch.zeros(1008, 2048)                                               # ignored keys
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros(1)
    sd["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(0)
    buf = tower.pack_state_dict(sd)
    by_name = {p["name"]: p for p in tower.manifest}
    for c in tower.convs:
        n = c["name"]
        g, b, m, v = (sd[f"{n}.bn.{k}"].double().numpy() for k in ("weight", "bias", "running_mean", "running_var"))
        s = g / np.sqrt(v + BN_EPS)
        w = sd[n + ".conv.weight"].double().numpy() * s[:, None, None, None]
        want_w = np.zeros((c["n_padded"], c["kpad"]), dtype=np.float32)
        want_w[:c["cout"], :c["kh"] * c["kw"] * c["cin"]] = w.transpose(0, 2, 3, 1).reshape(c["cout"], -1).astype(np.float32)
        want_b = np.zeros(c["n_padded"], dtype=np.float32)
        want_b[:c["cout"]] = (b - m * s).astype(np.float32)
        pw, pb = by_name[n + ".conv.weight"], by_name[n + ".bn.bias"]
        got_w = buf[pw["offset"]:pw["offset"] + want_w.size * 4].view(torch.float32).numpy().reshape(want_w.shape)
        got_b = buf[pb["offset"]:pb["offset"] + want_b.size * 4].view(torch.float32).numpy()
        assert np.array_equal(got_w, want_w), n
        assert np.array_equal(got_b, want_b), n
    with pytest.raises(KeyError):
        tower.pack_state_dict({k: v for k, v in sd.items() if k != "Mixed_7c.branch_pool.bn.running_var"})
    bad = dict(sd)
    bad["Mixed_6b.branch7x7_2.conv.weight"] = bad["Mixed_6b.branch7x7_2.conv.weight"].transpose(2, 3)
    with pytest.raises(sda.SdnError):
        tower.pack_state_dict(bad)


# ---- argument validation -------------------------------------------------------------------------------------------------------------
def test_kernels_reject_bad_arguments_on_the_host():
    lib = sda.lib()
    A, B_ = 0x10000, 0x20000
    ok = dict(h=9, w=7, c=3, kh=3, kw=3, sh=2, sw=2, ph=0, pw=0, kpad=64)

    def patch(inp=A, out=B_, batch=2, **kw):
        a = dict(ok, **kw)
        return lib.sdn_patch_rows_f32(inp, batch, a["h"], a["w"], a["c"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["kpad"], out, None)

    assert patch(batch=0) == 0                                                              # nothing to do is not an error
    for bad in (dict(inp=None), dict(out=None), dict(batch=-1), dict(kpad=27), dict(kpad=32), dict(kpad=40), dict(kh=0),
                dict(sh=0), dict(ph=3), dict(ph=-1), dict(h=2), dict(c=0), dict(inp=A + 4), dict(out=B_ + 8), dict(kh=17)):
        assert patch(**bad) == -1, bad
    pool = lambda mode=0, inp=A, batch=1, h=9, w=7, c=64, stride=2, pad=0, out=B_, ldo=256, c0=64: \
        lib.sdn_pool3_f32(mode, inp, batch, h, w, c, stride, pad, out, ldo, c0, None)
    assert pool(batch=0) == 0
    for bad in (dict(mode=2), dict(inp=None), dict(out=None), dict(stride=3), dict(pad=2), dict(h=2), dict(ldo=127), dict(c0=-1),
                dict(c0=200), dict(c=0), dict(inp=A + 2)):
        assert pool(**bad) == -1, bad
    assert pool(h=1, w=1, pad=1, stride=1, batch=0) == 0                                    # a 1x1 map with pad 1 is a valid pool
    assert lib.sdn_resize_bilinear_f32(A, 0, 64, 64, 299, 299, 2.0, -1.0, B_, None) == 0
    assert lib.sdn_resize_bilinear_f32(None, 1, 64, 64, 299, 299, 2.0, -1.0, B_, None) == -1
    assert lib.sdn_resize_bilinear_f32(A, 1, 0, 64, 299, 299, 2.0, -1.0, B_, None) == -1
    assert lib.sdn_resize_bilinear_f32(A, 1, 64, 64, 299, 9000, 2.0, -1.0, B_, None) == -1
    assert lib.sdn_resize_bilinear_f32(A, 1, 64, 64, 299, 299, 2.0, -1.0, B_ + 1, None) == -1
    assert lib.sdn_spatial_mean_f32(A, 0, 9, 2048, B_, None) == 0
    assert lib.sdn_spatial_mean_f32(A, 1, 0, 2048, B_, None) == -1
    assert lib.sdn_spatial_mean_f32(A, 1, 9, 0, B_, None) == -1
    assert lib.sdn_spatial_mean_f32(None, 1, 9, 2048, B_, None) == -1


def test_the_16_bit_gemms_refuse_the_relu_code():
    """SDN_ACT_RELU (9) belongs to sdn_gemm_f32 / sdn_gemm_x3; that those accept it, and still refuse 6 and 8, is checked where they run
    (tests/test_gpu_inception.py): their validation of `act` sits behind the M == 0 early return."""
    lib = sda.lib()
    A, B_, Cc = 0x10000, 0x20000, 0x30000
    d16 = _lib.GemmDesc(M=128, N=256, K=128, act=9)
    assert lib.sdn_gemm_bf16(C.byref(d16), A, None, B_, None, None, None, None, Cc, None) == -1
    assert lib.sdn_gemm_f16(C.byref(d16), A, None, B_, None, None, None, None, Cc, None) == -1


def test_create_and_forward_reject_bad_arguments(tower):
    lib = sda.lib()
    h = C.c_void_p()
    for bad in (dict(image_size=74), dict(image_size=1025), dict(normalize_input=2), dict(dtype=0), dict(dtype=1), dict(dtype=3)):
        cfg = _lib.InceptionConfig(**dict(dict(image_size=299, normalize_input=1, dtype=2), **bad))
        assert lib.sdn_inception_create(C.byref(cfg), C.byref(h)) == -1, bad
    assert lib.sdn_inception_create(None, C.byref(h)) == -1
    W, X, O, WS = 0x10000, 0x20000, 0x30000, 0x40000
    fwd = lambda hd=tower._h, w=W, x=X, o=O, b=1, ih=256, iw=256, rs=1, ws=WS, n=1 << 40: \
        lib.sdn_inception_forward(hd, w, x, o, b, ih, iw, rs, ws, n, None)
    assert fwd(n=0) == -3                                                                   # reaches the plan runner: workspace too small
    for bad in (dict(hd=None), dict(w=None), dict(x=None), dict(o=None), dict(ws=None), dict(b=0), dict(b=-1), dict(ih=0), dict(iw=9000),
                dict(rs=2), dict(rs=0), dict(x=X + 2), dict(o=O + 1), dict(b=100)):
        assert fwd(**bad) == -1, bad
    assert fwd(rs=0, ih=299, iw=299, n=0) == -3                                             # resize = 0 takes the trunk's own size
    assert lib.sdn_unet_workspace_bytes(tower._h, 32) > 0 and lib.sdn_unet_workspace_bytes(tower._h, 100) == 0
    info = _lib.InceptionConv()
    assert lib.sdn_inception_conv_info(tower._h, 94, C.byref(info)) == -1 and lib.sdn_inception_conv_info(tower._h, 0, None) == -1


def test_foreign_handles_are_refused(tower):
    lib = sda.lib()
    cfg = _lib.ClipConfig(vocab_size=128, hidden_size=128, intermediate_size=128, num_layers=2, num_heads=2, max_position_embeddings=77, dtype=0)
    clip = C.c_void_p()
    assert lib.sdn_clip_create(C.byref(cfg), C.byref(clip)) == 0
    try:
        W, X, O, WS = 0x10000, 0x20000, 0x30000, 0x40000
        assert lib.sdn_inception_forward(clip, W, X, O, 1, 256, 256, 1, WS, 0, None) == -1
        assert lib.sdn_inception_conv_count(clip) == 0
        assert lib.sdn_clip_forward(tower._h, W, X, None, O, 1, WS, 0, None) == -1
        assert lib.sdn_unet_forward(tower._h, W, X, 1.0, X, O, 1, WS, 0, None) == -1
        assert lib.sdn_clip_vision_forward(tower._h, W, X, None, O, 1, WS, 0, None) == -1
    finally:
        lib.sdn_unet_destroy(clip)


# ---- Frechet distance ------------------------------------------------------------------------------------------------------------------
def _features(n, d, seed, shift=0.0):
    g = np.random.default_rng(seed)
    mix = g.standard_normal((d, d)) / np.sqrt(d)
    return np.abs(g.standard_normal((n, d)) @ mix + shift)                                   # non-negative like pooled ReLU features


def _fid_sqrtm(mu1, s1, mu2, s2):
    """calculate_frechet_distance's formula with scipy's Schur square root of the non-symmetric product."""
    covmean = scipy.linalg.sqrtm(s1 @ s2)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean.real))


@pytest.mark.parametrize("n, d, bound", [(512, 64, 1e-9), (2048, 256, 1e-9), (16, 64, 1e-6)])
def test_frechet_distance_against_scipy_sqrtm(n, d, bound):
    a, b = _features(n, d, 1), _features(n, d, 2, shift=0.3)
    st = lambda x: (x.mean(0), np.cov(x, rowvar=False))
    (mu1, s1), (mu2, s2) = st(a), st(b)
    got, want = frechet_distance(mu1, s1, mu2, s2), _fid_sqrtm(mu1, s1, mu2, s2)
    rel = abs(got - want) / abs(want)
    print(f"n {n} d {d}: eigh {got!r} sqrtm {want!r} rel {rel:.3g}")
    assert rel <= bound
    assert frechet_distance(torch.from_numpy(mu1), torch.from_numpy(s1), mu2, s2) == got     # tensors are welcome


def test_fid_of_a_set_against_itself_is_zero():
    a = _features(512, 64, 3)
    mu, s = a.mean(0), np.cov(a, rowvar=False)
    v = frechet_distance(mu, s, mu, s)
    print(f"FID(A, A) / tr = {v / np.trace(s):.3g}")
    assert abs(v) <= 1e-6 * np.trace(s)
    with pytest.raises(sda.SdnError):
        frechet_distance(mu, s, mu[:-1], s)


def test_fid_statistics_split_merge_and_numpy_semantics():
    a, b = torch.from_numpy(_features(300, 48, 4)).float(), torch.from_numpy(_features(257, 48, 5, shift=0.2)).float()
    whole = FrechetInceptionDistance()
    whole.update_features(a, real=True)
    whole.update_features(b)
    # np.mean / np.cov(rowvar=False) of the float64 rows
    mu, cov = whole._sets[False].mean_cov()
    assert np.allclose(mu, b.double().numpy().mean(0), rtol=1e-13, atol=0)
    assert np.allclose(cov, np.cov(b.double().numpy(), rowvar=False), rtol=1e-10, atol=1e-13)
    r0, r1 = FrechetInceptionDistance(), FrechetInceptionDistance()
    r0.update_features(a[:100], real=True); r0.update_features(b[:31]); r0.update_features(b[31:120])
    r1.update_features(a[100:], real=True); r1.update_features(b[120:])
    r0.merge(r1)
    for real in (True, False):
        s, w = r0.statistics(real), whole.statistics(real)
        assert s["n"] == w["n"] and type(s["n"]) is int
        assert np.allclose(s["sum"], w["sum"], rtol=1e-14, atol=0)
        assert np.allclose(s["outer"], w["outer"], rtol=1e-14, atol=1e-14)
    assert abs(r0.compute() - whole.compute()) <= 1e-12 * abs(whole.compute())
    assert whole.state() == (0.0, 257)
    # a statistics dict merges like an instance; a loaded reference replaces the real set
    r2 = FrechetInceptionDistance()
    r2.merge(whole.statistics(False), real=False)
    r2.load_reference(*whole._sets[True].mean_cov())
    assert abs(r2.compute() - whole.compute()) <= 1e-12 * abs(whole.compute())
    whole.reset()
    assert whole.state() == (0.0, 0) and whole.statistics(True)["n"] == 300
    with pytest.raises(sda.SdnError):
        whole.compute()
    with pytest.raises(sda.SdnError):
        whole.update([object()])                                                             # no tower


# ---- KID -----------------------------------------------------------------------------------------------------------------------------
def _mmd2_direct(x, y, degree, gamma, coef):
    """The unbiased estimator written out pair by pair, float64."""
    m = len(x)
    k = lambda p, q: (gamma * float(np.dot(p, q)) + coef) ** degree
    xx = sum(k(x[i], x[j]) for i in range(m) for j in range(m) if i != j)
    yy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j)
    xy = sum(k(x[i], y[j]) for i in range(m) for j in range(m))
    return (xx + yy) / (m * (m - 1)) - 2 * xy / (m * m)


def test_kid_against_the_mmd_formula_on_fixed_subsets():
    real, fake = torch.from_numpy(_features(40, 32, 6)).float(), torch.from_numpy(_features(35, 32, 7, shift=0.25)).float()
    kid = KernelInceptionDistance(subsets=5, subset_size=12, generator=torch.Generator().manual_seed(11))
    kid.update_features(real[:25], real=True); kid.update_features(real[25:], real=True)
    kid.update_features(fake)
    mean, std = kid.compute()
    g = torch.Generator().manual_seed(11)                                                    # the same draws, restated
    vals = []
    for _ in range(5):
        i = torch.randperm(40, generator=g)[:12]
        j = torch.randperm(35, generator=g)[:12]
        vals.append(_mmd2_direct(real[i].double().numpy(), fake[j].double().numpy(), 3, 1.0 / 32, 1.0))
    assert abs(mean - np.mean(vals)) <= 1e-12 * abs(np.mean(vals))
    assert abs(std - np.std(vals)) <= 1e-9 * np.std(vals)
    again = KernelInceptionDistance(subsets=5, subset_size=12, generator=torch.Generator().manual_seed(11))
    again.update_features(real, real=True); again.update_features(fake)
    assert again.compute() == (mean, std)                                                    # reproducible with generator=
    assert kid.state() == (0.0, 35)
    v = poly_mmd2(real[:12], fake[:12], degree=2, gamma=0.5, coef=0.0)
    assert abs(float(v) - _mmd2_direct(real[:12].double().numpy(), fake[:12].double().numpy(), 2, 0.5, 0.0)) <= 1e-12 * abs(float(v))
    small = KernelInceptionDistance(subsets=2, subset_size=50)
    small.update_features(real, real=True); small.update_features(fake)
    with pytest.raises(sda.SdnError):
        small.compute()                                                                      # subset_size exceeds a set
    with pytest.raises(sda.SdnError):
        KernelInceptionDistance(subset_size=1)
