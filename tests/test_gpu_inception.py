"""The Inception-v3 pool3 tower on the GPU: its four data-movement kernels against torch restatements (bit equality where the
operator is exact, tests_support/exact.py's per-element criterion where it is not), one convolution per kernel geometry of the
trunk as "patch rows, then sdn_gemm_f32 with bias + ReLU into a channel slice" against float64 F.conv2d, the whole trunk against
the float64 oracle, the full path's bit-level invariances (resize in or before the plan, batch position, chunk boundary), and
evaluate_fid on two directories of PNGs.  Synthetic weights from a seed; measured distances go to profiles/inception_parity.json."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from safe_denoiser_amd import metrics as M
from safe_denoiser_amd.inception import InceptionV3, resize_bilinear
from tests_support import exact as X
from tests_support import inception_oracle as oracle
from tests_support import ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "inception_parity.json")
F32, F64 = torch.float32, torch.float64


def record(key, value):
    data = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            data = json.load(f)
    data[key] = value
    with open(PARITY, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def bits(t):
    return t.contiguous().view(torch.int32)


def up(v, m):
    return -(-v // m) * m


def out_side(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ---- callers ---------------------------------------------------------------------------------------------------------------------
def patch_rows(x, k, stride, pad, out, kpad):
    b, h, w, c = x.shape
    _lib.check(sda.lib().sdn_patch_rows_f32(x.data_ptr(), b, h, w, c, k[0], k[1], stride, stride, pad[0], pad[1], kpad, out.data_ptr(),
                                            _lib.stream_ptr()), "sdn_patch_rows_f32")


def pool3(mode, x, stride, pad, full, c0):
    """full: the [rows, ldo] map whose columns c0 .. c0 + C receive the result."""
    b, h, w, c = x.shape
    _lib.check(sda.lib().sdn_pool3_f32(mode, x.data_ptr(), b, h, w, c, stride, pad, full.data_ptr(), full.stride(0), c0, _lib.stream_ptr()),
               "sdn_pool3_f32")


def unfold_rows(x, k, stride, pad, kpad):
    """The patch matrix restated with F.unfold (channel-major columns) and reordered to (ky, kx, c), zero-padded to kpad."""
    b, h, w, c = x.shape
    cols = F.unfold(x.permute(0, 3, 1, 2), k, padding=pad, stride=stride)                  # [B, C kh kw, L]
    rows = cols.view(b, c, k[0] * k[1], -1).permute(0, 3, 2, 1).reshape(-1, k[0] * k[1] * c)
    return F.pad(rows, (0, kpad - rows.shape[1]))


# the kernel geometries of the trunk (ISSUE table): (H, W, C), kernel, stride, pad
GEOMETRIES = [((9, 7, 3), (3, 3), 2, (0, 0)), ((7, 7, 80), (1, 1), 1, (0, 0)), ((8, 5, 48), (5, 5), 1, (2, 2)),
              ((7, 9, 128), (1, 7), 1, (0, 3)), ((9, 7, 128), (7, 1), 1, (3, 0)), ((5, 5, 384), (1, 3), 1, (0, 1)),
              ((5, 5, 384), (3, 1), 1, (1, 0)), ((9, 9, 64), (3, 3), 2, (0, 0))]
GEO_IDS = [f"{h}x{w}x{c}-k{k[0]}x{k[1]}-s{s}-p{p[0]}{p[1]}" for (h, w, c), k, s, p in GEOMETRIES]


# ---- patch rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc, k, stride, pad", GEOMETRIES, ids=GEO_IDS)
def test_patch_rows_bit_equal_to_unfold(hwc, k, stride, pad):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, *hwc, generator=g).cuda()
    kpad = up(k[0] * k[1] * hwc[2], 64)
    rows = 2 * out_side(hwc[0], k[0], stride, pad[0]) * out_side(hwc[1], k[1], stride, pad[1])
    buf, out = X.guarded(rows, kpad, F32, "cuda")
    patch_rows(x, k, stride, pad, out, kpad)
    torch.cuda.synchronize()
    want = unfold_rows(x, k, stride, pad, kpad)
    assert want.shape == out.shape
    assert torch.equal(bits(out), bits(want))
    assert X.sentinels_intact(buf, out) == 0


# ---- pools -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w, stride, pad", [(9, 7, 2, 0), (8, 8, 2, 0), (3, 3, 1, 1)])
def test_max_pool_bit_equal_into_a_channel_slice(h, w, stride, pad):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, h, w, 64, generator=g).cuda()
    ho, wo = out_side(h, 3, stride, pad), out_side(w, 3, stride, pad)
    buf, full = X.guarded(2 * ho * wo, 256, F32, "cuda")
    pool3(0, x, stride, pad, full, 64)
    torch.cuda.synchronize()
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, 64)
    got = full[:, 64:128]
    assert torch.equal(bits(got), bits(want))
    assert X.sentinels_intact(buf, got) == 0                                               # columns 0..63 and 128..255 untouched


@pytest.mark.parametrize("h, w", [(1, 1), (3, 3), (5, 4)])
def test_average_pool_excludes_the_padding(h, w):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, h, w, 64, generator=g) + 0.5).cuda()
    buf, full = X.guarded(2 * h * w, 256, F32, "cuda")
    pool3(1, x, 1, 1, full, 64)
    torch.cuda.synchronize()
    pool = lambda t: F.avg_pool2d(t.to(F64).permute(0, 3, 1, 2), 3, stride=1, padding=1, count_include_pad=False).permute(0, 2, 3, 1).reshape(-1, 64)
    got = full[:, 64:128]
    # <= 8 additions and one division, each within 2^-24 of S = mean |x| over the window: 9 x 2^-24 < ACC = 2^-20
    st = X.analyse(got, pool(x), pool(x.abs()))
    assert not X.failures(st, exact_fn=False, direction=False), st
    assert X.sentinels_intact(buf, got) == 0
    if (h, w) == (1, 1):
        assert torch.equal(bits(got), bits(x.reshape(-1, 64)))                              # one tap, count 1: the value itself


# ---- resize -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [64, 256, 512, 299])
def test_resize_against_float64_interpolate(side):
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, side, side, generator=g)
    xd = x.cuda()
    buf, out = X.guarded_like((2, 299, 299, 3), F32, "cuda")
    _lib.check(sda.lib().sdn_resize_bilinear_f32(xd.data_ptr(), 2, side, side, 299, 299, 2.0, -1.0, out.data_ptr(), _lib.stream_ptr()),
               "sdn_resize_bilinear_f32")
    torch.cuda.synchronize()
    interp = lambda t: F.interpolate(t.to(F64), size=(299, 299), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    # every weight is >= 0, so sum |w| |x| = interp(|x|); 2 v - 1 carries S = 2 interp(|x|) + 1.  Roundings: two weights and their two
    # complements, six per row pair, three for the column blend, one for the -1 (2 x is exact): <= 14 x 2^-24 S < ACC = 2^-20 S
    st = X.analyse(out.cpu(), 2 * interp(x) - 1, 2 * interp(x.abs()) + 1)
    assert not X.failures(st, exact_fn=False, direction=False), st
    assert X.sentinels_intact(buf, out) == 0
    if side == 299:                                                                         # the same size: a layout change and 2 x - 1
        assert torch.equal(bits(out), bits(2 * xd.permute(0, 2, 3, 1) - 1))
    assert torch.equal(bits(resize_bilinear(xd, (299, 299), 2.0, -1.0)), bits(out))


# ---- spatial mean ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [9, 64])
def test_spatial_mean(hw):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3, hw, 2048, generator=g) + 1.0).cuda()
    buf, out = X.guarded(3, 2048, F32, "cuda")
    _lib.check(sda.lib().sdn_spatial_mean_f32(x.data_ptr(), 3, hw, 2048, out.data_ptr(), _lib.stream_ptr()), "sdn_spatial_mean_f32")
    torch.cuda.synchronize()
    # summed and divided in double, rounded to f32 once: 1/2 ulp and the double arithmetic's (hw + 1) x 2^-53 S
    st = X.analyse(out, x.to(F64).mean(1), x.to(F64).abs().mean(1), acc=2.0 ** -45)
    assert not X.failures(st, exact_fn=False, direction=False), st
    assert X.sentinels_intact(buf, out) == 0


# ---- one convolution per geometry ---------------------------------------------------------------------------------------------------------
def test_f32_gemm_takes_the_relu_code_and_still_refuses_six_and_eight():
    a, w = torch.randn(64, 64).cuda(), torch.randn(32, 64).cuda()
    got = ops.gemm(a, w, act=9)
    torch.cuda.synchronize()
    y = a.to(F64) @ w.to(F64).T
    st = X.analyse(got, y.clamp_min(0), a.to(F64).abs() @ w.to(F64).abs().T, acc=X.X3_ACC["f32"])
    assert not X.failures(st, exact_fn=False, direction=False), st
    assert bool((got == 0).any()) and bool((got > 0).any())
    for code in (6, 8, 10):
        with pytest.raises(sda.SdnError):
            ops.gemm(a, w, act=code)
    for half in (torch.bfloat16, torch.float16):
        with pytest.raises(sda.SdnError):
            ops.gemm(torch.randn(128, 128).cuda().to(half), torch.randn(256, 128).cuda().to(half), act=9)


@pytest.mark.parametrize("cout", [80, 48])
@pytest.mark.parametrize("hwc, k, stride, pad", GEOMETRIES, ids=GEO_IDS)
def test_convolution_as_patch_rows_and_gemm(hwc, k, stride, pad, cout):
    """BasicConv2d with its norm folded: patch rows, sdn_gemm_f32 with bias + ReLU, n_valid = cout under N = cout rounded up to 32
    (80 -> 96, 48 -> 64), into columns 32 .. 32 + cout of a 160-wide map; against float64 F.conv2d."""
    g = torch.Generator().manual_seed(6)
    cin, kk = hwc[2], k[0] * k[1] * hwc[2]
    x = torch.randn(2, *hwc, generator=g).cuda()
    w = (torch.randn(cout, cin, *k, generator=g) * kk ** -0.5).cuda()
    bias = torch.randn(cout, generator=g).cuda()
    kpad, npad = up(kk, 64), up(cout, 32)
    wp = torch.zeros(npad, kpad, device="cuda")
    wp[:cout, :kk] = w.permute(0, 2, 3, 1).reshape(cout, -1)
    bp = torch.zeros(npad, device="cuda")
    bp[:cout] = bias
    rows = 2 * out_side(hwc[0], k[0], stride, pad[0]) * out_side(hwc[1], k[1], stride, pad[1])
    pr = torch.empty(rows, kpad, device="cuda")
    patch_rows(x, k, stride, pad, pr, kpad)
    buf, full = X.guarded(rows, 160, F32, "cuda")
    got = full[:, 32:32 + cout]
    ops.gemm(pr, wp, bias=bp, act=9, out_kind=1, n_valid=cout, out=got)
    torch.cuda.synchronize()
    conv = lambda a, b, c: F.conv2d(a.to(F64).permute(0, 3, 1, 2), b.to(F64), c.to(F64), stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(rows, cout)
    y, s = conv(x, w, bias), conv(x.abs(), w.abs(), bias.abs())
    st = X.analyse(got, y.clamp_min(0), s, acc=X.X3_ACC["f32"])                             # ReLU is 1-Lipschitz: S passes through
    assert not X.failures(st, exact_fn=False, direction=False), st
    assert X.sentinels_intact(buf, got) == 0


# ---- the trunk ------------------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.to(F64).cpu(), b.to(F64).cpu()
    return float((a - b).norm() / b.norm())


def test_whole_trunk_against_the_float64_oracle():
    """resize_input=False at 139 x 139, B = 3: maps of 69, 67, 33, 31, 15, 7 and 3 -- every map odd.  The engine must be within 4 x
    the distance of the SAME trunk evaluated in float32 on the CPU from its float64 run: both are fp32 arithmetic and differ only in
    summation order and the one extra rounding of the fold.
    Measured on MI355X (profiles/inception_parity.json): engine 7.81e-7, float32 on the CPU 3.61e-7 (bound 1.45e-6)."""
    tower = InceptionV3(resize_input=False, image_size=139)
    sd = tower.synthetic_state_dict(11)
    tower.load_state_dict(sd)
    x = torch.rand(3, 3, 139, 139, generator=torch.Generator().manual_seed(12))
    got = tower(x.cuda())
    torch.cuda.synchronize()
    assert got.shape == (3, 2048) and got.dtype == F32 and bool(torch.isfinite(got).all())
    ref64 = oracle.forward(sd, x, resize_input=False, dtype=F64)
    ref32 = oracle.forward(sd, x, resize_input=False, dtype=F32)
    cpu32, eng = rel_l2(ref32, ref64), rel_l2(got, ref64)
    print(f"trunk rel-L2 vs float64: engine {eng:.3e}, float32 on the CPU {cpu32:.3e}")
    record("trunk_139_b3", {"engine_rel_l2": eng, "cpu_float32_rel_l2": cpu32, "bound": 4 * cpu32, "features_rms": float(ref64.pow(2).mean().sqrt())})
    assert eng <= 4 * cpu32


@pytest.fixture(scope="module")
def tower299():
    t = InceptionV3()
    t.load_state_dict(t.synthetic_state_dict(13))
    return t


def test_full_path_at_256(tower299):
    x = torch.rand(5, 3, 256, 256, generator=torch.Generator().manual_seed(14)).cuda()
    two = tower299(x[:2])
    assert two.shape == (2, 2048) and two.dtype == F32 and bool(torch.isfinite(two).all())
    # the resize inside the plan == the tower without resize on the separately resized tensor
    plain = InceptionV3(resize_input=False)
    plain._weights = tower299._weights                                                     # the same packed buffer: packing knows no resize flag
    resized = resize_bilinear(x[:2], (299, 299)).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(bits(plain(resized)), bits(two))
    # an image's features: alone, inside a batch of 5, across a chunk boundary
    alone = tower299(x[3:4])
    five = tower299(x)
    assert torch.equal(bits(five[3:4]), bits(alone)) and torch.equal(bits(five[:2]), bits(two))
    tower299.CHUNK = 2
    try:
        chunked = tower299(x)                                                              # chunks 2 + 2 + 1
    finally:
        del tower299.CHUNK
    assert torch.equal(bits(chunked), bits(five))
    u8 = (x[:2] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()             # uint8 input = ToTensor's u8 / 255
    assert torch.equal(bits(tower299(u8)), bits(tower299(u8.permute(0, 3, 1, 2).float() / 255.0)))


def test_evaluate_fid_on_two_directories(tower299, tmp_path):
    from PIL import Image
    import yaml
    rng = np.random.default_rng(15)
    for name, lo, hi in (("samples", 0, 160), ("reference", 96, 256)):                      # two clearly different sets
        (tmp_path / name).mkdir()
        for i in range(6):
            side = (96, 128)[i % 2]                                                          # mixed sizes: Resize((256, 256)) comes first
            Image.fromarray(rng.integers(lo, hi, (side, side, 3), dtype=np.uint8)).save(tmp_path / name / f"{i}.png")
    out = M.evaluate_fid(str(tmp_path / "samples"), dataset_root=str(tmp_path / "reference"), batch_size=4, tower=tower299,
                         filename="fid_test", subsets=10, generator=torch.Generator().manual_seed(16))
    with open(tmp_path / "fid_test.yaml") as f:
        assert yaml.safe_load(f) == out
    print(out)
    assert set(out) == {"fid", "kid", "log_kid"} and all(np.isfinite(v) for v in out.values())
    assert out["fid"] > 0 and out["kid"] > 0
    # a directory against itself
    fid = M.FrechetInceptionDistance(tower299, batch_size=4)
    imgs = [Image.open(tmp_path / "samples" / f"{i}.png") for i in range(6)]
    fid.update(imgs, real=True)
    fid.update(imgs)
    tr = float(np.trace(fid._sets[False].mean_cov()[1]))
    same = M.evaluate_fid(str(tmp_path / "samples"), dataset_root=str(tmp_path / "samples"), batch_size=4, tower=tower299, subsets=2)
    print(f"FID(A, A) = {same['fid']:.3e}, tr = {tr:.3e}")
    assert abs(same["fid"]) <= 1e-6 * tr and abs(fid.compute()) <= 1e-6 * tr
    assert fid.state() == (0.0, 6)

