"""AutoencoderKL precision plans on the GPU (sdn_vae_config.dtype 2 = fp32, 3 = bf16x3) against a FLOAT64 evaluation of the oracle
(tests_support/vae_oracle64.py, pinned by tests/test_vae_precise_host.py).

Bounds.  rel L2 against float64 throughout.
  fp32:   4 x e32, where e32 is the distance of the CPU fp32 oracle (act_dtype=None) from the same float64 reference on the same
          inputs, computed here.  Both are fp32 evaluations of one function; they differ in summation order only (the engine's k loop
          sums strictly in order, the CPU's GEMMs in blocks), the margin tests/test_gpu_inception.py gives the same situation.
  bf16x3: 1e-4 per forward, the bound tests/test_gpu_mmdit_precise.py holds a bf16x3 network to (products to 2^-17 relative).
  f32 softmax, per element: t = scale * s is rounded at |t| <= 80 (4.8e-6 absolute), so is the row maximum, and t - max at up to 160
          (9.5e-6): the exponent is off by at most 1.9e-5, in the numerator and -- coherently, at worst -- in every term of the sum;
          expf, the 14-deep summation tree and the division add ~1e-6.  rtol 4e-5; atol 1e-37 for probabilities below the f32 normal
          range (the float64 softmax still resolves exp(-160)).  The row sum over the kernel's OWN probabilities sees only the tree's
          rounding and the divisions': 1e-6.
"""
import numpy as np
import pytest
import torch

from oracle.vae import OracleVAEDecoder, OracleVAEEncoder
from safe_denoiser_amd import _lib
from safe_denoiser_amd.vae import SD3_VAE_CONFIG, AutoencoderKL
from tests_support.vae_oracle64 import OracleVAE64, rel_l2

pytestmark = pytest.mark.gpu

PRECISE = ("fp32", "bf16x3")
SMALL = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=16)
SMALL_O = dict(block_out_channels=(64, 128), layers_per_block=1)
SCALE = 1.0 / 0.18215


def bound(precision, e32):
    return 4.0 * e32 if precision == "fp32" else 1e-4


# ---------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("n,rows", [(64, 7), (4096, 5), (16384, 3)])
def test_f32_softmax_rows_against_float64(n, rows):
    lib = _lib.lib()
    scale = 0.0442
    g = torch.Generator().manual_seed(n)
    s = (torch.rand(rows, n, generator=g) * 2 - 1) * (80.0 / scale)          # scale * s spans +-80: exp(80) overflows unshifted f32
    s[:, 1], s[:, n - 2] = 80.0 / scale, -80.0 / scale
    sd = s.cuda()
    p = torch.full((rows, n), float("nan"), device="cuda")
    _lib.check(lib.sdn_softmax_rows(2, sd.data_ptr(), n, rows, n, scale, p.data_ptr(), n, _lib.stream_ptr()), "softmax f32")
    p = p.cpu()
    ref = torch.softmax(s.double() * float(np.float32(scale)), dim=-1)
    assert torch.isfinite(p).all() and float(p.max()) > 1e-3
    worst = float(((p.double() - ref).abs() / ref.clamp_min(1e-30)).max())
    sums = p.double().sum(-1)
    print(f"f32 softmax n={n}: worst relative error {worst:.3e}, row sums within {float((sums - 1).abs().max()):.3e} of 1")
    torch.testing.assert_close(p.double(), ref, rtol=4e-5, atol=1e-37)
    torch.testing.assert_close(sums, torch.ones(rows, dtype=torch.float64), rtol=0, atol=1e-6)


@pytest.mark.parametrize("rows,cols,ld_in,ld_out", [(64, 128, 128, 64), (4096, 512, 512, 4096), (100, 72, 3 * 72, 104)])
def test_transpose32_is_bit_exact(rows, cols, ld_in, ld_out):
    lib = _lib.lib()
    m = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, ld_in), dtype=torch.int32, generator=torch.Generator().manual_seed(rows)).cuda()
    off = ld_in - cols                                                        # the strided view's first column (0 when dense)
    t = torch.full((cols, ld_out), 7, dtype=torch.int32, device="cuda")
    _lib.check(lib.sdn_transpose32(m.data_ptr() + 4 * off, rows, cols, ld_in, t.data_ptr(), ld_out, _lib.stream_ptr()), "transpose32")
    assert torch.equal(t[:, :rows].cpu(), m[:, off:off + cols].cpu().t())
    assert bool((t[:, rows:] == 7).all())                                     # nothing written past `rows` of an output row


def test_new_operators_refuse_bad_arguments_without_launching():
    lib = _lib.lib()
    s = torch.zeros(4, 64, device="cuda")
    p = torch.zeros(4, 64, device="cuda")
    a = (s.data_ptr(), p.data_ptr())
    assert lib.sdn_softmax_rows(2, a[0], 64, 4, 64, 1.0, a[1] + 8, 64, None) == -1          # misaligned f32 output
    assert lib.sdn_softmax_rows(2, a[0] + 4, 64, 4, 64, 1.0, a[1], 64, None) == -1
    assert lib.sdn_softmax_rows(2, a[0], 64, 4, 62, 1.0, a[1], 64, None) == -1              # n % 4
    assert lib.sdn_softmax_rows(2, a[0], 16388, 4, 16388, 1.0, a[1], 16388, None) == -1     # n > 16384
    assert lib.sdn_softmax_rows(3, a[0], 64, 4, 64, 1.0, a[1], 64, None) == -1
    assert lib.sdn_transpose32(a[0] + 2, 4, 64, 64, a[1], 4, None) == -1
    assert lib.sdn_transpose32(a[0], 4, 64, 63, a[1], 4, None) == -1 and lib.sdn_transpose32(a[0], 4, 64, 64, a[1], 3, None) == -1
    torch.cuda.synchronize()
    assert float(p.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------- small decoder / encoder
@pytest.fixture(scope="module")
def small_case():
    """Weights, inputs, the float64 reference and the fp32 oracle's own distance from it: computed once, never modified."""
    sd = AutoencoderKL(**SMALL).synthetic_state_dict(3, with_encoder=True)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(3, 4, 8, 8, generator=g)
    x = torch.randn(3, 3, 16, 16, generator=g).clamp(-1, 1)
    o64 = OracleVAE64(sd, SMALL_O)
    d64, m64 = o64.decode(z, SCALE), o64.encode(x)
    e32_d = rel_l2(OracleVAEDecoder(sd, SMALL_O, act_dtype=None).decode(z, SCALE), d64)
    e32_e = rel_l2(OracleVAEEncoder(sd, SMALL_O, act_dtype=None).encode(x), m64)
    return dict(sd=sd, z=z, x=x, d64=d64, m64=m64, e32_d=e32_d, e32_e=e32_e)


@pytest.fixture(scope="module")
def small_vaes(small_case):
    out = {}
    for precision in PRECISE:
        v = AutoencoderKL(precision=precision, **SMALL)
        v.load_state_dict(small_case["sd"])
        out[precision] = v
    return out


@pytest.mark.parametrize("precision", PRECISE)
def test_small_decoder_against_float64(small_case, small_vaes, precision):
    c, v = small_case, small_vaes[precision]
    v.profile_next()
    img = v.decode(c["z"].cuda(), latent_scale=SCALE).sample
    kernels = {r["kernel"] for r in v.profile_read()}
    assert img.shape == (3, 3, 16, 16) and img.dtype == torch.float32 and torch.isfinite(img).all()
    r = rel_l2(img, c["d64"])
    print(f"small VAE decoder {precision}: rel L2 vs float64 {r:.3e}; fp32 CPU oracle e32 {c['e32_d']:.3e}; bound {bound(precision, c['e32_d']):.3e}")
    assert r <= bound(precision, c["e32_d"])
    # what ran: the fp32 interpreter's kernels (M = 3 x 64 rows and up: every contraction of the bf16x3 plan on k_gemm_x3)
    assert kernels == {"k_latent_mix", "k_conv_in_f32", "k_gn_rows_f32", "k_transpose32", "k_softmax_rows_f32",
                       "k_gemm_f32" if precision == "fp32" else "k_gemm_x3"}
    # batch rows are independent, bit for bit
    torch.testing.assert_close(v.decode(c["z"][1:2].cuda(), latent_scale=SCALE).sample, img[1:2], rtol=0, atol=0)


@pytest.mark.parametrize("precision", PRECISE)
def test_small_encoder_against_float64_and_the_sampling_path(small_case, small_vaes, precision):
    c, v = small_case, small_vaes[precision]
    dist = v.encode(c["x"].cuda()).latent_dist
    mom = dist.parameters
    assert mom.shape == (3, 8, 8, 8) and mom.dtype == torch.float32 and torch.isfinite(mom).all()
    assert v.encoder_half.precision == precision
    r = rel_l2(mom, c["m64"])
    print(f"small VAE encoder {precision}: moments rel L2 vs float64 {r:.3e}; fp32 CPU oracle e32 {c['e32_e']:.3e}; bound {bound(precision, c['e32_e']):.3e}")
    assert r <= bound(precision, c["e32_e"])
    torch.testing.assert_close(v.encode(c["x"][1:2].cuda()).latent_dist.parameters, mom[1:2], rtol=0, atol=0)
    # latent_dist on a precise encoder: mode, and sample = (mean + std * randn(generator)) * scale (tolerances of tests/test_gpu_vae.py)
    torch.testing.assert_close(dist.mode(0.18215), dist.mean * 0.18215, rtol=1e-6, atol=1e-7)
    zs = dist.sample(torch.Generator(device="cuda").manual_seed(9), scale=0.18215)
    noise = torch.randn(dist.mean.shape, generator=torch.Generator(device="cuda").manual_seed(9), device="cuda")
    torch.testing.assert_close(zs, (dist.mean + dist.std * noise) * 0.18215, rtol=1e-5, atol=1e-6)
    # the reference's embed_fn, seeded, as driver.build_repellency takes it
    e1 = v.embed_fn(torch.Generator(device="cuda").manual_seed(3))(c["x"].cuda())
    e2 = v.embed_fn(torch.Generator(device="cuda").manual_seed(3))(c["x"].cuda())
    torch.testing.assert_close(e1, e2, rtol=0, atol=0)


def test_precise_decoder_with_more_than_4096_attention_tokens():
    """16384 tokens: four query blocks of 4096 over 16384 keys (f32 softmax rows at the limit, V^T 64 x 16384)."""
    cfg = dict(block_out_channels=(64, 64), layers_per_block=1, sample_size=256)
    ocfg = dict(block_out_channels=(64, 64), layers_per_block=1)
    v = AutoencoderKL(precision="fp32", **cfg)
    sd = v.synthetic_state_dict(5)
    v.load_state_dict(sd)
    z = torch.randn(1, 4, 128, 128, generator=torch.Generator().manual_seed(2))
    img = v.decode(z.cuda()).sample
    d64 = OracleVAE64(sd, ocfg).decode(z)
    e32 = rel_l2(OracleVAEDecoder(sd, ocfg, act_dtype=None).decode(z), d64)
    r = rel_l2(img, d64)
    print(f"fp32 VAE decoder with 16384 attention tokens: rel L2 vs float64 {r:.3e}; fp32 CPU oracle e32 {e32:.3e}")
    assert img.shape == (1, 3, 256, 256) and r <= 4.0 * e32


def test_precise_sd3_style_vae():
    """16 latent channels, no (post_)quant_conv, decode(latents / scaling_factor + shift_factor), in fp32."""
    cfg = dict(SD3_VAE_CONFIG, block_out_channels=(64, 128), layers_per_block=1, sample_size=16)
    v = AutoencoderKL(precision="fp32", **cfg)
    sd = {k: t for k, t in v.synthetic_state_dict(9).items() if not k.startswith("post_quant_conv")}
    v.load_state_dict(sd)
    lat = torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(4)) * 1.5
    got = v.decode(v._unscale(lat.cuda()), latent_scale=1.0 / v.config.scaling_factor).sample
    osd = dict(sd)
    osd["post_quant_conv.weight"], osd["post_quant_conv.bias"] = torch.eye(16).reshape(16, 16, 1, 1), torch.zeros(16)
    ocfg = dict(latent_channels=16, block_out_channels=(64, 128), layers_per_block=1)
    d64 = OracleVAE64(osd, ocfg).decode(lat.double() / 1.5305 + 0.0609)
    e32 = rel_l2(OracleVAEDecoder(osd, ocfg, act_dtype=None).decode(lat / 1.5305 + 0.0609), d64)
    r = rel_l2(got, d64)
    print(f"fp32 SD-v3 style VAE decoder: rel L2 vs float64 {r:.3e}; fp32 CPU oracle e32 {e32:.3e}")
    assert got.shape == (2, 3, 16, 16) and r <= 4.0 * e32
    im = torch.from_numpy(v.decode_latents(lat.cuda()))
    assert float((im.double() - (d64 / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1)).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------- images
def test_precise_images_against_the_float64_image():
    """The small pipeline of tests/test_gpu_vae.py::test_pipeline_ends_like_the_reference_with_images: its final latents decoded to
    uint8 by a precise VAE, against round_half_even(255 clamp(x / 2 + 0.5, 0, 1)) of the float64 decoder.  The bf16 VAE -- the
    parent's behaviour -- is the yardstick for the share of differing values."""
    from safe_denoiser_amd.pipeline import SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import DDPMScheduler
    from safe_denoiser_amd.unet import UNet2DConditionModel
    u = UNet2DConditionModel(text_len=77, block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                             layers_per_block=1, attention_head_dim=8, cross_attention_dim=768, sample_size=16)
    u.load_state_dict(u.synthetic_state_dict(11))
    vcfg = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=32)
    lo = AutoencoderKL(**vcfg)
    sd = lo.synthetic_state_dict(4)
    lo.load_state_dict(sd)
    E = torch.randn(4, 77, 768, generator=torch.Generator().manual_seed(2)).cuda()
    gens = [torch.Generator(device="cuda").manual_seed(7 + i) for i in range(2)]
    lat = SafeDenoiserPipeline(u, DDPMScheduler(), variant="threshold_time", vae=lo)(
        prompt_embeddings=E, num_inference_steps=4, generator=gens, return_latents=True)
    ref = OracleVAE64(sd, SMALL_O).image_uint8(lat.cpu()).int()
    share_lo = float((lo.decode_latents_uint8(lat).cpu().int() != ref).float().mean())
    for precision in PRECISE:
        v = AutoencoderKL(precision=precision, **vcfg)
        v.load_state_dict(sd)
        u8 = v.decode_latents_uint8(lat).cpu()
        assert u8.shape == (2, 32, 32, 3) and u8.dtype == torch.uint8
        d = (u8.int() - ref).abs()
        share = float((d > 0).float().mean())
        print(f"uint8 image, {precision}: {share * 100:.3f} % of values differ from the float64 image (max {int(d.max())} level); bf16 VAE: {share_lo * 100:.1f} %")
        assert int(d.max()) <= 1
        assert share < share_lo


# ---------------------------------------------------------------------------------------------------- from_pretrained
def test_from_pretrained_vae_precision(tmp_path):
    from safe_denoiser_amd.clip import CLIPTextModel
    from safe_denoiser_amd.pipeline import SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import DDPMScheduler
    from safe_denoiser_amd.unet import UNet2DConditionModel
    from tests.test_gpu_from_pretrained import VAE_CFG, _write_checkpoint
    from tests.test_gpu_pipeline import SMALL as UNET_SMALL
    from tests.test_gpu_safree_call import CLIP_CFG
    from tests_support.fake_tokenizer import FakeCLIPTokenizer
    root = str(tmp_path / "ckpt")
    usd, vsd, csd = _write_checkpoint(root)
    tok = FakeCLIPTokenizer(vocab_size=CLIP_CFG["vocab_size"])
    hi = SafeDenoiserPipeline.from_pretrained(root, latent_repeat=3, tokenizer=tok, vae_precision="bf16x3")
    assert hi.vae.precision == "bf16x3" and hi.vae.dtype == torch.float32 and hi.unet.dtype == torch.bfloat16
    pipe = SafeDenoiserPipeline.from_pretrained(root, latent_repeat=3, tokenizer=tok)
    assert pipe.vae.precision is None and pipe.vae.dtype == torch.bfloat16                 # the default: the 16-bit VAE, as before
    # ... and the images of a pipeline built by hand the way from_pretrained built it before `vae_precision` existed
    u = UNet2DConditionModel(text_len=77, latent_repeat=3, **UNET_SMALL); u.load_state_dict(usd)
    v = AutoencoderKL(**VAE_CFG); v.load_state_dict(vsd)
    c = CLIPTextModel(precision="bf16x3", **CLIP_CFG); c.load_state_dict(csd)
    direct = SafeDenoiserPipeline(u, DDPMScheduler(), variant="threshold_time", vae=v, text_encoder=c, tokenizer=tok)
    prompt = "a painting of a woman standing near the sea , lustful mood"
    call = lambda p: p(prompt, generator=torch.Generator(device="cuda").manual_seed(11), num_inference_steps=3, height=128, width=128,
                       output_type="np", safree_dict={"lra": True})
    a, b, h = call(pipe), call(direct), call(hi)
    assert a.shape == (1, 32, 32, 3) and np.array_equal(a, b)
    assert h.shape == a.shape and float(np.abs(h - a).mean()) <= 5e-3                     # same latents, the precise decoder
