"""Host-side checks of the AutoencoderKL precision plans (sdn_vae_config.dtype 2 = fp32, 3 = bf16x3; no GPU is touched): both creates
accept the modes, the manifest and FLOPs equal the 16-bit plan's with f32 matrices, the chunk cap of the entry points, the argument checks of the new operators and the Python surface -- and the float64
reference of tests/test_gpu_vae_precise.py (tests_support/vae_oracle64.py) against the oracle it restates."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from oracle.vae import OracleVAEDecoder, OracleVAEEncoder, decoder_state_dict_shapes, encoder_state_dict_shapes
from safe_denoiser_amd import _lib
from safe_denoiser_amd.vae import SD3_VAE_CONFIG, AutoencoderKL
from tests_support.vae_oracle64 import OracleVAE64, rel_l2

PRECISE = ("fp32", "bf16x3")
SMALL = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=16)
SMALL_O = dict(block_out_channels=(64, 128), layers_per_block=1)


def _config(dtype, small):
    boc = (64, 128, 0, 0) if small else (128, 256, 512, 512)
    return _lib.VaeConfig(latent_channels=4, out_channels=3, sample_size=8 if small else 64, n_levels=2 if small else 4,
                          block_out_channels=(C.c_int32 * 4)(*boc), layers_per_block=1 if small else 2, norm_groups=32, dtype=dtype)


def _all_params(h):
    info, out = _lib.ParamInfo(), []
    for i in range(sda.lib().sdn_unet_param_count(h)):
        _lib.check(sda.lib().sdn_unet_param_info(h, i, C.byref(info)), "sdn_unet_param_info")
        out.append((info.name.decode(), info.kind, info.rows, info.cols, info.rows_padded))
    return out


@pytest.mark.parametrize("create", ["sdn_vae_decoder_create", "sdn_vae_encoder_create"])
@pytest.mark.parametrize("small", [True, False], ids=["small", "sd14"])
def test_both_creates_accept_the_precise_modes_with_the_16_bit_manifest(create, small):
    lib = sda.lib()
    fn = getattr(lib, create)
    h0 = C.c_void_p()
    assert fn(C.byref(_config(0, small)), C.byref(h0)) == 0
    ref, ref_bytes = _all_params(h0), lib.sdn_unet_weight_bytes(h0)
    a0 = C.c_double()
    f0 = lib.sdn_unet_flops(h0, 2, C.byref(a0))
    for dt in (2, 3):
        h = C.c_void_p()
        assert fn(C.byref(_config(dt, small)), C.byref(h)) == 0
        assert _all_params(h) == ref                                   # names, kinds, shapes and padding; no derived regions
        assert lib.sdn_unet_weight_bytes(h) > ref_bytes                # f32 matrices
        a = C.c_double()
        assert lib.sdn_unet_flops(h, 2, C.byref(a)) == f0 and a.value == a0.value and f0 > 0     # algorithmic FLOPs: storage-independent
        assert lib.sdn_unet_workspace_bytes(h, 1) > lib.sdn_unet_workspace_bytes(h0, 1)
        lib.sdn_unet_destroy(h)
    for bad in (4, -1):
        h = C.c_void_p()
        assert fn(C.byref(_config(bad, small)), C.byref(h)) == -1
    lib.sdn_unet_destroy(h0)


def _chunk_cap(h):
    """The batch at which the workspace stops growing: the entry points replay the plan on chunks of that many images."""
    ws = [sda.lib().sdn_unet_workspace_bytes(h, b) for b in range(1, 11)]
    assert ws[0] > 0
    for b in range(1, 10):
        if ws[b] == ws[b - 1]:
            assert all(w == ws[b] for w in ws[b:])
            return b
        assert ws[b] > ws[b - 1]
    raise AssertionError("the workspace never stops growing")


@pytest.mark.parametrize("create", ["sdn_vae_decoder_create", "sdn_vae_encoder_create"])
def test_precise_plans_take_at_most_half_the_16_bit_chunk(create):
    """Full SD-v1.4 at 512 x 512: the 16-bit plans replay 8 images per chunk; 4 bytes per element halve that (vae_chunk())."""
    fn = getattr(sda.lib(), create)
    caps = {}
    for dt in (0, 2, 3):
        h = C.c_void_p()
        assert fn(C.byref(_config(dt, False)), C.byref(h)) == 0
        caps[dt] = _chunk_cap(h)
        sda.lib().sdn_unet_destroy(h)
    assert caps[0] == 8 and caps[2] == caps[3] == 4
    assert 2 * caps[2] <= caps[0] and 2 * caps[3] <= caps[0]


def test_python_surface_and_chunk_bounds():
    with pytest.raises(_lib.SdnError):
        AutoencoderKL(precision="nonsense", **SMALL)
    with pytest.raises(_lib.SdnError):
        AutoencoderKL(dtype=torch.float64, **SMALL)
    v = AutoencoderKL(dtype=torch.float32, **SMALL)
    assert v.precision == "fp32" and v.dtype == torch.float32
    assert AutoencoderKL(**SMALL).precision is None
    for precision in PRECISE:
        v = AutoencoderKL(dtype=torch.float16, precision=precision, **SMALL)
        assert v.dtype == torch.float32 and v.precision == precision and v.MAX_CHUNK == 4
        enc = v._encoder()                                             # the lazily built encoder half inherits the mode
        assert enc.precision == precision and enc.dtype == torch.float32 and enc._role == "encoder"
        lo = AutoencoderKL(**SMALL)
        assert v.state_dict_shapes() == lo.state_dict_shapes() and enc.state_dict_shapes() == lo._encoder().state_dict_shapes()
        assert v.state_dict_shapes() == decoder_state_dict_shapes(SMALL_O)
        assert enc.state_dict_shapes() == encoder_state_dict_shapes(SMALL_O)
        # every matrix is packed as f32, bit for bit (conv kernels [O, I, 3, 3] -> [O][ky][kx][I])
        sd = v.synthetic_state_dict(3)
        buf = v.pack_state_dict(sd)
        assert buf.numel() == v.weight_bytes
        for p in v.manifest:
            t = sd[p["name"]].float()
            t = t.permute(0, 2, 3, 1) if (t.dim() == 4 and t.shape[-1] == 3) else t
            got = buf[p["offset"]:p["offset"] + 4 * t.numel()].view(torch.float32)
            assert torch.equal(got, t.reshape(-1)), p["name"]
    # full size: 512 x 512 -> 4 images per chunk, 1024 x 1024 -> 1 (the 1 GiB map behind the last upsampler), SD-v3's the same
    assert AutoencoderKL(precision="fp32").MAX_CHUNK == 4 and AutoencoderKL().MAX_CHUNK == 8
    assert AutoencoderKL(precision="bf16x3", sample_size=1024).MAX_CHUNK == 1
    assert AutoencoderKL(precision="bf16x3", **SD3_VAE_CONFIG).config.latent_channels == 16


def test_new_operators_reject_bad_arguments_on_host():
    lib = sda.lib()
    A = 0x10000                                                          # 16-byte aligned stand-ins; nothing is dereferenced

    def sm(dtype=2, s=A, n=64, rows=3, out=A + 0x4000, ld_s=None, ld_o=None):
        return lib.sdn_softmax_rows(dtype, s, n if ld_s is None else ld_s, rows, n, 0.125, out, n if ld_o is None else ld_o, None)
    assert sm(out=A + 0x4008) == -1 and sm(s=A + 4) == -1               # f32 probabilities are written as float4
    assert sm(dtype=0, out=A + 0x4008, rows=0) == 0                      # (8-byte alignment is the 16-bit rule)
    assert sm(n=66) == -1 and sm(n=16388) == -1 and sm(n=0) == -1
    assert sm(ld_o=60) == -1 and sm(ld_s=60) == -1 and sm(ld_o=66) == -1
    assert sm(dtype=3) == -1 and sm(dtype=-1) == -1
    assert sm(s=None) == -1 and sm(out=None) == -1
    assert sm(rows=0) == 0 and sm(n=16384, rows=0) == 0

    def tr(i=A, rows=100, cols=72, ld_in=216, out=A + 0x8000, ld_out=100):
        return lib.sdn_transpose32(i, rows, cols, ld_in, out, ld_out, None)
    assert tr(i=None) == -1 and tr(out=None) == -1
    assert tr(i=A + 2) == -1 and tr(out=A + 0x8001) == -1               # not 4-byte aligned
    assert tr(rows=0) == -1 and tr(cols=0) == -1 and tr(ld_in=71) == -1 and tr(ld_out=99) == -1


@pytest.mark.parametrize("seed", [3, 9])
def test_float64_reference_is_the_oracle_in_double(seed):
    """An fp32 evaluation cannot be further than ~1e-6 from its own float64 at this depth (some 20 normalised layers): 1e-5 or the
    restatement in tests_support/vae_oracle64.py is wrong."""
    v = AutoencoderKL(**SMALL)
    sd = v.synthetic_state_dict(seed, with_encoder=True)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(3, 4, 8, 8, generator=g)
    x = torch.randn(3, 3, 16, 16, generator=g).clamp(-1, 1)
    o64 = OracleVAE64(sd, SMALL_O)
    d64, e64 = o64.decode(z, 1.0 / 0.18215), o64.encode(x)
    assert d64.dtype == torch.float64 and e64.dtype == torch.float64 and d64.shape == (3, 3, 16, 16) and e64.shape == (3, 8, 8, 8)
    rd = rel_l2(OracleVAEDecoder(sd, SMALL_O, act_dtype=None).decode(z, 1.0 / 0.18215), d64)
    re_ = rel_l2(OracleVAEEncoder(sd, SMALL_O, act_dtype=None).encode(x), e64)
    print(f"fp32 oracle vs float64 reference: decoder {rd:.3e}, encoder {re_:.3e}")
    assert 0 < rd <= 1e-5 and 0 < re_ <= 1e-5
    # the blocked attention (more than Q_BLOCK tokens) is the same function: here 64 tokens in blocks of 16
    blocked = OracleVAE64(sd, SMALL_O)
    blocked.Q_BLOCK = 16
    torch.testing.assert_close(blocked.decode(z, 1.0 / 0.18215), d64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(blocked.encode(x), e64, rtol=1e-12, atol=1e-12)
    # the uint8 tail in double agrees with the fp32 oracle's up to single flips at rounding boundaries
    lat = z * 0.18215
    u64 = o64.image_uint8(lat)
    u32 = OracleVAEDecoder.to_uint8(OracleVAEDecoder(sd, SMALL_O, act_dtype=None).decode_latents(lat))
    assert u64.shape == u32.shape == (3, 16, 16, 3) and int((u64.int() - u32.int()).abs().max()) <= 1
