"""The handles whose plans tools/plan_fingerprint.py prints and tests/test_plan_digests.py pins: every configuration the host tests
create (full-size and small UNet, MMDiT, VAE decoder / encoder, CLIP, projected CLIP, T5, the CLIP vision towers and the Inception
tower) at every storage dtype its creator accepts, the UNet ones under every plan-rebuilding toggle as well.  Host only."""
import ctypes as C
import hashlib

from safe_denoiser_amd import _lib
from safe_denoiser_amd.clip import ACT_CODES, SD3_CLIP_G_CONFIG, SD3_CLIP_L_CONFIG, SD14_CLIP_CONFIG
from safe_denoiser_amd.clip_vision import VIT_H14_CONFIG, VIT_L14_CONFIG
from safe_denoiser_amd.mmdit import SD3_MEDIUM
from safe_denoiser_amd.t5 import T5_XXL_CONFIG
from safe_denoiser_amd.unet import SD14_CONFIG
from safe_denoiser_amd.vae import SD14_VAE_CONFIG

BATCHES = (1, 3, 6, 64, 65)
T5_LENGTHS = (2, 77, 512)
# (label, setter, value): sdn_unet_set_split_k / _conv_up4, every plan-rebuilding debug hook at its non-default value, sub-batching
UNET_TOGGLES = [("plain", None, 0), ("split_k", "sdn_unet_set_split_k", 1), ("x3_expand=0", "sdn_debug_set_x3_expand", 0),
                ("res_pre=0", "sdn_debug_set_res_pre", 0), ("ln_fold=0", "sdn_debug_set_ln_fold", 0),
                ("ln_prepass_all=1", "sdn_debug_set_ln_prepass_all", 1), ("ffn_fuse=0", "sdn_debug_set_ffn_fuse", 0),
                ("ff_fuse=0", "sdn_debug_set_ff_fuse", 0), ("ffn_own_stats=0", "sdn_debug_set_ffn_own_stats", 0),
                ("x3_pairs=0", "sdn_debug_set_x3_pairs", 0), ("gn_fuse=0", "sdn_debug_set_gn_fuse", 0),
                ("subbatch=24MiB", "sdn_debug_set_subbatch_bytes", 24 << 20), ("conv_up4=0", "sdn_unet_set_conv_up4", 0),
                ("gemm_k320=0", "sdn_debug_set_gemm_k320", 0)]
i4 = C.c_int32 * 4


def pad4(v):
    return i4(*(list(v) + [0] * (4 - len(v))))


def unet_cfg(dtype, latent_repeat, text_len=77, **kw):
    c = dict(SD14_CONFIG, **kw)
    boc = c["block_out_channels"]
    return _lib.UnetConfig(in_channels=c["in_channels"], out_channels=c["out_channels"], sample_size=c["sample_size"], n_levels=len(boc),
                           block_out_channels=pad4(boc), level_has_attn=pad4([int("CrossAttn" in t) for t in c["down_block_types"]]),
                           layers_per_block=c["layers_per_block"], n_heads=c["attention_head_dim"], cross_dim=c["cross_attention_dim"],
                           text_len=text_len, norm_groups=c["norm_num_groups"], dtype=dtype, latent_repeat=latent_repeat)


def mmdit_cfg(dtype, text_len=333, **kw):
    c = dict(SD3_MEDIUM, **kw)
    return _lib.MmditConfig(in_channels=c["in_channels"], out_channels=c["out_channels"], sample_size=c["sample_size"],
                            patch_size=c["patch_size"], num_layers=c["num_layers"], num_heads=c["num_attention_heads"],
                            head_dim=c["attention_head_dim"], joint_dim=c["joint_attention_dim"], pooled_dim=c["pooled_projection_dim"],
                            text_len=text_len, time_dim=256, dtype=dtype)


def vae_cfg(dtype, **kw):
    c = dict(SD14_VAE_CONFIG, **kw)
    boc = c["block_out_channels"]
    return _lib.VaeConfig(latent_channels=c["latent_channels"], out_channels=c["out_channels"],
                          sample_size=c["sample_size"] >> (len(boc) - 1), n_levels=len(boc), block_out_channels=pad4(boc),
                          layers_per_block=c["layers_per_block"], norm_groups=c["norm_num_groups"], dtype=dtype)


def clip_fields(c, dtype):
    return dict(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                num_layers=c["num_hidden_layers"], num_heads=c["num_attention_heads"],
                max_position_embeddings=c["max_position_embeddings"], dtype=dtype)


def clip_cfg(dtype, **kw):
    return _lib.ClipConfig(**clip_fields(dict(SD14_CLIP_CONFIG, **kw), dtype))


def clip_proj_cfg(dtype, base, act, projection_dim, hidden_tap=2, **kw):
    return _lib.ClipProjConfig(projection_dim=projection_dim, act=ACT_CODES[act], eos_token_id=2, hidden_tap=hidden_tap,
                               **clip_fields(dict(base, **kw), dtype))


def t5_cfg(dtype, **kw):
    c = dict(T5_XXL_CONFIG, **kw)
    return _lib.T5Config(vocab_size=c["vocab_size"], d_model=c["d_model"], d_kv=c["d_kv"], d_ff=c["d_ff"], num_layers=c["num_layers"],
                         num_heads=c["num_heads"], num_buckets=c["relative_attention_num_buckets"],
                         max_distance=c["relative_attention_max_distance"], eps=c["layer_norm_epsilon"], dtype=dtype)


def clip_vision_cfg(dtype, base=VIT_L14_CONFIG, **kw):
    c = dict(base, **kw)
    return _lib.ClipVisionConfig(image_size=c["image_size"], patch_size=c["patch_size"], hidden_size=c["hidden_size"],
                                 intermediate_size=c["intermediate_size"], num_layers=c["num_hidden_layers"],
                                 num_heads=c["num_attention_heads"], projection_dim=c["projection_dim"], act=ACT_CODES[c["hidden_act"]],
                                 dtype=dtype)


SMALL_UNET = dict(block_out_channels=(64, 64), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), layers_per_block=1,
                  attention_head_dim=1, cross_attention_dim=64, sample_size=8, norm_num_groups=32)
SMALL_MMDIT = dict(sample_size=16, num_layers=3, num_attention_heads=4, joint_attention_dim=128, pooled_projection_dim=64)
SMALL_VAE = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=16)
SMALL_CLIP = dict(vocab_size=128, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2)
SMALL_T5 = dict(vocab_size=512, d_model=128, d_ff=256, num_layers=2, num_heads=2)
SMALL_VISION = dict(image_size=56, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, projection_dim=64)


def handles():
    """(label, create symbol, config factory taking the dtype, accepted dtypes, kind)"""
    out = []
    for rep in (0, 3):
        out.append((f"unet/sd14/rep{rep}", "sdn_unet_create", lambda d, r=rep: unet_cfg(d, r), range(4), "unet"))
    out.append(("unet/small", "sdn_unet_create", lambda d: unet_cfg(d, 0, text_len=5, **SMALL_UNET), range(4), "unet"))
    out.append(("mmdit/sd3-medium", "sdn_mmdit_create", lambda d: mmdit_cfg(d), range(4), "other"))
    out.append(("mmdit/small", "sdn_mmdit_create", lambda d: mmdit_cfg(d, text_len=45, **SMALL_MMDIT), range(4), "other"))
    for role in ("decoder", "encoder"):
        out.append((f"vae_{role}/sd14", f"sdn_vae_{role}_create", lambda d: vae_cfg(d), range(4), "other"))
        out.append((f"vae_{role}/small", f"sdn_vae_{role}_create", lambda d: vae_cfg(d, **SMALL_VAE), range(4), "other"))
    out.append(("clip/L", "sdn_clip_create", lambda d: clip_cfg(d), range(4), "other"))
    out.append(("clip/small", "sdn_clip_create", lambda d: clip_cfg(d, **SMALL_CLIP), range(4), "other"))
    out.append(("clip_proj/L", "sdn_clip_proj_create", lambda d: clip_proj_cfg(d, SD3_CLIP_L_CONFIG, "quick_gelu", 768), range(4), "other"))
    out.append(("clip_proj/bigG", "sdn_clip_proj_create", lambda d: clip_proj_cfg(d, SD3_CLIP_G_CONFIG, "gelu", 1280), range(4), "other"))
    out.append(("clip_proj/small", "sdn_clip_proj_create",
                lambda d: clip_proj_cfg(d, SD14_CLIP_CONFIG, "quick_gelu", 64, num_hidden_layers=3, **{k: v for k, v in SMALL_CLIP.items() if k != "num_hidden_layers"}),
                range(4), "other"))
    out.append(("t5/xxl", "sdn_t5_create", lambda d: t5_cfg(d), range(2), "t5"))
    out.append(("t5/small", "sdn_t5_create", lambda d: t5_cfg(d, **SMALL_T5), range(2), "t5"))
    out.append(("clip_vision/L14", "sdn_clip_vision_create", lambda d: clip_vision_cfg(d), range(2), "other"))
    out.append(("clip_vision/H14", "sdn_clip_vision_create", lambda d: clip_vision_cfg(d, VIT_H14_CONFIG), range(2), "other"))
    out.append(("clip_vision/small", "sdn_clip_vision_create", lambda d: clip_vision_cfg(d, **SMALL_VISION), range(2), "other"))
    for size in (299, 75):                                                      # pytorch-fid's side, and the smallest the creator accepts
        out.append((f"inception/{size}", "sdn_inception_create",
                    lambda d, s=size: _lib.InceptionConfig(image_size=s, normalize_input=1, dtype=d), (2,), "other"))
    return out


def manifest_hash(lib, h):
    sha, info = hashlib.sha256(), _lib.ParamInfo()
    for i in range(lib.sdn_unet_param_count(h)):
        assert lib.sdn_unet_param_info(h, i, C.byref(info)) == 0
        sha.update(repr((info.name, info.kind, info.rows, info.cols, info.rows_padded, info.offset)).encode())
    return sha.hexdigest()


def library():
    """libsdn with the argument types of the hooks include/sdn.h does not declare"""
    lib = _lib.lib()
    for name in {t[1] for t in UNET_TOGGLES if t[1]} - set(_lib.SIGNATURES):
        getattr(lib, name).restype, getattr(lib, name).argtypes = None, [C.c_void_p, C.c_longlong if "subbatch" in name else C.c_int]
    lib.sdn_debug_plan_digest.restype = C.c_int
    lib.sdn_debug_plan_digest.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    return lib


def cases():
    """(label, create symbol, config factory, dtype, kind, toggle label, setter, value), one per fingerprinted handle"""
    for label, create, cfg, dtypes, kind in handles():
        for dt in dtypes:
            for toggle, setter, value in (UNET_TOGGLES if kind == "unet" else UNET_TOGGLES[:1]):
                yield label, create, cfg, dt, kind, toggle, setter, value


def fingerprint_lines(lib, case):
    """The fingerprint of one case: a line per batch (and, for T5, per sequence length), from a fresh handle (creators set their own
    defaults)."""
    label, create, cfg, dt, kind, toggle, setter, value = case
    h, attn, ops = C.c_void_p(), C.c_double(), C.c_uint64()
    rc = getattr(lib, create)(C.byref(cfg(dt)), C.byref(h))
    assert rc == 0, (label, dt, rc)
    if setter:
        getattr(lib, setter)(h, value)
    lines = []
    for b in BATCHES:
        for n in (T5_LENGTHS if kind == "t5" else (0,)):
            if kind == "t5":
                ws, fl = lib.sdn_t5_workspace_bytes(h, b, n), lib.sdn_t5_flops(h, b, n, C.byref(attn))
            else:
                ws, fl = lib.sdn_unet_workspace_bytes(h, b), lib.sdn_unet_flops(h, b, C.byref(attn))
            assert lib.sdn_debug_plan_digest(h, b, n, C.byref(ops)) == 0
            lines.append(f"{label} dtype={dt} {toggle} B={b} n={n} params={lib.sdn_unet_param_count(h)} "
                         f"manifest={manifest_hash(lib, h)} weights={lib.sdn_unet_weight_bytes(h)} ws={ws} "
                         f"flops={fl!r} attn={attn.value!r} ops={ops.value:016x}")
    lib.sdn_unet_destroy(h)
    return lines


def case_key(case):
    return f"{case[0]} dtype={case[3]} {case[5]}"


def case_digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()
