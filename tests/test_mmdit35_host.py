"""Host side of the SD-3.5 MMDiT (no GPU): the parameter count that pins the wiring of the two additions (q/k RMS norm, dual-attention
blocks), sdn_mmdit_create_ex against sdn_mmdit_create, the checkpoint mapping, sdn_qk_rmsnorm's argument checks, and the self-checks
of tests_support/mmdit35_oracle.py that make the GPU comparison mean something: the deliberately wrong networks (norms skipped,
attn2 skipped, one gain vector replaced by ones) lie far outside the bounds the engine is held to."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint
from safe_denoiser_amd.mmdit import SD35_MEDIUM, SD3Transformer2DModel
from tests_support import mmdit35_case as case
from tests_support import plan_cases

# transformer/config.json of stabilityai/stable-diffusion-3.5-medium, as published
SD35_MEDIUM_JSON = {"_class_name": "SD3Transformer2DModel", "_diffusers_version": "0.31.0.dev0", "attention_head_dim": 64,
                    "caption_projection_dim": 1536, "dual_attention_layers": list(range(13)), "in_channels": 16,
                    "joint_attention_dim": 4096, "num_attention_heads": 24, "num_layers": 24, "out_channels": 16, "patch_size": 2,
                    "pooled_projection_dim": 2048, "pos_embed_max_size": 384, "qk_norm": "rms_norm", "sample_size": 128}


def test_sd35_medium_parameter_count_and_key_families():
    shapes = SD3Transformer2DModel(**dict(SD35_MEDIUM, sample_size=64)).state_dict_shapes()
    count = lambda sh: sum(torch.Size(s).numel() for k, s in sh.items() if k != "pos_embed.pos_embed")
    assert count(shapes) == 2_243_171_520
    # = SD3-medium's count + 24 blocks x 4 gains of 64 + 13 dual blocks x (3 more adaLN chunks + attn2's four linears + its 2 gains)
    Cw = 1536
    assert count(shapes) == 2_028_328_000 + 24 * 256 + 13 * (3 * Cw * Cw + 3 * Cw + 4 * (Cw * Cw + Cw) + 128)
    assert shapes["pos_embed.pos_embed"] == (1, 384 * 384, Cw)
    for i in range(24):
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):            # the last block's norm_added_q too
            assert shapes[f"transformer_blocks.{i}.attn.{n}.weight"] == (64,)
        dual = i < 13
        assert shapes[f"transformer_blocks.{i}.norm1.linear.weight"] == ((9 if dual else 6) * Cw, Cw)
        assert shapes[f"transformer_blocks.{i}.norm1.linear.bias"] == ((9 if dual else 6) * Cw,)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            assert (f"transformer_blocks.{i}.attn2.{n}.weight" in shapes) == dual
            if dual:
                assert shapes[f"transformer_blocks.{i}.attn2.{n}.weight"] == (Cw, Cw)
                assert shapes[f"transformer_blocks.{i}.attn2.{n}.bias"] == (Cw,)
        for n in ("norm_q", "norm_k"):
            assert (f"transformer_blocks.{i}.attn2.{n}.weight" in shapes) == dual
    assert not any("attn2" in k and ("add_" in k or "norm_added" in k) for k in shapes)


def test_constructor_keeps_the_additions_in_config_and_refuses_other_norms():
    m = case.model()
    assert m.config.qk_norm == "rms_norm" and m.config.dual_attention_layers == (0, 2)
    plain = SD3Transformer2DModel(text_len=45, **case.SMALL)
    assert plain.config.qk_norm is None and plain.config.dual_attention_layers == ()
    with pytest.raises(NotImplementedError, match="layer_norm"):
        SD3Transformer2DModel(text_len=45, qk_norm="layer_norm", **case.SMALL)
    with pytest.raises(_lib.SdnError):
        SD3Transformer2DModel(text_len=45, dual_attention_layers=(3,), **case.SMALL)
    # every existing configuration's synthetic draws are untouched; the new gains are U(1, 3)
    sd = case.state_dict()
    gains = [v for k, v in sd.items() if "norm_q" in k or "norm_k" in k or "norm_added" in k]
    assert len(gains) == 3 * 4 + 2 * 2 and all(v.shape == (64,) and 1.0 <= float(v.min()) and float(v.max()) <= 3.0 for v in gains)
    assert max(float(v.max()) for v in gains) > 2.5 and min(float(v.min()) for v in gains) < 1.5


def _cfg(num_layers=3):
    return _lib.MmditConfig(in_channels=16, out_channels=16, sample_size=16, patch_size=2, num_layers=num_layers, num_heads=4,
                            head_dim=64, joint_dim=128, pooled_dim=64, text_len=45, time_dim=256, dtype=1)


def _fingerprint(lib, h):
    out = [lib.sdn_unet_param_count(h), plan_cases.manifest_hash(lib, h), lib.sdn_unet_weight_bytes(h)]
    for b in (1, 2):
        ops = C.c_uint64()
        assert lib.sdn_debug_plan_digest(h, b, 0, C.byref(ops)) == 0
        out += [lib.sdn_unet_workspace_bytes(h, b), ops.value]
    return out


def test_create_ex_without_additions_is_create():
    lib = plan_cases.library()
    cfg, handles = _cfg(), []
    for make in (lambda h: lib.sdn_mmdit_create(C.byref(cfg), C.byref(h)),
                 lambda h: lib.sdn_mmdit_create_ex(C.byref(cfg), None, C.byref(h)),
                 lambda h: lib.sdn_mmdit_create_ex(C.byref(cfg), C.byref(_lib.MmditExt()), C.byref(h))):
        h = C.c_void_p()
        assert make(h) == 0
        handles.append(h)
    ext = _lib.MmditExt(qk_norm=1, qk_norm_eps=1e-6, dual_attention_mask=0b101)
    h = C.c_void_p()
    assert lib.sdn_mmdit_create_ex(C.byref(cfg), C.byref(ext), C.byref(h)) == 0
    handles.append(h)
    try:
        prints = [_fingerprint(lib, h) for h in handles]
        assert prints[1] == prints[0] and prints[2] == prints[0]
        assert prints[3][4] != prints[0][4] and prints[3][0] > prints[0][0]           # the additions do change the plan
    finally:
        for h in handles:
            lib.sdn_unet_destroy(h)


@pytest.mark.parametrize("layers,ext", [(3, dict(qk_norm=2)), (3, dict(dual_attention_mask=1 << 3)), (3, dict(dual_attention_mask=1 << 63)),
                                        (65, dict(dual_attention_mask=1)), (3, dict(qk_norm=-1))])
def test_create_ex_refuses(layers, ext):
    lib = sda.lib()
    cfg, h = _cfg(layers), C.c_void_p()
    assert lib.sdn_mmdit_create_ex(C.byref(cfg), C.byref(_lib.MmditExt(qk_norm_eps=1e-6, **ext)), C.byref(h)) == -1
    assert not h.value
    if layers == 65:                                                             # the layer count itself is fine without a mask
        assert lib.sdn_mmdit_create_ex(C.byref(cfg), C.byref(_lib.MmditExt(qk_norm=1, qk_norm_eps=1e-6)), C.byref(h)) == 0
        lib.sdn_unet_destroy(h)


def test_mmdit_kwargs_with_the_sd35_flag():
    kw = checkpoint.mmdit_kwargs(SD35_MEDIUM_JSON, sd35=True)
    assert kw == dict(in_channels=16, out_channels=16, sample_size=128, patch_size=2, num_layers=24, num_attention_heads=24,
                      attention_head_dim=64, joint_attention_dim=4096, pooled_projection_dim=2048, pos_embed_max_size=384,
                      qk_norm="rms_norm", dual_attention_layers=tuple(range(13)))
    assert dict(SD35_MEDIUM, sample_size=128) == dict(sda.mmdit.SD3_MEDIUM, **kw)
    sd3 = {k: v for k, v in SD35_MEDIUM_JSON.items() if k not in ("qk_norm", "dual_attention_layers")}
    assert checkpoint.mmdit_kwargs(sd3, sd35=True) == dict(checkpoint.mmdit_kwargs(sd3), qk_norm=None, dual_attention_layers=())
    for key, value in (("qk_norm", "layer_norm"), ("caption_projection_dim", 1024), ("dual_attention_layers", [24]),
                       ("_class_name", "FluxTransformer2DModel")):
        with pytest.raises(NotImplementedError, match=key if key != "_class_name" else "FluxTransformer2DModel"):
            checkpoint.mmdit_kwargs(dict(SD35_MEDIUM_JSON, **{key: value}), sd35=True)
    with pytest.raises(NotImplementedError, match="2432"):                       # SD-3.5-large: 38 heads x 64
        checkpoint.mmdit_kwargs(dict(SD35_MEDIUM_JSON, num_attention_heads=38, caption_projection_dim=2432), sd35=True)
    for key, value in (("qk_norm", "rms_norm"), ("dual_attention_layers", [0])):   # without the flag: as before
        with pytest.raises(NotImplementedError, match=key):
            checkpoint.mmdit_kwargs({**SD35_MEDIUM_JSON, "qk_norm": None, "dual_attention_layers": [], key: value})


def test_qk_rmsnorm_argument_checks():
    lib = sda.lib()
    raw = C.create_string_buffer(4096 + 16)
    base = (C.addressof(raw) + 15) & ~15                       # 16-byte aligned host memory; nothing is dereferenced
    X, WQ, WK = base, base + 2048, base + 2048 + 256
    ok = dict(dtype=1, qkv=X, rows=4, heads=4, ld=768, wq=WQ, wk=WK, eps=1e-6)
    call = lambda **kw: lib.sdn_qk_rmsnorm(*[dict(ok, **kw)[k] for k in ("dtype", "qkv", "rows", "heads", "ld", "wq", "wk", "eps")], None)
    for bad in (dict(qkv=None), dict(wq=None), dict(wk=None), dict(heads=0), dict(heads=-1), dict(ld=767), dict(ld=760),
                dict(ld=772), dict(dtype=2, ld=770), dict(qkv=X + 8), dict(eps=0.0), dict(eps=-1e-6), dict(dtype=3), dict(dtype=-1),
                dict(rows=-1)):
        assert call(**bad) == -1, bad
    for dt in (0, 1, 2):
        assert call(dtype=dt, rows=0) == 0
    assert call(dtype=2, ld=772, rows=0) == 0 and call(ld=776, rows=0) == 0      # 4-element (f32) and 8-element (16-bit) strides


# ---- oracle self-checks ----------------------------------------------------------------------------------------------------------
def test_oracle_reduces_to_the_sd3_oracle_without_the_additions():
    from oracle.mmdit import OracleMMDiT
    from tests_support.mmdit35_oracle import OracleMMDiT35
    sd = SD3Transformer2DModel(text_len=45, **case.SMALL).synthetic_state_dict(5)
    x, e, pl = case.inputs()
    for dt in (None, torch.float16):
        assert torch.equal(OracleMMDiT35(sd, case.SMALL_O, act_dtype=dt)(x, 812.0, e, pl), OracleMMDiT(sd, case.SMALL_O, act_dtype=dt)(x, 812.0, e, pl))


def test_oracle_margins():
    """(a), (b): the emulating oracles sit inside the bounds the engine is held to; (c), (d), (e): a network without the q/k norms,
    without attn2, or with one live gain vector replaced by ones is at least 10x / 10x / 5x the fp16 bound away; the last block's
    norm_added_q is dead (its text output is discarded), so only the kernel test covers that gain.
    Measured: (a) 8.2e-4, (b) 6.6e-3, (c) 1.7e-1, (d) 1.3e-1, (e) 5.2e-2 / 7.3e-2 / 5.0e-2 (mmdit35_case.LIVE_GAINS)."""
    r32 = case.reference(None)
    a, b = case.rel_l2(case.reference(torch.float16), r32), case.rel_l2(case.reference(torch.bfloat16), r32)
    wrong = {k: case.rel_l2(v, r32) for k, v in case.wrong_references().items()}
    print(f"sd35 small oracle: fp16-emulating {a:.2e}, bf16-emulating {b:.2e} from fp32; wrong networks {wrong}")
    assert a <= 5e-3 and b <= 4e-2
    assert wrong["no_qk_norm"] >= 5e-2 and wrong["no_attn2"] >= 5e-2
    assert len(wrong) == 5 and all(v >= 2.5e-2 for k, v in wrong.items() if k.startswith("ones:"))
    assert torch.equal(case.oracle_out(case.with_ones(case.DEAD_GAIN)), r32)
