"""Host side of SD-3.5-large on the engine (no GPU): the configuration's parameter count and key shapes, the checkpoint mapping with
and without `max_width`, sdn_mmdit_create_ex at the new width limit, the argument checks of the LayerNorm entry points above 2048
columns, max_samples(), and the power of the wide network test: the two deliberately wrong oracles of
tests_support/mmdit35_large_case.py lie outside the fp16 bound the engine is held to."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint, mmdit
from safe_denoiser_amd.mmdit import SD35_LARGE, SD3Transformer2DModel
from tests_support import mmdit35_large_case as case


def _block_formula(Cw, layers, qk_norm, joint=4096, pooled=2048, time_dim=256, patch_in=64, patch_out=64):
    """Parameters of an SD-v3 MMDiT without dual-attention blocks and without pos_embed.pos_embed, from the published block layout."""
    lin = lambda o, i: o * i + o
    top = lin(Cw, patch_in) + lin(Cw, time_dim) + lin(Cw, Cw) + lin(Cw, pooled) + lin(Cw, Cw) + lin(Cw, joint) + lin(2 * Cw, Cw) + lin(patch_out, Cw)
    stream = 4 * lin(Cw, Cw) + lin(4 * Cw, Cw) + lin(Cw, 4 * Cw)             # q, k, v, out; the feed-forward
    full = 2 * lin(6 * Cw, Cw) + 2 * stream
    last = lin(6 * Cw, Cw) + lin(2 * Cw, Cw) + stream + 3 * lin(Cw, Cw)      # context_pre_only: add_q / add_k / add_v only
    return top + (layers - 1) * full + last + (layers * 4 * 64 if qk_norm else 0)


def test_sd35_large_parameter_count_and_key_families():
    assert SD35_LARGE == dict(mmdit.SD3_MEDIUM, num_layers=38, num_attention_heads=38, qk_norm="rms_norm")
    assert SD35_LARGE["pos_embed_max_size"] == 192 and "dual_attention_layers" not in SD35_LARGE and mmdit.MAX_WIDTH == 2560
    assert _block_formula(1536, 24, False) == 2_028_328_000                 # the formula reproduces SD3-medium's pinned count
    assert _block_formula(2432, 38, True) == 8_056_627_520
    shapes = SD3Transformer2DModel(**SD35_LARGE).state_dict_shapes()
    count = sum(torch.Size(s).numel() for k, s in shapes.items() if k != "pos_embed.pos_embed")
    assert count == 8_056_627_520
    Cw = 2432
    assert shapes["pos_embed.pos_embed"] == (1, 192 * 192, Cw) and shapes["pos_embed.proj.weight"] == (Cw, 16, 2, 2)
    assert shapes["context_embedder.weight"] == (Cw, 4096) and shapes["norm_out.linear.weight"] == (2 * Cw, Cw)
    assert shapes["proj_out.weight"] == (64, Cw)
    for i in range(38):
        pfx = f"transformer_blocks.{i}."
        last = i == 37
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            assert shapes[pfx + f"attn.{n}.weight"] == (64,)
        assert shapes[pfx + "norm1.linear.weight"] == (6 * Cw, Cw)
        assert shapes[pfx + "norm1_context.linear.weight"] == ((2 if last else 6) * Cw, Cw)
        for n in ("to_q", "to_k", "to_v", "to_out.0", "add_q_proj", "add_k_proj", "add_v_proj"):
            assert shapes[pfx + f"attn.{n}.weight"] == (Cw, Cw) and shapes[pfx + f"attn.{n}.bias"] == (Cw,)
        assert shapes[pfx + "ff.net.0.proj.weight"] == (4 * Cw, Cw) and shapes[pfx + "ff.net.2.weight"] == (Cw, 4 * Cw)
        assert (pfx + "attn.to_add_out.weight" in shapes) == (not last) and (pfx + "ff_context.net.2.weight" in shapes) == (not last)
    assert not any("attn2" in k for k in shapes)


def test_mmdit_kwargs_takes_the_large_config_only_with_max_width():
    kw = checkpoint.mmdit_kwargs(case.SD35_LARGE_JSON, sd35=True, max_width=2560)
    assert kw == dict(in_channels=16, out_channels=16, sample_size=128, patch_size=2, num_layers=38, num_attention_heads=38,
                      attention_head_dim=64, joint_attention_dim=4096, pooled_projection_dim=2048, pos_embed_max_size=192,
                      qk_norm="rms_norm", dual_attention_layers=())
    assert dict(SD35_LARGE, sample_size=128, dual_attention_layers=()) == dict(mmdit.SD3_MEDIUM, **kw)
    assert checkpoint.mmdit_kwargs(case.SD35_LARGE_JSON, sd35=True, max_width=mmdit.MAX_WIDTH) == kw
    with pytest.raises(NotImplementedError, match="2432"):                    # the default limit stays 2048
        checkpoint.mmdit_kwargs(case.SD35_LARGE_JSON, sd35=True)
    for heads in (42, 35):                                                     # 2688: above the limit; 2240: not a multiple of 128
        with pytest.raises(NotImplementedError, match=str(64 * heads)):
            checkpoint.mmdit_kwargs(dict(case.SD35_LARGE_JSON, num_attention_heads=heads, caption_projection_dim=64 * heads), sd35=True,
                                    max_width=2560)
    # widths the 2048 limit admitted are untouched by the 128 rule (SD3-medium's 1536, and 1984 = 31 x 64)
    for heads in (24, 31):
        j = dict(case.SD35_LARGE_JSON, num_attention_heads=heads, caption_projection_dim=64 * heads)
        assert checkpoint.mmdit_kwargs(j, sd35=True)["num_attention_heads"] == heads


def _cfg(heads, layers=2):
    return _lib.MmditConfig(in_channels=16, out_channels=16, sample_size=8, patch_size=2, num_layers=layers, num_heads=heads,
                            head_dim=64, joint_dim=128, pooled_dim=64, text_len=13, time_dim=256, dtype=1)


def test_create_ex_width_limit():
    lib = sda.lib()
    ext = _lib.MmditExt(qk_norm=1, qk_norm_eps=1e-6)
    for heads, rc in ((38, 0), (40, 0), (34, 0), (42, -1), (44, -1)):          # 2432, 2560, 2176 / 2688, 2816
        for dt in (0, 1, 2, 3):
            cfg, h = _cfg(heads), C.c_void_p()
            cfg.dtype = dt
            assert lib.sdn_mmdit_create_ex(C.byref(cfg), C.byref(ext), C.byref(h)) == rc, (heads, dt)
            assert bool(h.value) == (rc == 0)
            if h.value:
                assert lib.sdn_unet_param_count(h) > 0
                lib.sdn_unet_destroy(h)
    cfg, h = _cfg(38), C.c_void_p()                                            # the plain entry point shares the limit
    assert lib.sdn_mmdit_create(C.byref(cfg), C.byref(h)) == 0
    lib.sdn_unet_destroy(h)


def test_layernorm_entry_points_above_2048_columns():
    """rows = 0 on aligned host memory: the argument checks run, nothing is launched or dereferenced.  Above 2048 columns only the
    multiples of 128 up to 2560 are taken; at and below 2048 every multiple of 8 (4 for the f32 adaLN) as before."""
    lib = sda.lib()
    raw = C.create_string_buffer(256)
    p = (C.addressof(raw) + 15) & ~15
    entries = {
        "layernorm_bf16": lambda c: lib.sdn_layernorm_bf16(p, 0, c, 1e-6, p, p, p, None),
        "layernorm_f16": lambda c: lib.sdn_layernorm_f16(p, 0, c, 1e-6, p, p, p, None),
        "layernorm_mod_bf16": lambda c: lib.sdn_layernorm_mod_bf16(p, 0, c, 1e-6, p, p, 3 * c, 4, p, None),
        "layernorm_mod_f16": lambda c: lib.sdn_layernorm_mod_f16(p, 0, c, 1e-6, p, p, 3 * c, 4, p, None),
        "row_stats_bf16": lambda c: lib.sdn_row_stats_bf16(p, 0, c, 1e-6, p, None),
        "row_stats_f16": lambda c: lib.sdn_row_stats_f16(p, 0, c, 1e-6, p, None),
        "layernorm_mod_f32": lambda c: lib.sdn_layernorm_mod_f32(p, 0, c, 1e-6, p, p, 3 * c, 4, p, None),
    }
    for name, call in entries.items():
        for c in (2176, 2432, 2560, 2048, 2040, 1536):
            assert call(c) == 0, (name, c)
        for c in (2056, 2688, 2440, 2052, 2564, 4096):
            assert call(c) == -1, (name, c)


def test_max_samples_follows_the_feed_forward_operand():
    for side, prec, want in ((64, None, 107), (128, None, 26), (64, "fp32", 53), (128, "bf16x3", 13)):
        m = SD3Transformer2DModel(precision=prec, **dict(SD35_LARGE, sample_size=side)) if prec else SD3Transformer2DModel(**dict(SD35_LARGE, sample_size=side))
        tokens, esz = (side // 2) ** 2, 4 if prec else 2
        assert m.max_samples() == ((1 << 31) - 1) // (tokens * 4 * 2432 * esz) == want
        assert m.max_samples() * tokens * 4 * 2432 * esz < 1 << 31 <= (m.max_samples() + 1) * tokens * 4 * 2432 * esz


def test_wide_oracle_margins():
    """The emulating oracles of the wide network sit inside the bounds the engine is held to, and the two wrong networks -- LayerNorm
    over columns 0..2047 only, attention over heads 0..31 only -- at least 5x outside the fp16 bound.
    Measured: fp16-emulating 6.4e-4, bf16-emulating 5.2e-3 from fp32 (small SD-3.5 network: 8.2e-4, so s = 1); ln2048 4.0e-1,
    heads32 4.8e-2."""
    r32 = case.reference(None)
    d_wide, d_small, s = case.scale()
    b = case.bounds()
    a16, ab = case.rel_l2(case.reference(torch.float16), r32), case.rel_l2(case.reference(torch.bfloat16), r32)
    wrong = {k: case.rel_l2(case.reference(None, k), r32) for k in ("ln2048", "heads32")}
    print(f"wide sd35 oracle: fp16-emulating {a16:.2e}, bf16-emulating {ab:.2e} from fp32; d_wide {d_wide:.3e}, d_small {d_small:.3e}, s {s:.3f}; "
          f"wrong networks {wrong}; bounds {b}")
    assert a16 == d_wide and 1.0 <= s < 1.5
    assert a16 <= b["fp16"] and ab <= b["bf16"]
    assert wrong["ln2048"] >= 5 * b["fp16"] and wrong["heads32"] >= 5 * b["fp16"]

