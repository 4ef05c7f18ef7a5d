"""Host-side checks of the SD-v3 MMDiT precision plans (sdn_mmdit_config.dtype 2 = fp32, 3 = bf16x3): the plan's manifest, weight
layout, FLOPs and batch limit, the dtype / precision validation, the argument checks of the new f32 operators (no GPU is touched)
and the SD-v3 pipeline's precision-schedule arguments."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from safe_denoiser_amd.mmdit import P_POS_CROP, SD3Transformer2DModel
from safe_denoiser_amd.unet import P_VEC_F32

PRECISE = ("fp32", "bf16x3")
SMALL = dict(sample_size=16, num_layers=3, num_attention_heads=4, joint_attention_dim=128, pooled_projection_dim=64,
             pos_embed_max_size=24)


def _all_params(m):
    """Every region of the plan's weight buffer, in manifest order (the MMDiT plan has no engine-derived regions)."""
    info, out = _lib.ParamInfo(), []
    for i in range(sda.lib().sdn_unet_param_count(m._h)):
        _lib.check(sda.lib().sdn_unet_param_info(m._h, i, C.byref(info)), "sdn_unet_param_info")
        out.append((info.name.decode(), info.kind, info.rows, info.cols, info.rows_padded, info.offset))
    return out


@pytest.fixture(scope="module")
def fp16_plan():
    return SD3Transformer2DModel(sample_size=64)


@pytest.mark.parametrize("precision", PRECISE)
def test_precise_plan_has_the_fp16_manifest_and_an_f32_layout(fp16_plan, precision):
    m = SD3Transformer2DModel(sample_size=64, precision=precision)
    assert m.dtype == torch.float32 and m.precision == precision
    ref = _all_params(fp16_plan)
    got = _all_params(m)
    assert [p[:5] for p in got] == [p[:5] for p in ref]
    assert m.state_dict_shapes() == fp16_plan.state_dict_shapes()
    # f32 layout: 4 B per element for every kind, each region 256-byte aligned, in manifest order
    off = 0
    for name, kind, rows, cols, rows_padded, offset in got:
        assert offset == off, name
        off += (rows_padded * max(cols, 1) * 4 + 255) // 256 * 256
    assert m.weight_bytes == off
    # ... and the 16-bit plan's rule, for comparison: 2 B per matrix / position-embedding element
    off = 0
    for name, kind, rows, cols, rows_padded, offset in ref:
        assert offset == off, name
        off += (rows_padded * max(cols, 1) * (4 if kind == P_VEC_F32 else 2) + 255) // 256 * 256
    assert fp16_plan.weight_bytes == off
    assert any(p[1] == P_POS_CROP for p in got)
    assert m.flops(1) == fp16_plan.flops(1) and m.flops(3) == fp16_plan.flops(3)


def test_precise_plan_packs_every_kind_in_f32():
    m = SD3Transformer2DModel(text_len=45, precision="bf16x3", **SMALL)
    sd = m.synthetic_state_dict(5)
    buf = m.pack_state_dict(sd)
    assert buf.numel() == m.weight_bytes
    for p in m.manifest:
        t = sd[p["name"]].float()
        if p["kind"] == P_POS_CROP:
            t = m.crop_pos_embed(t)
        n = t.numel()
        got = buf[p["offset"]:p["offset"] + 4 * n].view(torch.float32)
        assert torch.equal(got, t.reshape(-1)), p["name"]


def test_invalid_dtype_and_precision_are_rejected():
    c = _lib.MmditConfig(in_channels=16, out_channels=16, sample_size=16, patch_size=2, num_layers=3, num_heads=4, head_dim=64,
                         joint_dim=128, pooled_dim=64, text_len=45, time_dim=256, dtype=4)
    h = C.c_void_p()
    assert sda.lib().sdn_mmdit_create(C.byref(c), C.byref(h)) == -1
    c.dtype = -1
    assert sda.lib().sdn_mmdit_create(C.byref(c), C.byref(h)) == -1
    for dt in (2, 3):
        c.dtype = dt
        assert sda.lib().sdn_mmdit_create(C.byref(c), C.byref(h)) == 0
        sda.lib().sdn_unet_destroy(h)
    with pytest.raises(_lib.SdnError):
        SD3Transformer2DModel(text_len=45, precision="fp64", **SMALL)
    with pytest.raises(_lib.SdnError):
        SD3Transformer2DModel(text_len=45, dtype=torch.float64, **SMALL)
    assert SD3Transformer2DModel(text_len=45, dtype=torch.float32, **SMALL).precision == "fp32"
    assert SD3Transformer2DModel(text_len=45, dtype=torch.float16, precision="bf16x3", **SMALL).dtype == torch.float32


def test_new_f32_operators_reject_bad_arguments_on_host():
    lib = sda.lib()
    A = 0x10000                                                          # 16-byte aligned stand-ins; nothing is dereferenced
    B, Hh, n1, n = 2, 4, 64, 109
    ld = 3 * Hh * 64
    s2 = _lib.AttnSegment2(A + 0x1000, A + 0x2000, A + 0x3000, A + 0x4000, n1, ld, ld, ld, Hh * 64)

    def ja(mode=0, q=A, seg=C.byref(s2), head_dim=64, ldq=ld, n_total=n):
        return lib.sdn_joint_attention_f32(mode, q, A + 0x100, A + 0x200, A + 0x300, seg, B, Hh, n_total, head_dim, ldq, ld, ld,
                                           Hh * 64, 0.125, None)
    assert ja(seg=None) == -1                                            # null segment
    assert ja(head_dim=80) == -1                                         # head_dim != 64
    assert ja(q=A + 4) == -1 and ja(mode=1, q=A + 4) == -1               # misaligned q
    assert ja(ldq=ld + 2) == -1                                          # leading dimension not a multiple of 4 floats
    assert ja(mode=2) == -1 and ja(mode=-1) == -1
    assert ja(n_total=n1) == -1                                          # empty second stream
    for bad in ("q2", "k2", "v2"):
        t = _lib.AttnSegment2(A + 0x1000, A + 0x2000, A + 0x3000, A + 0x4000, n1, ld, ld, ld, Hh * 64)
        setattr(t, bad, getattr(t, bad) + 8)                             # misaligned second-stream operand
        assert ja(seg=C.byref(t)) == -1
    t = _lib.AttnSegment2(A + 0x1000, None, A + 0x3000, A + 0x4000, n1, ld, ld, ld, Hh * 64)
    assert ja(seg=C.byref(t)) == -1
    assert lib.sdn_joint_attention_f32(0, A, A, A, A, C.byref(s2), 0, Hh, n, 64, ld, ld, ld, Hh * 64, 0.125, None) == 0  # empty batch

    def lm(x=A, rows=10, c=1536, scale=A + 0x100, shift=A + 0x200, ld_mod=3 * 1536, rpb=5, out=A + 0x300):
        return lib.sdn_layernorm_mod_f32(x, rows, c, 1e-6, scale, shift, ld_mod, rpb, out, None)
    assert lm(x=None) == -1 and lm(scale=None) == -1 and lm(out=None) == -1
    assert lm(x=A + 4) == -1 and lm(scale=A + 0x104) == -1 and lm(out=A + 8) == -1   # misaligned
    assert lm(c=1538) == -1 and lm(c=4096) == -1                          # c % 4, c > 2048
    assert lm(rpb=0) == -1 and lm(ld_mod=1535) == -1 and lm(ld_mod=3 * 1536 + 2) == -1
    assert lm(rows=0) == 0
    assert lib.sdn_patchify_f32(A, 2, 16, 9, 8, 2, A + 0x1000, None) == -1                  # H % p
    assert lib.sdn_patchify_f32(None, 2, 16, 8, 8, 2, A + 0x1000, None) == -1
    assert lib.sdn_patchify_f32(A, 0, 16, 8, 8, 2, A + 0x1000, None) == 0


def test_precise_plans_batch_limit():
    """fp32 storage doubles the widest operand (the feed-forward hidden state): the 16-bit plan's 2 GiB rule at 4 B per element."""
    for precision in PRECISE:
        assert SD3Transformer2DModel(sample_size=64, precision=precision).max_samples() == 85
        assert SD3Transformer2DModel(sample_size=128, precision=precision).max_samples() == 21
    assert SD3Transformer2DModel(sample_size=64).max_samples() == 170 and SD3Transformer2DModel(sample_size=128).max_samples() == 42


def test_sd3_pipeline_precision_schedule_arguments():
    from safe_denoiser_amd.pipeline import SafeDenoiserPipeline
    from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
    lo_net = SD3Transformer2DModel(text_len=45, **SMALL)
    hi_net = SD3Transformer2DModel(text_len=45, precision="bf16x3", **SMALL)
    sch = FlowMatchEulerDiscreteScheduler()
    with pytest.raises(_lib.SdnError):
        SD3SafeDenoiserPipeline(lo_net, sch, transformer_hi=hi_net)                        # both or neither
    with pytest.raises(_lib.SdnError):
        SD3SafeDenoiserPipeline(lo_net, sch, precision_schedule="all")
    with pytest.raises(_lib.SdnError):
        SD3SafeDenoiserPipeline(lo_net, sch, transformer_hi=SD3Transformer2DModel(text_len=44, precision="bf16x3", **SMALL),
                                precision_schedule="all")
    with pytest.raises(_lib.SdnError):
        SD3SafeDenoiserPipeline(lo_net, sch, transformer_hi=SD3Transformer2DModel(text_len=45, precision="bf16x3",
                                                                                 **dict(SMALL, num_layers=2)), precision_schedule="all")
    pipe = SD3SafeDenoiserPipeline(lo_net, sch, transformer_hi=hi_net, precision_schedule={"window": True})
    assert pipe.transformer_hi is hi_net
    ts = [1000.0, 900.0, 780.0, 779.0, 500.0]
    assert pipe.hi_steps(ts, "t", 780, 1000) == [True, True, True, False, False]
    assert pipe.hi_steps(ts, "no window", 780, 1000) == [False] * 5        # no processor: no window steps
    for ps in ("all", "none", {"first": 2, "last": 1}, [True, False, True, False, False], lambda i, t, w: i == 3):
        pipe.precision_schedule = ps
        ref = SafeDenoiserPipeline.__new__(SafeDenoiserPipeline)
        ref.precision_schedule = ps
        assert pipe.hi_steps(ts, "t", 780, 1000) == ref.hi_steps(ts, "t", 780, 1000)
