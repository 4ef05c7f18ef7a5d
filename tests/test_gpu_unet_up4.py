"""The UNet plan with its qualifying upsampler convs in phase form (sdn_unet_set_conv_up4, on by default).

A two-level network with sample_size 32: its one upsampler goes 16^2 -> 32^2 (a stored map of 256 pixels, Cin = N = 640), so it
qualifies; the 8^2 -> 16^2 upsampler of tests/test_gpu_unet.py's small configuration does not."""
import ctypes as C

import pytest
import torch

import safe_denoiser_amd as sda
from oracle.unet import OracleUNet
from safe_denoiser_amd.unet import UNet2DConditionModel

pytestmark = pytest.mark.gpu

CFG = dict(block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
           layers_per_block=1, attention_head_dim=8, cross_attention_dim=768, sample_size=32)
CFG_O = dict(block_out_channels=(320, 640), level_has_attn=(True, False), layers_per_block=1, n_heads=8,
             cross_dim=768, sample_size=32)
SMALL16 = dict(CFG, sample_size=16)
BOUND = 2.5e-2               # tests/test_gpu_unet.py: its small configuration against the bf16-emulating and the fp32 oracle


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _regions(u):
    """Every region of the handle's weight buffer, derived ones included: (name, kind, offset, padded bytes)."""
    from safe_denoiser_amd import _lib
    info, out = _lib.ParamInfo(), []
    for i in range(sda.lib().sdn_unet_param_count(u._h)):
        _lib.check(sda.lib().sdn_unet_param_info(u._h, i, C.byref(info)), "sdn_unet_param_info")
        esz = 4 if info.kind in (0, 4) else 2
        nbytes = info.rows if info.kind == 6 else info.rows_padded * max(info.cols, 1) * esz
        out.append((info.name.decode(), info.kind, info.offset, (nbytes + 255) // 256 * 256))
    return out


def _kernels(u, x, e):
    u.profile_next()
    u(x, 781.0, encoder_hidden_states=e)
    return {r["kernel"]: r["launches"] for r in u.profile_read()}


@pytest.fixture(scope="module")
def net():
    u = UNet2DConditionModel(text_len=77, **CFG)
    sd = u.synthetic_state_dict(7)
    u.load_state_dict(sd)
    return u, sd


def test_phase_form_runs_keeps_batch_rows_bit_equal_and_meets_the_oracle_bound(net):
    u, sd = net
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, 32, 32, generator=g).cuda()
    e = torch.randn(3, 77, 768, generator=g).cuda()
    assert _kernels(u, x, e).get("k_conv_up4<10>") == 1
    y_on = u(x, 781.0, encoder_hidden_states=e).sample
    for i in range(3):                                               # a sample has the same bits at B = 1 and B = 3
        y1 = u(x[i:i + 1].contiguous(), 781.0, encoder_hidden_states=e[i:i + 1].contiguous()).sample
        torch.testing.assert_close(y1, y_on[i:i + 1], rtol=0, atol=0)
    f_on, w_on = u.flops(3), _regions(u)
    u.set_conv_up4(False)
    try:
        ks = _kernels(u, x, e)
        assert not any(k.startswith("k_conv_up4") for k in ks), ks
        y_off = u(x, 781.0, encoder_hidden_states=e).sample
        assert u.flops(3) == f_on                                    # the algorithmic (nine-tap) count either way
        assert _regions(u) == w_on and sda.lib().sdn_unet_weight_bytes(u._h) == u.weight_bytes   # the manifest does not change
    finally:
        u.set_conv_up4(True)
    torch.testing.assert_close(u(x, 781.0, encoder_hidden_states=e).sample, y_on, rtol=0, atol=0)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    ref_bf = OracleUNet(sd, CFG_O, act_dtype=torch.bfloat16, device="cuda")(x, 781.0, e)
    ref_32 = OracleUNet(sd, CFG_O, act_dtype=None, device="cuda")(x, 781.0, e)
    for name, y in (("phase form", y_on), ("nine-tap", y_off)):
        r1, r2 = rel_l2(y, ref_bf), rel_l2(y, ref_32)
        print(f"two-level unet, sample_size 32, {name}: rel L2 vs bf16-emulating oracle {r1:.3e}, vs fp32 oracle {r2:.3e}")
        assert r1 <= BOUND and r2 <= BOUND
    print(f"phase form vs nine-tap: rel L2 {rel_l2(y_on, y_off):.3e}")


def test_derived_regions_are_the_last_manifest_entries_whatever_the_switch(net):
    """The manifest is fixed at creation and does not depend on the switch (the first test asserts it is identical on and off): a
    weight buffer packed once serves both plans.  Against the nine-tap-only layout it grows by the derived regions alone: the phase
    weights are the LAST regions of the manifest (16 N Cin elements per qualifying upsampler), behind every region the nine-tap plan
    has, so no other offset moves.  A configuration whose upsampler does not qualify registers none."""
    u, _ = net
    regs = _regions(u)
    up4 = [r for r in regs if r[0].startswith("up4@")]
    assert len(up4) == 1 and regs[-1] == up4[0] and up4[0][1] == 6 and up4[0][3] == 16 * 640 * 640 * 2
    conv_w = [r for r in regs if r[0] == "up_blocks.0.upsamplers.0.conv.weight"]
    assert up4[0][0] == f"up4@{conv_w[0][2]}"                       # named after the nine-tap matrix it is derived from
    off = 0
    for name, kind, offset, nbytes in regs:                          # contiguous: the buffer is exactly its regions
        assert offset == off, name
        off += nbytes
    assert off == u.weight_bytes and up4[0][2] + up4[0][3] == u.weight_bytes
    small = UNet2DConditionModel(text_len=77, **SMALL16)
    assert not any(r[0].startswith("up4@") for r in _regions(small))


def test_split_k_plan_keeps_the_phase_op_unsplit(net):
    u, _ = net
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 4, 32, 32, generator=g).cuda()
    e = torch.randn(1, 77, 768, generator=g).cuda()
    u.set_split_k(True)
    try:
        ks = _kernels(u, x, e)
    finally:
        u.set_split_k(False)
    assert ks.get("k_conv_up4<10>") == 1 and any("/s" in k for k in ks), ks
