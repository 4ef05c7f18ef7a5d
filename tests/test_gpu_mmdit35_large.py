"""A 2432-wide MMDiT on the engine (SD-3.5-large's width: 38 heads of 64, q/k RMS norm, no dual-attention blocks): the small network of
tests_support/mmdit35_large_case.py -- 2 blocks, so the ordinary and the context_pre_only block both occur -- against
tests_support/mmdit35_oracle.py in every storage mode, graph replays and row blocks bit for bit, and a two-shard checkpoint directory
through SD3SafeDenoiserPipeline.from_pretrained.
Bounds (mmdit35_large_case.bounds): those tests/test_gpu_mmdit35.py holds the small SD-3.5 network to, times s = max(1, d_wide /
d_small), d = the fp16-emulating oracle's distance from the fp32 oracle of each network (reference-only; measured d_wide 6.4e-4,
d_small 8.4e-4, s = 1): 5e-3 fp16, 4e-2 bf16, 1.47e-6 fp32, 1.47e-5 bf16x3 (the figures of the run on MI355X; the test computes them
where it runs).  tests/test_mmdit35_large_host.py asserts that a network
whose LayerNorms stop at column 2048, or whose attention stops at head 32, lies 4.0e-1 / 4.8e-2 from the right one: outside these.
Measured on MI355X, rel L2 vs the emulating / the fp32 oracle: fp16 3.3e-4 / 6.4e-4, bf16 2.4e-3 / 5.2e-3; vs the fp32 oracle: fp32
1.21e-6, bf16x3 1.61e-6; the fp16 output is 4.3e-1 / 4.8e-2 from the two wrong networks."""
import json
import os

import pytest
import torch

from safe_denoiser_amd import _lib
from tests_support import mmdit35_large_case as case

pytestmark = pytest.mark.gpu


def _forward(m):
    x, e, pl = case.inputs()
    y = m(x.cuda(), timestep=torch.tensor([case.T_STEP] * 2).cuda(), encoder_hidden_states=e.cuda(), pooled_projections=pl.cuda())[0]
    torch.cuda.synchronize()
    return y


@pytest.fixture
def no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_wide_sd35_matches_oracle(dtype):
    m = case.model(dtype)
    m.load_state_dict(case.state_dict())
    y = _forward(m)
    assert y.shape == (2, 16, 8, 8) and torch.isfinite(y).all()
    bound = case.bounds()["fp16" if dtype == torch.float16 else "bf16"]
    r_em, r_32 = case.rel_l2(y, case.reference(dtype)), case.rel_l2(y, case.reference(None))
    print(f"wide sd35 mmdit {dtype}: rel L2 vs emulating oracle {r_em:.3e}, vs fp32 oracle {r_32:.3e} (bound {bound:.3e}, scale {case.scale()})")
    assert r_em <= bound and r_32 <= bound
    if dtype == torch.float16:
        far = {k: case.rel_l2(y, case.reference(None, k)) for k in ("ln2048", "heads32")}
        print(f"wide sd35 mmdit fp16: distance to the wrong networks {far}")
        assert min(far.values()) > 4 * bound


def test_wide_sd35_precise_plans(no_tf32):
    b = case.bounds()
    res = {}
    for precision in ("fp32", "bf16x3"):
        m = case.model(precision=precision)
        m.load_state_dict(case.state_dict())
        y = _forward(m)
        assert y.dtype == torch.float32 and torch.isfinite(y).all()
        res[precision] = case.rel_l2(y, case.reference(None))
        del m
    print(f"wide sd35 mmdit vs the fp32 oracle: fp32 {res['fp32']:.2e} (bound {b['fp32']:.2e}), bf16x3 {res['bf16x3']:.2e} (bound {b['bf16x3']:.2e})")
    assert res["fp32"] <= b["fp32"] and res["bf16x3"] <= b["bf16x3"]


def test_row_blocks_and_graph_replays_are_bit_identical():
    m = case.model(torch.float16)
    m.load_state_dict(case.state_dict())
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 16, 8, 8, generator=g).cuda(); e = m.prepare_text(torch.randn(5, case.TEXT_LEN, 128, generator=g).cuda())
    pl = torch.randn(5, 64, generator=g).cuda().half()
    ref, y = torch.empty(5, 16, 8, 8, device="cuda"), torch.empty(5, 16, 8, 8, device="cuda")
    m.forward_into(x, case.T_STEP, e, pl, ref)
    m.max_samples = lambda: 2                                        # 5 samples as 2 + 2 + 1
    m.forward_into(x, case.T_STEP, e, pl, y)
    assert torch.equal(y, ref)
    del m.max_samples
    _lib.lib().sdn_unet_set_graph_mode(m._h, 1)
    for _ in range(2):                                               # capture, then replay
        y.zero_()
        m.forward_into(x, case.T_STEP, e, pl, y)
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
    _lib.lib().sdn_unet_set_graph_mode(m._h, 0)


def test_full_depth_sd35_large_plan_runs():
    """All 38 blocks at 2432 wide (8.06 B parameters generated on the GPU), latent side 16: with this depth the stacked adaLN weight is
    5.4 GB, above the 16-bit GEMM's 2 GiB operand limit, so the planner emits that GEMM in three groups (sdn_plan_mmdit.hip); the
    forward is finite and each row of the B = 2 forward equals its B = 1 forward."""
    from safe_denoiser_amd.mmdit import SD35_LARGE, SD3Transformer2DModel
    m = SD3Transformer2DModel(**dict(SD35_LARGE, sample_size=16))
    m.load_synthetic_on_device(0)
    x = torch.randn(2, 16, 16, 16, device="cuda"); e = torch.randn(2, 333, 4096, device="cuda"); pl = torch.randn(2, 2048, device="cuda")
    y = m(x, timestep=900.0, encoder_hidden_states=e, pooled_projections=pl)[0]
    y0 = m(x[:1], timestep=900.0, encoder_hidden_states=e[:1], pooled_projections=pl[:1])[0]
    y1 = m(x[1:], timestep=900.0, encoder_hidden_states=e[1:], pooled_projections=pl[1:])[0]
    torch.cuda.synchronize()
    assert y.shape == (2, 16, 16, 16) and torch.isfinite(y).all() and float(y.float().std()) > 0
    assert torch.equal(y0, y[:1]) and torch.equal(y1, y[1:])


def test_from_a_two_shard_checkpoint_directory(tmp_path):
    """A directory with this configuration and a sharded transformer/ (two files and the index): from_pretrained, which passes
    max_width = mmdit.MAX_WIDTH, builds the same transformer as the constructor, bit for bit."""
    from safetensors.torch import save_file

    from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline
    root = tmp_path / "sd35_wide"
    (root / "transformer").mkdir(parents=True)
    (root / "scheduler").mkdir()
    tjson = {**case.WIDE, "_class_name": "SD3Transformer2DModel", "in_channels": 16, "out_channels": 16, "patch_size": 2, "attention_head_dim": 64,
             "caption_projection_dim": case.WIDTH, "sample_size": 128, "qk_norm": "rms_norm", "dual_attention_layers": []}
    (root / "transformer" / "config.json").write_text(json.dumps(tjson))
    sd = case.state_dict()
    names = sorted(sd)
    shards = {"diffusion_pytorch_model-00001-of-00002.safetensors": names[:len(names) // 2],
              "diffusion_pytorch_model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for fname, keys in shards.items():
        save_file({k: sd[k].half().contiguous() for k in keys}, os.path.join(root, "transformer", fname))
    index = {"metadata": {}, "weight_map": {k: fname for fname, keys in shards.items() for k in keys}}
    (root / "transformer" / "diffusion_pytorch_model.safetensors.index.json").write_text(json.dumps(index))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps({"_class_name": "FlowMatchEulerDiscreteScheduler",
                                                                          "num_train_timesteps": 1000, "shift": 3.0}))
    pipe = SD3SafeDenoiserPipeline.from_pretrained(str(root), image_length=64)
    tr = pipe.transformer
    assert tr.config.qk_norm == "rms_norm" and tr.config.dual_attention_layers == () and tr.config.num_attention_heads == 38
    assert tr.config.sample_size == 8 and tr.text_len == 333
    hand = case.model(torch.float16, text_len=333)
    hand.load_state_dict({k: v.half() for k, v in sd.items()})
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16, 8, 8, generator=g).cuda(); e = torch.randn(2, 333, 128, generator=g).cuda(); pl = torch.randn(2, 64, generator=g).cuda()
    kw = dict(timestep=500.0, encoder_hidden_states=e, pooled_projections=pl)
    y = tr(x, **kw)[0]
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and torch.equal(y, hand(x, **kw)[0])
