"""SD-3.5 MMDiT on the engine (q/k RMS norm, dual-attention blocks): the small network of tests_support/mmdit35_case.py against
tests_support/mmdit35_oracle.py in every storage mode, each addition on its own, row blocks and graph replays bit for bit, the full
SD-3.5-medium plan, and a checkpoint directory through SD3SafeDenoiserPipeline.from_pretrained.
Bounds: 16-bit plans, those of test_small_mmdit_matches_oracle (5e-3 fp16, 4e-2 bf16); precise plans, the small-net bounds of
tests/test_gpu_mmdit_precise.py (1.2e-6 fp32, 1.2e-5 bf16x3) times s = max(1, d35 / d3), where d35 and d3 are the distances of the
fp16-emulating from the fp32 oracle for this network and for the small SD-3 one: a reference-only measure of how much more this
network amplifies rounding.  Measured on two hosts: d35 = 8.25e-4 / 8.40e-4, d3 = 6.89e-4 / 6.86e-4, s = 1.197 / 1.225 (the CPU oracle's
own sums differ with the host's vector width); the test computes s where it runs.
Measured on MI355X (profiles/sd35_mmdit.json), rel L2 vs the emulating / the fp32 oracle: fp16 5.2e-4 / 8.3e-4, bf16 4.0e-3 / 6.7e-3,
q/k norm alone 4.6e-4 / 7.6e-4, dual attention alone 2.5e-4 / 7.1e-4; precise plans vs the fp32 oracle: fp32 8.2e-7, bf16x3 7.2e-6
(bounds 1.47e-6 / 1.47e-5 at s = 1.225); distance of the fp16 output to the wrong networks 5.0e-2 ... 1.7e-1."""
import json
import os

import pytest
import torch

from safe_denoiser_amd import _lib
from safe_denoiser_amd.mmdit import SD35_MEDIUM, SD3Transformer2DModel
from tests_support import mmdit35_case as case

pytestmark = pytest.mark.gpu


def _forward(m, batch=2):
    x, e, pl = case.inputs()
    y = m(x[:batch].cuda(), timestep=torch.tensor([case.T_STEP] * batch).cuda(), encoder_hidden_states=e[:batch].cuda(),
          pooled_projections=pl[:batch].cuda())[0]
    torch.cuda.synchronize()
    return y


@pytest.fixture
def no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_small_sd35_matches_oracle(dtype):
    m = case.model(dtype)
    m.load_state_dict(case.state_dict())
    y = _forward(m)
    assert y.shape == (2, 16, 16, 16) and torch.isfinite(y).all()
    r_em, r_32 = case.rel_l2(y, case.reference(dtype)), case.rel_l2(y, case.reference(None))
    print(f"small sd35 mmdit {dtype}: rel L2 vs emulating oracle {r_em:.3e}, vs fp32 oracle {r_32:.3e}")
    assert r_em <= case.TOL[dtype] and r_32 <= case.TOL[dtype]
    if dtype == torch.float16:
        # a plan without the norms, without attn2 or with a gain of ones would sit ON one of these; the right one is far from all
        far = {k: case.rel_l2(y, v) for k, v in case.wrong_references().items()}
        print(f"small sd35 mmdit fp16: distance to the wrong networks {far}")
        assert min(far.values()) > 2.5e-2


@pytest.mark.parametrize("features", [dict(qk_norm="rms_norm", dual_attention_layers=()), dict(qk_norm=None, dual_attention_layers=(1,))],
                         ids=["qk_norm_only", "dual_only"])
def test_each_addition_alone(features):
    m = case.model(torch.float16, **features)
    m.load_state_dict(case.state_dict(**features))
    y = _forward(m)
    key = tuple(sorted(features.items()))
    r_em, r_32 = case.rel_l2(y, case.reference(torch.float16, key)), case.rel_l2(y, case.reference(None, key))
    print(f"small sd35 mmdit fp16 {features}: rel L2 vs emulating oracle {r_em:.3e}, vs fp32 oracle {r_32:.3e}")
    assert torch.isfinite(y).all() and r_em <= 5e-3 and r_32 <= 5e-3


def test_small_sd35_precise_plans(no_tf32):
    d35, d3 = case.amplification()
    s = max(1.0, d35 / d3)
    res = {}
    for precision in ("fp32", "bf16x3"):
        m = case.model(precision=precision)
        m.load_state_dict(case.state_dict())
        y = _forward(m)
        assert y.dtype == torch.float32 and torch.isfinite(y).all()
        res[precision] = case.rel_l2(y, case.reference(None))
    print(f"small sd35 mmdit vs the fp32 oracle: fp32 {res['fp32']:.2e}, bf16x3 {res['bf16x3']:.2e}; d35 {d35:.3e}, d3 {d3:.3e}, s {s:.3f}")
    assert 1.0 <= s < 1.5                                            # the two networks amplify rounding alike (measured 1.20 / 1.23)
    assert res["fp32"] <= 1.2e-6 * s and res["bf16x3"] <= 1.2e-5 * s


def test_row_blocks_and_graph_replays_are_bit_identical():
    m = case.model(torch.float16)
    m.load_state_dict(case.state_dict())
    g = torch.Generator().manual_seed(9)
    x = torch.randn(7, 16, 16, 16, generator=g).cuda(); e = m.prepare_text(torch.randn(7, 45, 128, generator=g).cuda())
    pl = torch.randn(7, 64, generator=g).cuda().half()
    ref, y = torch.empty(7, 16, 16, 16, device="cuda"), torch.empty(7, 16, 16, 16, device="cuda")
    m.forward_into(x, case.T_STEP, e, pl, ref)
    m.max_samples = lambda: 3                                        # 7 samples as 2 + 2 + 2 + 1
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


def test_full_sd35_medium_plan_runs():
    """The 2.24 B-parameter SD-3.5-medium plan at 512 x 512 (latent 64), weights generated on the GPU: shape, finiteness, batch rows
    independent (each row of the B = 2 forward is its B = 1 forward)."""
    m = SD3Transformer2DModel(**dict(SD35_MEDIUM, sample_size=64))
    m.load_synthetic_on_device(0)
    x = torch.randn(2, 16, 64, 64, device="cuda"); e = torch.randn(2, 333, 4096, device="cuda"); pl = torch.randn(2, 2048, device="cuda")
    y = m(x, timestep=900.0, encoder_hidden_states=e, pooled_projections=pl)[0]
    y0 = m(x[:1], timestep=900.0, encoder_hidden_states=e[:1], pooled_projections=pl[:1])[0]
    y1 = m(x[1:], timestep=900.0, encoder_hidden_states=e[1:], pooled_projections=pl[1:])[0]
    torch.cuda.synchronize()
    assert y.shape == (2, 16, 64, 64) and torch.isfinite(y).all()
    assert torch.equal(y0, y[:1]) and torch.equal(y1, y[1:])
    assert float(y.float().std()) > 0


def test_from_a_checkpoint_directory(tmp_path):
    """A tiny SD-3.5-layout directory (transformer config + safetensors, scheduler; no tokenizers, no VAE: embeddings go in, latents come
    out): from_pretrained builds the same transformer as the constructor, bit for bit, and a 3-step call runs."""
    from safetensors.torch import save_file

    from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline
    root = tmp_path / "sd35"
    (root / "transformer").mkdir(parents=True)
    (root / "scheduler").mkdir()
    tjson = {**case.SMALL, "_class_name": "SD3Transformer2DModel", "in_channels": 16, "out_channels": 16, "patch_size": 2, "attention_head_dim": 64,
             "caption_projection_dim": 256, "sample_size": 128, "qk_norm": "rms_norm", "dual_attention_layers": [0, 2]}
    (root / "transformer" / "config.json").write_text(json.dumps(tjson))
    sd = case.state_dict()
    save_file({k: t.contiguous() for k, t in sd.items()}, os.path.join(root, "transformer", "diffusion_pytorch_model.safetensors"))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps({"_class_name": "FlowMatchEulerDiscreteScheduler",
                                                                          "num_train_timesteps": 1000, "shift": 3.0}))
    pipe = SD3SafeDenoiserPipeline.from_pretrained(str(root), image_length=128)
    tr = pipe.transformer
    assert tr.config.qk_norm == "rms_norm" and tr.config.dual_attention_layers == (0, 2) and tr.config.sample_size == 16 and tr.text_len == 333
    assert pipe.text_front_end is None and pipe.vae is None
    hand = case.model(torch.float16, text_len=333)
    hand.load_state_dict(sd)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16, 16, 16, generator=g).cuda(); e = torch.randn(2, 333, 128, generator=g).cuda(); pl = torch.randn(2, 64, generator=g).cuda()
    kw = dict(timestep=500.0, encoder_hidden_states=e, pooled_projections=pl)
    assert torch.equal(tr(x, **kw)[0], hand(x, **kw)[0])
    tape = torch.randn(1, 1, 16, 16, 16, generator=g)
    lat = pipe(prompt_embeds=e, pooled_prompt_embeds=pl, num_inference_steps=3, noise_fn=lambda p, shape: tape[p].clone())
    torch.cuda.synchronize()
    assert tuple(lat.shape) == (1, 16, 16, 16) and bool(torch.isfinite(lat).all())
