"""The smallest MMDiT that is still as wide as SD-3.5-large (2432 = 38 heads of 64), shared by tests/test_mmdit35_large_host.py and
tests/test_gpu_mmdit35_large.py: 2 blocks (one ordinary, one context_pre_only), q/k RMS norm, no dual-attention blocks, latent side 8
(16 image tokens), 13 text tokens -- about 0.36 B parameters.  Everything here runs on the CPU and is computed once per process
(functools caches): the tests only read the results.

Two deliberately WRONG oracles stand for the two ways the width can go wrong on the engine without anything else failing:
  ln2048:  every LayerNorm takes its statistics over columns 0..2047 and writes those columns only (zeros behind them): a row-wise
           kernel that stopped at the old four chunks;
  heads32: the attention output of heads 32..37 is zero: an attention launch that covered 32 heads.
The host test asserts both land outside the fp16 bound the engine is held to."""
import functools
import types

import torch
import torch.nn.functional as F

from safe_denoiser_amd.mmdit import SD3Transformer2DModel
from tests_support import mmdit35_case as small
from tests_support import mmdit35_oracle
from tests_support.mmdit35_oracle import OracleMMDiT35

WIDTH = 2432
WIDE = dict(sample_size=8, num_layers=2, num_attention_heads=38, joint_attention_dim=128, pooled_projection_dim=64, pos_embed_max_size=24)
WIDE_O = dict(sample_size=8, num_layers=2, num_heads=38, joint_dim=128, pooled_dim=64, pos_embed_max_size=24)
FEATURES = dict(qk_norm="rms_norm", dual_attention_layers=())
TEXT_LEN, T_STEP, WEIGHT_SEED, INPUT_SEED = 13, 812.0, 5, 3
# transformer/config.json of stabilityai/stable-diffusion-3.5-large, restated from the published definition
SD35_LARGE_JSON = {"_class_name": "SD3Transformer2DModel", "_diffusers_version": "0.31.0.dev0", "attention_head_dim": 64,
                   "caption_projection_dim": 2432, "dual_attention_layers": [], "in_channels": 16, "joint_attention_dim": 4096,
                   "num_attention_heads": 38, "num_layers": 38, "out_channels": 16, "patch_size": 2, "pooled_projection_dim": 2048,
                   "pos_embed_max_size": 192, "qk_norm": "rms_norm", "sample_size": 128}
rel_l2 = small.rel_l2


def model(dtype=torch.float16, precision=None, text_len=TEXT_LEN):
    if precision:
        return SD3Transformer2DModel(text_len=text_len, precision=precision, **WIDE, **FEATURES)
    return SD3Transformer2DModel(text_len=text_len, dtype=dtype, **WIDE, **FEATURES)


@functools.lru_cache(maxsize=None)
def state_dict():
    """Synthetic weights (seed 5; q/k gains from U(1, 3)).  Shared: do not modify."""
    return model().synthetic_state_dict(WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def inputs():
    g = torch.Generator().manual_seed(INPUT_SEED)
    return torch.randn(2, 16, 8, 8, generator=g), torch.randn(2, TEXT_LEN, 128, generator=g), torch.randn(2, 64, generator=g)


def _ln_first_2048(x):
    y = torch.zeros_like(x)
    y[..., :2048] = F.layer_norm(x[..., :2048], (2048,), eps=1e-6)
    return y


def _sdpa_first_32_heads(q, k, v):
    a = F.scaled_dot_product_attention(q, k, v)                    # [b, heads, n, 64]
    a[:, 32:] = 0
    return a


@functools.lru_cache(maxsize=None)
def reference(act_dtype=None, wrong=None):
    """Output of the oracle of the wide network; wrong = "ln2048" / "heads32": one of the two wrong networks (module docstring)."""
    x, e, pl = inputs()
    o = OracleMMDiT35(state_dict(), WIDE_O, act_dtype=act_dtype, **FEATURES)
    if wrong == "ln2048":
        o.ln = _ln_first_2048
        return o(x, T_STEP, e, pl)
    if wrong == "heads32":
        real = mmdit35_oracle.F
        proxy = types.SimpleNamespace(**{n: getattr(real, n) for n in ("conv2d", "silu", "gelu", "linear", "layer_norm")},
                                      scaled_dot_product_attention=_sdpa_first_32_heads)
        mmdit35_oracle.F = proxy                                      # the oracle's attention only; restored below
        try:
            return o(x, T_STEP, e, pl)
        finally:
            mmdit35_oracle.F = real
    assert wrong is None
    return o(x, T_STEP, e, pl)


@functools.lru_cache(maxsize=None)
def scale():
    """(d_wide, d_small, s): the fp16-emulating oracle's distance from the fp32 oracle for this network and for the small SD-3.5 one
    (tests_support/mmdit35_case.py), and s = max(1, d_wide / d_small): how much more the wide network amplifies rounding.  A
    reference-only quantity: the engine is not involved."""
    d_wide = rel_l2(reference(torch.float16), reference(None))
    d_small = small.amplification()[0]
    return d_wide, d_small, max(1.0, d_wide / d_small)


@functools.lru_cache(maxsize=None)
def bounds():
    """rel-L2 bounds per plan: those tests/test_gpu_mmdit35.py holds the small SD-3.5 network to (5e-3 fp16, 4e-2 bf16, and
    1.2e-6 / 1.2e-5 times its own s35 = max(1, d35 / d3) for the fp32 / bf16x3 plans), times s of scale()."""
    s = scale()[2]
    d35, d3 = small.amplification()
    s35 = max(1.0, d35 / d3)
    return {"fp16": small.TOL[torch.float16] * s, "bf16": small.TOL[torch.bfloat16] * s, "fp32": 1.2e-6 * s35 * s, "bf16x3": 1.2e-5 * s35 * s}
