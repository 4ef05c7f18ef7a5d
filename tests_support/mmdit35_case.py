"""The small SD-3.5 MMDiT case shared by tests/test_mmdit35_host.py and tests/test_gpu_mmdit35.py: configuration, weights, inputs and
the oracles (right and deliberately wrong) the two files compare with.  Everything here runs on the CPU and is computed once per
process (functools caches): the tests only read the results."""
import functools

import torch

from oracle.mmdit import OracleMMDiT
from safe_denoiser_amd.mmdit import QK_NORM_GAINS, SD3Transformer2DModel
from tests_support.mmdit35_oracle import OracleMMDiT35

# the small SD-3 network of tests/test_gpu_mmdit.py ...
SMALL = dict(sample_size=16, num_layers=3, num_attention_heads=4, joint_attention_dim=128, pooled_projection_dim=64, pos_embed_max_size=24)
SMALL_O = dict(sample_size=16, num_layers=3, num_heads=4, joint_dim=128, pooled_dim=64, pos_embed_max_size=24)
# ... with both additions; blocks 0 and 2 are dual, so the last (context_pre_only) block is
FEATURES = dict(qk_norm="rms_norm", dual_attention_layers=(0, 2))
TEXT_LEN, T_STEP, WEIGHT_SEED, INPUT_SEED = 45, 812.0, 5, 3
TOL = {torch.float16: 5e-3, torch.bfloat16: 4e-2}          # the bounds of test_small_mmdit_matches_oracle


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def model(dtype=torch.float16, precision=None, text_len=TEXT_LEN, **features):
    kw = dict(SMALL, **(features if features else FEATURES))
    if precision:
        return SD3Transformer2DModel(text_len=text_len, precision=precision, **kw)
    return SD3Transformer2DModel(text_len=text_len, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def _state_dict(features: tuple):
    return model(**dict(features)).synthetic_state_dict(WEIGHT_SEED)


def state_dict(**features):
    """Synthetic weights (seed 5) of the small network with `features` (default: both).  Shared: do not modify."""
    return _state_dict(tuple(sorted((features if features else FEATURES).items())))


@functools.lru_cache(maxsize=None)
def inputs():
    g = torch.Generator().manual_seed(INPUT_SEED)
    return torch.randn(2, 16, 16, 16, generator=g), torch.randn(2, 45, 128, generator=g), torch.randn(2, 64, generator=g)


def oracle_out(sd, act_dtype=None, features=None, **wrong):
    x, e, pl = inputs()
    return OracleMMDiT35(sd, SMALL_O, act_dtype=act_dtype, **(FEATURES if features is None else features), **wrong)(x, T_STEP, e, pl)


@functools.lru_cache(maxsize=None)
def reference(act_dtype=None, features: tuple = None):
    """Output of the (right) oracle of the small network with `features` (a sorted item tuple; default both)."""
    f = dict(features) if features is not None else FEATURES
    return oracle_out(state_dict(**f), act_dtype, f)


# Gain vectors whose replacement by ones the network output shows (measured on the fp32 oracle: 5.2e-2, 7.3e-2, 5.0e-2): one of the
# image stream, one of the text stream, one of attn2 -- the last of them the least visible of the 13 vectors of these families.
# NOT in this list: the text stream's norm_added_q of blocks 0 and 1 moves the output by 9.8e-3 / 7.8e-3 only (the text stream reaches
# the output through the next block's keys and values alone) -- above the fp16 bound, below the bf16 one; the kernel test's gain
# selection checks cover what the network test cannot see.
LIVE_GAINS = ("transformer_blocks.2.attn.norm_q.weight", "transformer_blocks.1.attn.norm_added_k.weight",
              "transformer_blocks.2.attn2.norm_k.weight")
DEAD_GAIN = "transformer_blocks.2.attn.norm_added_q.weight"     # the last block's text output is discarded


def with_ones(name):
    sd = dict(state_dict())
    assert name.endswith(QK_NORM_GAINS)
    sd[name] = torch.ones_like(sd[name])
    return sd


@functools.lru_cache(maxsize=None)
def wrong_references():
    """fp32 outputs of the wrong networks: (c) no q/k norms, (d) no attn2, (e) one live gain vector replaced by ones (each of LIVE_GAINS)."""
    sd = state_dict()
    out = dict(no_qk_norm=oracle_out(sd, skip_qk_norm=True), no_attn2=oracle_out(sd, skip_attn2=True))
    out.update({"ones:" + k: oracle_out(with_ones(k)) for k in LIVE_GAINS})
    return out


@functools.lru_cache(maxsize=None)
def amplification():
    """(d35, d3): distance of the fp16-emulating from the fp32 oracle for the small SD-3.5 net and for the small SD-3 net of
    tests/test_gpu_mmdit_precise.py (same seeds): how much more the new net amplifies rounding."""
    d35 = rel_l2(reference(torch.float16), reference(None))
    m3 = SD3Transformer2DModel(text_len=TEXT_LEN, **SMALL)
    sd3 = m3.synthetic_state_dict(WEIGHT_SEED)
    x, e, pl = inputs()
    d3 = rel_l2(OracleMMDiT(sd3, SMALL_O, act_dtype=torch.float16)(x, T_STEP, e, pl), OracleMMDiT(sd3, SMALL_O, act_dtype=None)(x, T_STEP, e, pl))
    return d35, d3
