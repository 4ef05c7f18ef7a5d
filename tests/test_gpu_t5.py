"""T5 encoder on the engine (sdn_t5_*, safe_denoiser_amd/t5.py, text_sd3.py) on an MI355X: the plan against the transformers
fixture, the new operators alone, exact properties, full-width parity against the torch oracle on the GPU, and the SD-v3
pipeline driven from prompt strings through SD3TextFrontEnd.  Measured distances go to profiles/t5_parity.json."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib
from safe_denoiser_amd.t5 import T5EncoderModel
from safe_denoiser_amd.text_sd3 import SD3TextFrontEnd
from tests_support import exact as X
from tests_support import t5_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "t5_parity.json")
G = O.load_golden()
CFG = dict(G["cfg"])
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
# 16-bit attention bounds of tests/test_gpu_ops.py (same kernel family, same output rounding): bf16 6e-3 on ordinary inputs and
# 8e-3 on inputs that force the running-maximum rescale; fp16 1.2e-3 throughout.
ATTN_BOUND = {"bf16": 6e-3, "f16": 1.2e-3}
ATTN_BOUND_EXTREME = {"bf16": 8e-3, "f16": 1.2e-3}
# Full width, 4 layers, bf16, against the fp32 torch oracle on the same 16-bit weights: measured on MI355X + 25 %
# (the convention of tests/test_gpu_pipeline.py's LOOP_BOUND); the measurements are in profiles/t5_parity.json.
FULL_BOUND = {"2x256": 1.36e-2, "19x21": 1.14e-2}      # measured 1.086e-2 / 9.07e-3


def record(key, value, bound):
    data = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            data = json.load(f)
    data[key] = {"measured": value, "bound": bound}
    with open(PARITY, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def small(dtype, peaked=False):
    m = T5EncoderModel(dtype=dtype, **CFG)
    m.load_state_dict(O.golden_state_dict(G, peaked))
    return m


# ---------------------------------------------------------------------------------------------- 1. engine vs fixture
@pytest.mark.parametrize("arm", ["", "peaked_"])
@pytest.mark.parametrize("case", ["plain", "masked", "n13"])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_engine_matches_the_transformers_fixture(tag, case, arm):
    """Bound = 2 x the distance of transformers' own run at that storage width from its fp32 run (recorded in the fixture)."""
    m = small(DT[tag], peaked=bool(arm))
    ids = torch.from_numpy(G["ids13"] if case == "n13" else G["ids"])
    mask = torch.from_numpy(G["mask"]) if case == "masked" else None
    out = m(ids, attention_mask=mask)
    assert out[0] is out.last_hidden_state and out[0].dtype == DT[tag] and tuple(out[0].shape) == tuple(ids.shape) + (CFG["d_model"],)
    got = out[0].float().cpu()
    assert torch.isfinite(got).all()
    ref = torch.from_numpy(G[arm + case])
    if case == "masked":                           # (padded query rows attend to real keys only; they are compared as well)
        assert got.shape == ref.shape
    err, bound = O.rel_l2(got, ref), 2.0 * float(G[f"err_{tag}_{arm}{case}"])
    print(f"t5 {tag} {arm}{case}: rel L2 {err:.3e} (transformers at this width {bound / 2:.3e}, bound {bound:.3e})")
    record(f"fixture/{tag}/{arm}{case}", err, bound)
    assert err <= bound


# ---------------------------------------------------------------------------------------------- 2. biased attention alone
def run_bias_attention(qkv, bias, mask, H, scale, dtype):
    B, n, _ = qkv.shape
    I = H * 64
    g = qkv.cuda()
    out = torch.empty(B, n, I, dtype=dtype, device="cuda")
    bv = bias.float().cuda().contiguous()
    mk = None if mask is None else mask.to(torch.int32).cuda().contiguous()
    es = 2
    rc = sda.lib().sdn_bias_attention(0 if dtype == torch.bfloat16 else 1, g.data_ptr(), g.data_ptr() + I * es, g.data_ptr() + 2 * I * es,
                                      out.data_ptr(), bv.data_ptr(), None if mk is None else mk.data_ptr(), B, H, n, 64, 3 * I, 3 * I, 3 * I,
                                      I, scale, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.float().cpu()


def ref_bias_attention(qkv, bias, mask, H, scale):
    B, n, _ = qkv.shape
    I = H * 64
    sp = lambda t: t.float().reshape(B, n, H, 64).transpose(1, 2)
    o = O.biased_attention(sp(qkv[..., :I]), sp(qkv[..., I:2 * I]), sp(qkv[..., 2 * I:]), bias.float(), mask, scale)
    return o.transpose(1, 2).reshape(B, n, I)


@pytest.mark.parametrize("amp", [1.0, 30.0])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [2, 13, 77, 256, 512])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_bias_attention_against_torch(tag, n, masked, scale, amp):
    """Strided q / k / v views of ONE stacked [B, n, 3 I] buffer, as the plan passes them."""
    B, H = 3, 4
    g = torch.Generator().manual_seed(1000 + n)
    qkv = (torch.randn(B, n, 3 * H * 64, generator=g) * 0.5).to(DT[tag])
    bias = amp * torch.randn(H, 2 * n - 1, generator=g)
    mask = None
    if masked:
        keep = torch.tensor([n, max(1, n // 3), max(1, n - 1)])
        mask = (torch.arange(n)[None] < keep[:, None]).long()
    out = run_bias_attention(qkv, bias, mask, H, scale, DT[tag])
    ref = ref_bias_attention(qkv, bias, mask, H, scale)
    assert torch.isfinite(out).all()
    err = O.rel_l2(out, ref)
    print(f"bias attention {tag} n={n} masked={masked} scale={scale} amp={amp}: {err:.2e}")
    assert err <= ATTN_BOUND[tag], err


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [13, 77])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_bias_attention_head_inner_block_order(tag, n, masked):
    """batch % 8 == 0 with at most 128 keys selects the head-innermost block order of the attention grid (a masked-token batch
    such as [16, 18] takes it): the bias row must follow the decoded head.  Distinct bias rows per head, amplitude 30."""
    B, H = 8, 4
    g = torch.Generator().manual_seed(2000 + n)
    qkv = (torch.randn(B, n, 3 * H * 64, generator=g) * 0.5).to(DT[tag])
    bias = 30.0 * torch.randn(H, 2 * n - 1, generator=g)
    mask = (torch.arange(n)[None] < torch.randint(1, n + 1, (B, 1), generator=g)).long() if masked else None
    out = run_bias_attention(qkv, bias, mask, H, 1.0, DT[tag])
    ref = ref_bias_attention(qkv, bias, mask, H, 1.0)
    err = O.rel_l2(out, ref)
    print(f"bias attention {tag} B=8 n={n} masked={masked}: {err:.2e}")
    assert torch.isfinite(out).all() and err <= ATTN_BOUND[tag], err


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_bias_attention_large_scores_stay_finite(tag):
    """q scaled so that row maxima of Q K^T + bias reach ~150: exp leaves f32 past 88 without a running maximum."""
    B, H, n = 2, 4, 256
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(B, n, 3 * H * 64, generator=g) * 0.5
    qkv[..., :H * 64] *= 14.0
    qkv = qkv.to(DT[tag])
    bias = 30.0 * torch.randn(H, 2 * n - 1, generator=g)
    I = H * 64
    s = torch.matmul(qkv[..., :I].float().reshape(B, n, H, 64).transpose(1, 2), qkv[..., I:2 * I].float().reshape(B, n, H, 64).transpose(1, 2).transpose(-1, -2))
    s = s + O.expand_bias(bias, n)[None]
    row_max = s.amax(-1)
    print(f"row maxima: median {float(row_max.median()):.1f}, max {float(row_max.max()):.1f}")
    assert float(row_max.median()) > 100 and float(row_max.max()) > 150
    out = run_bias_attention(qkv, bias, None, H, 1.0, DT[tag])
    ref = ref_bias_attention(qkv, bias, None, H, 1.0)
    assert torch.isfinite(out).all()
    err = O.rel_l2(out, ref)
    print(f"bias attention {tag} large scores: {err:.2e}")
    assert err <= ATTN_BOUND_EXTREME[tag], err


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("n", [2, 13, 256, 512])
def test_relative_bias_vector_on_device(tag, n):
    H = 6
    table = torch.randn(32, H, generator=torch.Generator().manual_seed(n)).to(DT[tag])
    out = torch.full((H, 2 * n - 1), float("nan"), device="cuda")
    t = table.cuda()
    assert sda.lib().sdn_t5_relative_bias(0 if tag == "bf16" else 1, t.data_ptr(), 32, 128, H, n, out.data_ptr(), _lib.stream_ptr()) == 0
    assert torch.equal(out.cpu(), O.bias_vector(table.float(), n))              # a table lookup: bit for bit


# ---------------------------------------------------------------------------------------------- 3. RMS norm / gated tanh-GELU GEMM
@pytest.mark.parametrize("x_f32", [True, False])
@pytest.mark.parametrize("rows,c", [(37, 128), (5, 4096), (3, 1000)])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_rmsnorm_against_float64(tag, rows, c, x_f32):
    """One output rounding.  The f32 arithmetic in front of it: the sum of c squares (random-walk error sqrt(c) 2^-24 <= 2^-18 at
    c = 4096, halved by the rsqrt) and three multiplications (2^-24 each): below 2^-18 |y| = ACC * 4 |y|."""
    dt = DT[tag]
    g = torch.Generator().manual_seed(rows * c)
    x = torch.randn(rows, c, generator=g) * 3.0
    x = x if x_f32 else x.to(dt)
    w = 1.0 + 0.2 * torch.randn(c, generator=g)
    buf, view = X.guarded_like((rows, c), dt, "cuda")
    xg, wg = x.cuda(), w.cuda()
    rc = sda.lib().sdn_rmsnorm(0 if tag == "bf16" else 1, xg.data_ptr(), 1 if x_f32 else 0, rows, c, 1e-6, wg.data_ptr(), view.data_ptr(),
                               _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    xd = x.double()
    y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
    st = X.analyse(view.cpu(), y, 4.0 * y.abs())
    print(f"rmsnorm {tag} [{rows},{c}] f32={x_f32}: max ulp {st['max_ulp']:.3f}, exact-rounding rate {st['rate']:.4f}")
    assert X.failures(st, exact_fn=False, direction=False) == []
    assert X.sentinels_intact(buf, view) == 0


@pytest.mark.parametrize("M,N,K", [(200, 512, 128), (384, 20480, 128), (130, 256, 4096)])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_gated_tanh_gelu_gemm_against_float64(tag, M, N, K):
    """SDN_ACT_GEGLU_TANH: out = (x Wv^T) * gelu_tanh(x Wg^T) from the interleaved weight, bias = NULL; the criterion of
    tests/test_gpu_gemm_exact.py (tests_support/exact.py) with the exact tanh-GELU and its evaluation error ACT_REL |g| |h|."""
    from safe_denoiser_amd.unet import _interleave16
    dt = DT[tag]
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(dt)
    wv = (torch.randn(N // 2, K, generator=g) / math.sqrt(K)).to(dt)
    wg = (torch.randn(N // 2, K, generator=g) * 2.0 / math.sqrt(K)).to(dt)
    w = _interleave16(torch.cat([wv, wg]))
    buf, view = X.guarded_like((M, N // 2), dt, "cuda")
    ag, wgp = X.with_nan_tail(a.cuda(), 8), w.cuda()
    d = _lib.GemmDesc(M=M, N=N, K=K, act=5)
    fn = sda.lib().sdn_gemm_bf16 if tag == "bf16" else sda.lib().sdn_gemm_f16
    assert fn(C.byref(d), ag.data_ptr(), None, wgp.data_ptr(), None, None, None, None, view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    A = a.double()
    h, gg = A @ wv.double().t(), A @ wg.double().t()
    sh, sg = A.abs() @ wv.double().abs().t(), A.abs() @ wg.double().abs().t()
    sub_h, sub_g = X.subnormal_term(A, wv.double(), dt), X.subnormal_term(A, wg.double(), dt)
    sh, sg = sh + sub_h / X.ACC, sg + sub_g / X.ACC
    act = X.gelu_tanh64(gg)
    y = h * act
    s = sh * act.abs() + X.GELU_D * h.abs() * sg
    st = X.analyse(view.cpu(), y, s, e_epi=X.ACT_REL * gg.abs() * h.abs())
    print(f"gated tanh-GELU {tag} [{M},{N},{K}]: max ulp {st['max_ulp']:.3f}, max err / bound {st['max_err_over_tol']:.3f}")
    assert X.failures(st, exact_fn=False, direction=False) == []
    assert X.sentinels_intact(buf, view) == 0


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_gemm_into_f32_residual_stream(tag):
    """sdn_gemm_desc.f32_stream: x += A W^T with x F32 in place, 16-bit operands of either dtype (no 16-bit output rounding)."""
    dt = DT[tag]
    M, N, K = 300, 256, 512
    g = torch.Generator().manual_seed(9)
    a, w = torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt)
    x = torch.randn(M, N, generator=g)
    buf, view = X.guarded_like((M, N), torch.float32, "cuda")
    view.copy_(x)
    ag, wg = X.with_nan_tail(a.cuda(), 8), w.cuda()
    d = _lib.GemmDesc(M=M, N=N, K=K, out_kind=1, f32_stream=1)
    fn = sda.lib().sdn_gemm_bf16 if tag == "bf16" else sda.lib().sdn_gemm_f16
    assert fn(C.byref(d), ag.data_ptr(), None, wg.data_ptr(), None, None, None, view.data_ptr(), view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    y = a.double() @ w.double().t() + x.double()
    s = a.double().abs() @ w.double().abs().t() + x.double().abs() + X.subnormal_term(a.double(), w.double(), dt) / X.ACC
    st = X.analyse(view.cpu(), y, s, dtype=torch.float32)
    assert X.failures(st, exact_fn=False, direction=False) == []
    assert X.sentinels_intact(buf, view) == 0


def test_embed_tokens_clamps_and_widens():
    table = torch.randn(50, 64, generator=torch.Generator().manual_seed(2)).half()
    ids = torch.tensor([0, 49, 7, -3, 99], dtype=torch.int32)
    out = torch.empty(5, 64, device="cuda")
    t, i = table.cuda(), ids.cuda()
    assert sda.lib().sdn_embed_tokens(1, i.data_ptr(), t.data_ptr(), 5, 64, 50, out.data_ptr(), _lib.stream_ptr()) == 0
    assert torch.equal(out.cpu(), table.float()[ids.clamp(0, 49).long()])


# ---------------------------------------------------------------------------------------------- 4. properties
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_batch_permutation_and_masked_positions_are_exact(tag):
    m = small(DT[tag], peaked=True)
    ids, mask = torch.from_numpy(G["ids"]), torch.from_numpy(G["mask"])
    perm = torch.tensor([2, 0, 1])
    a = m(ids)[0]
    assert torch.equal(m(ids[perm])[0], a[perm])
    b = m(ids, attention_mask=mask)[0]
    assert torch.equal(m(ids[perm], attention_mask=mask[perm])[0], b[perm])
    ids2 = ids.clone()
    ids2[mask == 0] = torch.randint(2, 512, (int((mask == 0).sum()),), generator=torch.Generator().manual_seed(4))
    c = m(ids2, attention_mask=mask)[0]
    keep = mask.bool().cuda()
    assert torch.equal(c[keep], b[keep]) and not torch.equal(c, b)


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_short_sequence_equals_its_padded_and_masked_form(tag):
    """n = 13 against n = 32 padded with id 0 and masked: the same function of the 13 tokens, other tile boundaries."""
    m = small(DT[tag])
    ids13 = torch.from_numpy(G["ids13"])
    ids32 = torch.zeros(1, 32, dtype=torch.long)
    ids32[:, :13] = ids13
    mask = (torch.arange(32)[None] < 13).long()
    a = m(ids13)[0].float().cpu()
    b = m(ids32, attention_mask=mask)[0][:, :13].float().cpu()
    ref = torch.from_numpy(G["n13"])
    bound = 2.0 * float(G[f"err_{tag}_n13"])
    ea, eb = O.rel_l2(a, ref), O.rel_l2(b, ref)
    print(f"n=13 {ea:.3e}, n=32 padded + masked {eb:.3e}, between them {O.rel_l2(a, b):.3e} (bound {bound:.3e})")
    assert ea <= bound and eb <= bound and O.rel_l2(a, b) <= bound


def test_key_padding_mask_does_not_outlive_its_forward():
    """One handle runs a forward with a key-padding mask (keys masked in every row), then one without: the second equals a fresh
    handle's unmasked forward on the same ids, bit for bit.  n = 8, batch 2."""
    ids = torch.from_numpy(G["ids"])[:2, :8]
    mask = (torch.arange(8)[None] < torch.tensor([[5], [3]])).long()
    m, fresh = small(DT["bf16"]), small(DT["bf16"])
    want = fresh(ids)[0]
    assert not torch.equal(m(ids, attention_mask=mask)[0], want)          # the mask is not a no-op on these rows
    assert torch.equal(m(ids)[0], want)


# ---------------------------------------------------------------------------------------------- 5. full width
XXL4 = dict(num_layers=4)


def device_state_dict(m, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for name, shape in m.state_dict_shapes().items():
        if len(shape) == 1:
            sd[name] = 1.0 + 0.1 * (torch.rand(shape, generator=g, device="cuda") - 0.5)
        else:
            # T5's own initialisation scales (transformers T5PreTrainedModel._init_weights): std fan_in^-0.5, and q smaller by
            # sqrt(d_kv) -- the 1 / sqrt(d) that T5 attention does not apply lives in q's weights.  Bias amplitude of a trained table.
            amp = 4.0 if "relative_attention_bias" in name else (3.0 / shape[1]) ** 0.5 / (8.0 if name.endswith(".q.weight") else 1.0)
            sd[name] = ((torch.rand(shape, generator=g, device="cuda") * 2 - 1) * amp).to(m.dtype)
    return sd


@pytest.fixture(scope="module")
def xxl4():
    m = T5EncoderModel(dtype=torch.bfloat16, **XXL4)
    sd = device_state_dict(m, 11)
    m.load_state_dict(sd)
    return m, sd


@pytest.mark.parametrize("shape", [(2, 256), (19, 21)])
def test_full_width_four_layers_against_the_oracle_on_the_gpu(xxl4, shape):
    m, sd = xxl4
    key = f"{shape[0]}x{shape[1]}"
    ids = torch.randint(0, 32128, shape, generator=torch.Generator().manual_seed(shape[1])).cuda()
    out = m(ids)[0].float()
    ref = O.t5_encoder({k: v.float() for k, v in sd.items()}, ids, None, num_heads=64, d_kv=64)
    assert torch.isfinite(out).all() and tuple(out.shape) == shape + (4096,)
    err = O.rel_l2(out, ref)
    print(f"T5 full width, 4 layers, bf16 {key}: rel L2 vs fp32 oracle {err:.3e} (bound {FULL_BOUND[key]:.3e})")
    record(f"full_width_4_layers/bf16/{key}", err, FULL_BOUND[key])
    assert err <= FULL_BOUND[key]


def test_full_depth_forward_is_finite():
    m = T5EncoderModel(dtype=torch.bfloat16).load_synthetic_on_device(3)
    ids = torch.randint(0, 32128, (2, 256), generator=torch.Generator().manual_seed(1)).cuda()
    out = m(ids)[0]
    assert tuple(out.shape) == (2, 256, 4096) and out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    assert float(out.float().abs().mean()) > 0.1


# ---------------------------------------------------------------------------------------------- 6. pipeline from prompt strings
def test_sd3_pipeline_with_the_engine_front_end():
    from safe_denoiser_amd.mmdit import SD3Transformer2DModel
    from safe_denoiser_amd.pipeline_sd3 import SD3_NEGATIVE_PROMPT_SPACE, SD3SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
    import tests.test_gpu_mmdit as tm                      # its small MMDiT configuration, read and not edited
    t5 = small(torch.float16)
    tok = O.FakeT5Tokenizer(vocab_size=CFG["vocab_size"])

    def clip_embeds(prompts):
        import zlib
        g = [torch.Generator().manual_seed(zlib.crc32(p.encode())) for p in prompts]
        return (torch.stack([torch.randn(77, 96, generator=x) for x in g]).cuda(), torch.stack([torch.randn(64, generator=x) for x in g]).cuda())

    fe = SD3TextFrontEnd(t5, tok, clip_embeds)
    m = SD3Transformer2DModel(text_len=77 + 256, dtype=torch.float16, **tm.SMALL)
    m.load_state_dict(m.synthetic_state_dict(5))
    prompts = ["a lustful portrait in oil", "two cats asleep on a red sofa in the evening sun"]
    P = len(prompts)
    tape = torch.randn(P, 1, 16, 16, 16, generator=torch.Generator().manual_seed(3))
    nf = lambda p, shape: tape[p].clone()
    kw = dict(num_inference_steps=4, guidance_scale=3.5, noise_fn=nf)
    pipe = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler(), text_front_end=fe)
    out = pipe(prompt=prompts, **kw)
    stats = dict(pipe.last_stats)
    joined = ", ".join(SD3_NEGATIVE_PROMPT_SPACE)
    pe, ne, pp, npp = fe.encode_prompt(prompt=prompts, negative_prompt=[joined] * P)
    assert pe.shape == (P, 333, 128) and pe.dtype == torch.float16 and torch.all(pe[:, :77, 96:] == 0)
    masked = [fe.masked_encode_prompt(p) for p in prompts]
    assert [tuple(x.shape) for x in masked] == [(len(p.split()) - 1, 128) for p in prompts]
    space = fe.encode_negative_prompt_space(SD3_NEGATIVE_PROMPT_SPACE)
    plain = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler())
    same = plain(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=npp,
                 masked_embs=masked, negspace_embs=space, **kw)
    assert torch.isfinite(out).all() and torch.equal(out, same)
    assert plain.last_stats == stats
