"""Host-side checks of the T5 encoder work: the torch oracle against the transformers fixture, the relative-position bias vector
against transformers' compute_bias, the engine's bucket function, SD3TextFrontEnd's id construction with stub encoders,
checkpoint helpers, and argument validation of the new C entry points.  No GPU."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint
from safe_denoiser_amd.t5 import T5EncoderModel
from safe_denoiser_amd.text_sd3 import SD3TextFrontEnd
from tests_support import t5_oracle as O

G = O.load_golden()
CFG = dict(G["cfg"])


@pytest.mark.parametrize("arm", ["", "peaked_"])
@pytest.mark.parametrize("case", ["plain", "masked", "n13"])
def test_oracle_reproduces_the_fixture(arm, case):
    sd = O.golden_state_dict(G, peaked=bool(arm))
    ids = torch.from_numpy(G["ids13"] if case == "n13" else G["ids"])
    mask = torch.from_numpy(G["mask"]) if case == "masked" else None
    out = O.t5_encoder(sd, ids, mask, num_heads=CFG["num_heads"], d_kv=CFG["d_kv"])
    err = O.rel_l2(out, torch.from_numpy(G[arm + case]))
    print(arm + case, err)
    assert err <= 1e-5                                         # fp32 summation order and nothing else


@pytest.mark.parametrize("n", [2, 13, 256, 512])
def test_bias_vector_equals_transformers_compute_bias(n):
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention
    torch.manual_seed(1)
    att = T5Attention(T5Config(d_model=128, d_kv=64, num_heads=4, relative_attention_num_buckets=32,
                               relative_attention_max_distance=128, is_decoder=False), has_relative_attention_bias=True)
    with torch.no_grad():
        full = att.compute_bias(n, n)[0]                                          # [H, n, n]
        vec = O.bias_vector(att.relative_attention_bias.weight, n)
    assert torch.equal(O.expand_bias(vec, n), full)                               # Toeplitz, and a table lookup: bit for bit
    # ... and the engine's host bucket function agrees with transformers on every distance
    rel = torch.arange(-(n - 1), n)
    want = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128)
    got = [sda.lib().sdn_t5_bucket(int(r), 32, 128) for r in rel]
    assert got == want.tolist()


class _StubT5:
    """Records the ids it is called with; hidden state [b, n, d] = id + 1000 * position (so a test can see what was read)."""
    dtype = torch.float32

    def __init__(self, d_model=8):
        self.config = SimpleNamespace(d_model=d_model)
        self.calls = []

    def __call__(self, input_ids, attention_mask=None):
        self.calls.append((input_ids.clone(), None if attention_mask is None else attention_mask.clone()))
        b, n = input_ids.shape
        h = (input_ids.float() + 1000.0 * torch.arange(n)[None])[:, :, None].expand(b, n, self.config.d_model).contiguous()
        return _Out(h)


class _Out(tuple):
    def __new__(cls, h):
        o = super().__new__(cls, (h,))
        o.last_hidden_state = h
        return o


def _clip(prompts):
    p = len(prompts)
    return torch.full((p, 77, 6), 7.0), torch.full((p, 5), 3.0)


def test_front_end_masked_ids_and_empty_prompt():
    t5, tok = _StubT5(), O.FakeT5Tokenizer(vocab_size=512)
    fe = SD3TextFrontEnd(t5, tok, _clip)
    ids = tok("a photo of a cat", padding="longest", max_length=256, truncation=True).input_ids      # 5 words + end token
    assert ids.shape == (1, 6)
    out = fe.masked_encode_prompt("a photo of a cat")
    (seen, mask), = t5.calls
    assert mask is None and seen.shape == (4, 6) and out.shape == (4, 8)          # n_real = n - 2, the reference's count
    for i in range(4):
        want = ids[0].clone(); want[i + 1] = 0
        assert torch.equal(seen[i], want)
    assert torch.equal(out[:, 0], seen[:, 0].float())                             # position 0 of every row
    t5.calls.clear()
    empty = fe.masked_encode_prompt("cat")                                        # 1 word + end token: n = 2, n_real = 0
    assert empty.shape == (0, 8) and t5.calls == []
    long = fe.masked_ids(" ".join(["w%d" % i for i in range(400)]))
    assert long.shape == (254, 256)


def test_front_end_negative_space_and_encode_prompt():
    t5, tok = _StubT5(), O.FakeT5Tokenizer(vocab_size=512)
    fe = SD3TextFrontEnd(t5, tok, _clip)
    ns = fe.encode_negative_prompt_space(["Nudity", "Sexual Acts"])
    (seen, mask), = t5.calls
    assert seen.shape == (2, 256) and mask is not None and mask.sum(1).tolist() == [2, 3] and ns.shape == (2, 8)
    assert torch.equal(mask, (seen != 0).long())
    t5.calls.clear()
    pe, npe, pp, npp = fe.encode_prompt(prompt=["a cat", "a dog on a mat"], negative_prompt=["x y", "x y"])
    assert [c[1] for c in t5.calls] == [None, None] and all(c[0].shape == (2, 256) for c in t5.calls)
    assert pe.shape == npe.shape == (2, 77 + 256, 8) and pp.shape == npp.shape == (2, 5)
    assert torch.all(pe[:, :77, :6] == 7.0) and torch.all(pe[:, :77, 6:] == 0.0)      # CLIP rows first, zero-padded to d_model
    assert torch.equal(pe[:, 77:, 0], t5.calls[0][0].float() + 1000.0 * torch.arange(256)[None])
    assert torch.equal(npe[:, 77:, 0], t5.calls[1][0].float() + 1000.0 * torch.arange(256)[None])
    with pytest.raises(sda.SdnError):
        fe.encode_prompt(prompt=["a", "b"], negative_prompt=["x"])


XXL = dict(architectures=["T5EncoderModel"], d_ff=10240, d_kv=64, d_model=4096, dense_act_fn="gelu_new", feed_forward_proj="gated-gelu",
           is_gated_act=True, is_encoder_decoder=True, layer_norm_epsilon=1e-6, num_heads=64, num_layers=24,
           relative_attention_max_distance=128, relative_attention_num_buckets=32, vocab_size=32128, model_type="t5")


def test_t5_kwargs_accepts_xxl_and_refuses_the_rest():
    from safe_denoiser_amd.t5 import T5_XXL_CONFIG
    assert checkpoint.t5_kwargs(XXL) == T5_XXL_CONFIG
    for bad in (dict(feed_forward_proj="relu"), dict(d_kv=128), dict(architectures=["T5ForConditionalGeneration"]),
                dict(is_decoder=True), dict(dense_act_fn="relu")):
        with pytest.raises(NotImplementedError):
            checkpoint.t5_kwargs({**XXL, **bad})


def test_sharded_safetensors_directory_loads(tmp_path):
    from safetensors.torch import save_file
    a = {"encoder.block.0.w": torch.randn(3, 4), "shared.weight": torch.randn(5, 2)}
    b = {"encoder.block.1.w": torch.randn(3, 4)}
    save_file(a, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file(b, str(tmp_path / "model-00002-of-00002.safetensors"))
    wm = {**{k: "model-00001-of-00002.safetensors" for k in a}, **{k: "model-00002-of-00002.safetensors" for k in b}}
    (tmp_path / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": wm}))
    sd = checkpoint.load_weights(str(tmp_path))
    assert sorted(sd) == sorted({**a, **b}) and all(torch.equal(sd[k], v) for k, v in {**a, **b}.items())
    os.remove(tmp_path / "model-00002-of-00002.safetensors")
    with pytest.raises(FileNotFoundError):
        checkpoint.load_weights(str(tmp_path))


def _cfg(**kw):
    base = dict(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=2, num_buckets=32, max_distance=128, eps=1e-6, dtype=0)
    base.update(kw)
    return _lib.T5Config(**base)


def test_t5_plan_manifest_and_host_argument_checks():
    lib = sda.lib()
    h = C.c_void_p()
    for bad in (dict(d_kv=128), dict(dtype=2), dict(dtype=3), dict(d_model=100), dict(num_buckets=30), dict(num_layers=0)):
        assert lib.sdn_t5_create(C.byref(_cfg(**bad)), C.byref(h)) == -1, bad
    assert lib.sdn_t5_create(None, C.byref(h)) == -1
    assert lib.sdn_t5_create(C.byref(_cfg(num_heads=3)), C.byref(h)) == 0         # num_heads * 64 need not equal d_model
    lib.sdn_unet_destroy(h)
    m = T5EncoderModel(dtype=torch.float16, **{k: CFG[k] for k in CFG})
    names = {p["name"] for p in m.manifest}
    sd = {k[len("encoder."):]: v for k, v in O.golden_state_dict(G).items()}
    assert names == set(sd)                                                        # exactly transformers' keys, minus `encoder.`
    assert all(tuple(sd[k].shape) == s for k, s in m.state_dict_shapes().items())
    h = m._h
    for n in (1, 513):
        assert lib.sdn_t5_workspace_bytes(h, 1, n) == 0
        assert lib.sdn_t5_forward(h, 0x1000, 0x2000, None, n, 0x3000, 1, 0x4000, 1 << 30, None) == -1
    assert lib.sdn_t5_forward(h, None, 0x2000, None, 16, 0x3000, 1, 0x4000, 1 << 30, None) == -1
    assert lib.sdn_t5_forward(h, 0x1000, None, None, 16, 0x3000, 1, 0x4000, 1 << 30, None) == -1
    assert lib.sdn_t5_forward(h, 0x1000, 0x2000, None, 16, 0x3000, 1, 0x4000, 16, None) == -3      # workspace too small
    assert 0 < lib.sdn_t5_workspace_bytes(h, 3, 13) < lib.sdn_t5_workspace_bytes(h, 3, 256) <= lib.sdn_unet_workspace_bytes(h, 3)
    assert lib.sdn_clip_forward(h, 0x1000, 0x2000, None, 0x3000, 1, 0x4000, 1 << 30, None) == -1   # not a CLIP handle
    assert lib.sdn_t5_flops(h, 2, 513, None) == 0.0 and lib.sdn_unet_flops(h, 2, None) == lib.sdn_t5_flops(h, 2, 512, None)
    lib.sdn_unet_set_split_k(h, 1)                                              # refused on a T5 handle: the plans stand
    total, attn = m.flops(2, 256)
    rows, d, i, f = 512, 128, 128, 256
    assert total == 2 * (2.0 * rows * d * (3 * i + i + 3 * f)) + attn and attn == 2 * 4.0 * 2 * 2 * 256 * 256 * 64
    # the packed layout: value (wi_1) / gate (wi_0) row blocks of 16 interleaved, as SDN_ACT_GEGLU* reads them
    buf = m.pack_state_dict(O.golden_state_dict(G))
    p1 = next(p for p in m.manifest if p["name"] == "block.0.layer.1.DenseReluDense.wi_1.weight")
    p0 = next(p for p in m.manifest if p["name"] == "block.0.layer.1.DenseReluDense.wi_0.weight")
    assert p0["offset"] == p1["offset"] + 16 * 128 * 2
    pair = buf[p1["offset"]:p1["offset"] + 2 * 256 * 128 * 2].view(torch.float16).view(16, 2, 16, 128)
    assert torch.equal(pair[:, 0].reshape(256, 128), sd["block.0.layer.1.DenseReluDense.wi_1.weight"].half())
    assert torch.equal(pair[:, 1].reshape(256, 128), sd["block.0.layer.1.DenseReluDense.wi_0.weight"].half())
    with pytest.raises(sda.SdnError):
        m(torch.zeros(1, 1, dtype=torch.long))
    with pytest.raises(sda.SdnError):
        m(torch.zeros(1, 513, dtype=torch.long))
    with pytest.raises(sda.SdnError):
        m(torch.full((1, 8), 512, dtype=torch.long))                               # id outside the vocabulary (CPU tensor)
    with pytest.raises(sda.SdnError):
        T5EncoderModel(dtype=torch.float32)


def test_new_operators_reject_bad_arguments_on_host():
    lib = sda.lib()
    A, B_, Cc, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    assert lib.sdn_rmsnorm(0, None, 1, 4, 128, 1e-6, B_, Cc, None) == -1
    assert lib.sdn_rmsnorm(0, A, 1, 4, 130, 1e-6, B_, Cc, None) == -1            # c % 4
    assert lib.sdn_rmsnorm(2, A, 1, 4, 128, 1e-6, B_, Cc, None) == -1            # dtype
    assert lib.sdn_rmsnorm(0, A + 4, 1, 4, 128, 1e-6, B_, Cc, None) == -1        # misaligned
    assert lib.sdn_rmsnorm(0, A, 1, 0, 128, 1e-6, B_, Cc, None) == 0             # zero rows: a no-op
    assert lib.sdn_embed_tokens(0, None, B_, 4, 128, 512, Cc, None) == -1
    assert lib.sdn_embed_tokens(0, A, B_, 4, 127, 512, Cc, None) == -1
    assert lib.sdn_t5_relative_bias(0, None, 32, 128, 2, 16, Cc, None) == -1
    for n in (1, 513):
        assert lib.sdn_t5_relative_bias(0, A, 32, 128, 2, n, Cc, None) == -1
        assert lib.sdn_bias_attention(0, A, B_, Cc, D, E, None, 1, 2, n, 64, 384, 384, 384, 128, 1.0, None) == -1
    assert lib.sdn_bias_attention(0, A, B_, Cc, D, None, None, 1, 2, 16, 64, 384, 384, 384, 128, 1.0, None) == -1    # no bias
    assert lib.sdn_bias_attention(0, A, B_, Cc, D, E, None, 1, 2, 16, 40, 384, 384, 384, 128, 1.0, None) == -1       # head dim
    assert lib.sdn_bias_attention(0, None, B_, Cc, D, E, None, 1, 2, 16, 64, 384, 384, 384, 128, 1.0, None) == -1
    assert lib.sdn_bias_attention(2, A, B_, Cc, D, E, None, 1, 2, 16, 64, 384, 384, 384, 128, 1.0, None) == -1
    assert lib.sdn_t5_bucket(3, 30, 128) == -1
    # the new descriptor codes of the GEMM: gated tanh-GELU takes no residual; the f32-residual form takes no activation
    d = _lib.GemmDesc(M=128, N=256, K=128, act=5)
    assert lib.sdn_gemm_bf16(C.byref(d), A, None, B_, None, None, None, Cc, D, None) == -1
    d = _lib.GemmDesc(M=128, N=256, K=128, act=3, out_kind=1, f32_stream=1)
    assert lib.sdn_gemm_f16(C.byref(d), A, None, B_, None, None, None, Cc, D, None) == -1
    d = _lib.GemmDesc(M=128, N=256, K=128, f32_stream=1)                         # needs out_kind = SDN_OUT_F32
    assert lib.sdn_gemm_bf16(C.byref(d), A, None, B_, None, None, None, Cc, D, None) == -1
    d = _lib.GemmDesc(M=128, N=256, K=128, out_kind=1, f32_stream=1, x3_out=1)
    assert lib.sdn_gemm_bf16(C.byref(d), A, None, B_, None, None, None, Cc, D, None) == -1
    d = _lib.GemmDesc(M=128, N=256, K=128, x3_out=6)
    assert lib.sdn_gemm_bf16(C.byref(d), A, None, B_, None, None, None, Cc, D, None) == -1
    d = _lib.GemmDesc(M=128, N=256, K=128, act=6)
    assert lib.sdn_gemm_bf16(C.byref(d), A, None, B_, None, None, None, None, D, None) == -1
