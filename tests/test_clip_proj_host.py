"""Host-side checks of the projected CLIP text encoders (SD-v3 text_encoder / text_encoder_2): the torch oracle against the
transformers fixture, the plan's manifest for the real CLIP-L and bigG configs, argument validation of the new C entry points,
checkpoint.clip_projection_kwargs, and SD3TextFrontEnd's argument rules and id construction with stub encoders.  No GPU."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint
from safe_denoiser_amd.clip import ACT_CODES, CLIPTextModelWithProjection
from safe_denoiser_amd.text_sd3 import SD3TextFrontEnd
from tests_support import clip_proj_oracle as O
from tests_support.t5_oracle import FakeT5Tokenizer

G = O.load_golden()


@pytest.mark.parametrize("arm", O.ARMS)
def test_oracle_reproduces_the_fixture(arm):
    cfg = G[f"{arm}/cfg"]
    out = O.clip_text_with_projection(O.golden_state_dict(G, arm), torch.from_numpy(G[f"{arm}/ids"]),
                                      num_heads=cfg["num_attention_heads"], hidden_act=cfg["hidden_act"], eos_token_id=cfg["eos_token_id"])
    assert len(out.hidden_states) == cfg["num_hidden_layers"] + 1 and cfg["num_hidden_layers"] >= 3
    errs = {"h2": O.rel_l2(out.hidden_states[-2], torch.from_numpy(G[f"{arm}/h2"])),
            "h3": O.rel_l2(out.hidden_states[-3], torch.from_numpy(G[f"{arm}/h3"])),
            "text_embeds": O.rel_l2(out.text_embeds, torch.from_numpy(G[f"{arm}/text_embeds"]))}
    print(arm, errs)
    assert max(errs.values()) <= 1e-5                          # fp32 summation order and nothing else (the T5 host test's bound)
    assert out.positions.tolist() == G[f"{arm}/positions"].tolist()


def test_fixture_arms_cover_what_they_should():
    a, b = G["a/cfg"], G["b/cfg"]
    assert a["hidden_act"] == "quick_gelu" and a["eos_token_id"] == 2 and a["projection_dim"] != a["hidden_size"]
    assert b["hidden_act"] == "gelu" and b["eos_token_id"] != 2 and b["pad_token_id"] > b["eos_token_id"]
    ids_b = torch.from_numpy(G["b/ids"])
    # the two pooling rules disagree on arm b, and one of its sequences holds two end tokens
    assert (O.pool_positions(ids_b, 2) != O.pool_positions(ids_b, b["eos_token_id"])).all()
    assert int((ids_b == b["eos_token_id"]).sum(1).max()) >= 2
    # an applied final_layer_norm would show: the tapped state is far from its normed self
    for arm in O.ARMS:
        h2 = torch.from_numpy(G[f"{arm}/h2"])
        assert O.rel_l2(O.final_norm(O.golden_state_dict(G, arm), h2), h2) > 0.2


@pytest.mark.parametrize("name,cfg", [("clip_l", O.CLIP_L_CONFIG), ("big_g", O.CLIP_G_CONFIG)])
def test_manifest_of_the_real_configs(name, cfg):
    kw = checkpoint.clip_projection_kwargs(dict(cfg, architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model"))
    m = CLIPTextModelWithProjection(dtype=torch.float16, **kw)
    want = O.expected_state_dict_shapes(cfg)
    assert m.state_dict_shapes() == want                       # CLIPTextModelWithProjection.state_dict()'s keys minus `text_model.`
    assert m.config.hidden_act == cfg["hidden_act"] and m.hidden_tap == 2
    total, attn = m.flops(2)
    c, i, L, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["projection_dim"]
    assert attn == L * 4.0 * 2 * cfg["num_attention_heads"] * 77 * 77 * 64
    assert total == L * 2.0 * 154 * (4 * c * c + 2 * c * i) + 2.0 * 2 * p * c + attn


def test_manifest_of_the_fixture_equals_transformers_keys():
    for arm in O.ARMS:
        cfg = G[f"{arm}/cfg"]
        sd = O.golden_state_dict(G, arm)
        m = CLIPTextModelWithProjection(**checkpoint.clip_projection_kwargs(cfg))
        assert set(m.state_dict_shapes()) == set(O.canonical(sd)) and all(k.startswith("text_model.") or k == "text_projection.weight" for k in sd)
        assert all(tuple(O.canonical(sd)[k].shape) == s for k, s in m.state_dict_shapes().items())
        buf = m.pack_state_dict(sd)                            # prefixed keys are accepted
        p = next(q for q in m.manifest if q["name"] == "text_projection.weight")
        got = buf[p["offset"]:p["offset"] + 2 * p["rows"] * p["cols"]].view(torch.bfloat16).view(p["rows"], p["cols"])
        assert torch.equal(got, sd["text_projection.weight"].bfloat16())


def _cfg(**kw):
    base = dict(vocab_size=128, hidden_size=128, intermediate_size=128, num_layers=3, num_heads=2, max_position_embeddings=77, dtype=0,
                projection_dim=64, act=4, eos_token_id=2, hidden_tap=2)
    base.update(kw)
    return _lib.ClipProjConfig(**base)


def test_create_and_forward_reject_bad_arguments_on_host():
    lib = sda.lib()
    h = C.c_void_p()
    for bad in (dict(num_heads=3), dict(hidden_size=192, num_heads=3), dict(hidden_tap=0), dict(hidden_tap=4), dict(act=0), dict(act=3),
                dict(act=6), dict(act=2), dict(dtype=4), dict(projection_dim=40), dict(hidden_size=1408, num_heads=22), dict(num_layers=0),
                dict(eos_token_id=-1)):
        assert lib.sdn_clip_proj_create(C.byref(_cfg(**bad)), C.byref(h)) == -1, bad
    assert lib.sdn_clip_proj_create(None, C.byref(h)) == -1
    for ok in (dict(), dict(act=7, hidden_tap=3, dtype=3), dict(hidden_size=1280, num_heads=20, intermediate_size=5120, act=7, dtype=1),
               dict(hidden_tap=1, dtype=2)):
        assert lib.sdn_clip_proj_create(C.byref(_cfg(**ok)), C.byref(h)) == 0, ok
        lib.sdn_unet_destroy(h)
    assert lib.sdn_clip_proj_create(C.byref(_cfg()), C.byref(h)) == 0
    W, I, H, E, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    fwd = lambda hh=H, hbs=77 * 128, hrs=128, ee=E, ers=64, ws=1 << 30, hd=h: lib.sdn_clip_proj_forward(hd, W, I, hh, hbs, hrs, ee, ers, 1, WS, ws, None)
    assert fwd(hh=None) == -1 and fwd(ee=None) == -1
    assert fwd(hrs=120) == -1 and fwd(hrs=132) == -1            # narrower than the hidden size; not a multiple of 8
    assert fwd(hbs=76 * 128) == -1                              # sequences would overlap
    assert fwd(ers=56) == -1 and fwd(ers=68) == -1
    assert fwd(hh=H + 8) == -1 and fwd(ee=E + 2) == -1          # misaligned
    assert fwd(ws=16) == -3                                     # workspace too small
    assert lib.sdn_clip_forward(h, W, I, None, H, 1, WS, 1 << 30, None) == -1      # a projected handle is not a CLIPTextModel handle
    lib.sdn_unet_set_split_k(h, 1)                              # refused on this handle: the plans stand
    assert 0 < lib.sdn_unet_workspace_bytes(h, 2) < lib.sdn_unet_workspace_bytes(h, 8)
    lib.sdn_unet_destroy(h)
    plain = C.c_void_p()
    c = _lib.ClipConfig(vocab_size=128, hidden_size=128, intermediate_size=128, num_layers=2, num_heads=2, max_position_embeddings=77, dtype=0)
    assert lib.sdn_clip_create(C.byref(c), C.byref(plain)) == 0
    assert fwd(hd=plain) == -1                                  # ... and the other way round
    lib.sdn_unet_destroy(plain)
    c.hidden_size, c.num_heads = 1280, 20
    assert lib.sdn_clip_create(C.byref(c), C.byref(plain)) == -1                    # the plain CLIP plan's ceiling stands where it was


def test_new_operators_reject_bad_arguments_on_host():
    lib = sda.lib()
    A, B_, Cc, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    eos = lambda dtype=0, ids=A, x=B_, hidden=128, out=E, seq=77, vocab=128: lib.sdn_clip_eos_rows(dtype, ids, x, Cc, D, 2, seq, hidden, vocab, 2, 1e-5, out, None, None)
    assert eos(ids=None) == -1 and eos(x=None) == -1 and eos(out=None) == -1
    assert eos(dtype=3) == -1 and eos(hidden=130) == -1 and eos(seq=0) == -1 and eos(vocab=0) == -1
    assert eos(dtype=2, x=B_ + 8) == -1 and eos(x=B_ + 4) == -1
    assert lib.sdn_clip_eos_rows(0, A, B_, Cc, D, 0, 77, 128, 128, 2, 1e-5, E, None, None) == 0          # zero sequences: a no-op
    cp = lambda src=A, cols=128, eb=2, dst=B_, bs=77 * 256, rs=256, rows=77: lib.sdn_copy_rows_strided(src, 2, rows, cols, eb, dst, bs, rs, None)
    assert cp(src=None) == -1 and cp(dst=None) == -1 and cp(eb=3) == -1
    assert cp(cols=132) == -1                                   # 264-byte rows: not whole 16-byte chunks
    assert cp(rs=120) == -1 and cp(rs=260) == -1 and cp(bs=76 * 256) == -1 and cp(dst=B_ + 8) == -1
    assert lib.sdn_copy_rows_strided(A, 0, 77, 128, 2, B_, 77 * 256, 256, None) == 0
    # SDN_ACT_GELU on the 16-bit GEMMs: the lean staged epilogue only
    for extra, args in ((dict(out_kind=1), {}), (dict(n_valid=192), {}), (dict(split_k=2), {}), (dict(x3_out=1), {}), ({}, dict(residual=Cc)),
                        ({}, dict(rowgate=Cc))):
        d = _lib.GemmDesc(M=128, N=256, K=128, act=7, rows_per_batch=128, **extra)
        assert lib.sdn_gemm_f16(C.byref(d), A, None, B_, None, None, args.get("rowgate"), args.get("residual"), D, None) == -1, (extra, args)
    for act in (5, 6, 8):                                       # the f32-storage GEMMs know 0 .. 4 and 7
        d = _lib.GemmDesc(M=128, N=256, K=128, act=act)
        assert lib.sdn_gemm_f32(C.byref(d), A, None, B_, None, None, None, None, D, None) == -1
        assert lib.sdn_gemm_x3(C.byref(d), A, None, B_, None, None, None, None, D, None) == -1


L_CFG = dict(O.CLIP_L_CONFIG, architectures=["CLIPTextModelWithProjection"], layer_norm_eps=1e-5, attention_dropout=0.0, model_type="clip_text_model")


def test_clip_projection_kwargs_accepts_and_refuses():
    assert checkpoint.clip_projection_kwargs(L_CFG) == O.CLIP_L_CONFIG
    assert checkpoint.clip_projection_kwargs(dict(O.CLIP_G_CONFIG)) == O.CLIP_G_CONFIG
    assert set(ACT_CODES) == {"quick_gelu", "gelu"}
    for bad in (dict(hidden_act="gelu_new"), dict(hidden_act="relu"), dict(architectures=["CLIPTextModel"]), dict(projection_dim=None),
                dict(eos_token_id=None), dict(layer_norm_eps=1e-6), dict(num_attention_heads=8), dict(attention_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            checkpoint.clip_projection_kwargs({**L_CFG, **bad})
    no_proj = dict(L_CFG); del no_proj["projection_dim"]
    with pytest.raises(NotImplementedError):
        checkpoint.clip_projection_kwargs(no_proj)
    with pytest.raises(NotImplementedError):                    # the SD-v1.4 helper keeps refusing what it refused
        checkpoint.clip_kwargs(dict(O.CLIP_G_CONFIG))
    with pytest.raises(sda.SdnError):
        CLIPTextModelWithProjection(hidden_act="relu")
    with pytest.raises(sda.SdnError):
        CLIPTextModelWithProjection(clip_skip=-1)
    with pytest.raises(sda.SdnError):
        CLIPTextModelWithProjection(clip_skip=11)               # hidden_tap 13 of a 12-layer encoder
    assert CLIPTextModelWithProjection(clip_skip=1).hidden_tap == 3


def test_hidden_states_indexing_names_what_was_built():
    from safe_denoiser_amd.clip import TextEncoderProjOutput, _TappedHiddenStates
    t, e = torch.zeros(1, 77, 8), torch.ones(1, 4)
    out = TextEncoderProjOutput(e, _TappedHiddenStates(t, 3, 12))
    assert out[0] is e and out.text_embeds is e and out.hidden_states[-3] is t and out.hidden_states[10] is t and len(out.hidden_states) == 13
    for i in (-2, -1, -4, 0, 12):
        with pytest.raises(sda.SdnError, match=r"hidden_states\[-3\]"):
            out.hidden_states[i]


class _StubT5:
    dtype = torch.float32

    def __init__(self, d_model=16):
        self.config = SimpleNamespace(d_model=d_model)

    def __call__(self, input_ids, attention_mask=None):
        b, n = input_ids.shape
        h = input_ids.float()[:, :, None].expand(b, n, self.config.d_model).contiguous()
        return _Out(h)


class _Out(tuple):
    def __new__(cls, h):
        o = super().__new__(cls, (h,))
        o.last_hidden_state = h
        return o


class _StubClip:
    """forward_into writes id + 1000 * column into its slices, so a test can see which slice got what."""
    dtype = torch.float32

    def __init__(self, hidden, proj, tag):
        self.config = SimpleNamespace(hidden_size=hidden, projection_dim=proj)
        self.tag, self.seen = tag, []

    def forward_into(self, ids, hidden, text_embeds):
        self.seen.append(ids.clone())
        hidden.copy_(ids.float()[:, :, None] + 1000.0 * torch.arange(self.config.hidden_size)[None, None] + self.tag)
        text_embeds.fill_(self.tag)


def test_front_end_argument_rules_and_assembly():
    t5, tok3 = _StubT5(), FakeT5Tokenizer(vocab_size=512)
    e1, e2 = _StubClip(4, 3, 0.25), _StubClip(6, 5, 0.5)
    k1, k2 = O.FakeCLIPTokenizer(vocab_size=128), O.FakeCLIPTokenizer(vocab_size=256)
    clip = lambda prompts: (torch.zeros(len(prompts), 77, 4), torch.zeros(len(prompts), 5))
    enc = dict(text_encoder=e1, tokenizer=k1, text_encoder_2=e2, tokenizer_2=k2)
    with pytest.raises(sda.SdnError):
        SD3TextFrontEnd(t5, tok3)                                                   # neither
    with pytest.raises(sda.SdnError):
        SD3TextFrontEnd(t5, tok3, clip, **enc)                                      # both
    for missing in enc:
        with pytest.raises(sda.SdnError):
            SD3TextFrontEnd(t5, tok3, **{k: v for k, v in enc.items() if k != missing})
    with pytest.raises(sda.SdnError):
        SD3TextFrontEnd(t5, tok3, text_encoder=_StubClip(12, 3, 0), tokenizer=k1, text_encoder_2=e2, tokenizer_2=k2)   # 12 + 6 > d_model
    with pytest.raises(TypeError):
        SD3TextFrontEnd(t5, tok3, None, e1, k1, e2, k2)                             # the encoders are keyword-only
    assert SD3TextFrontEnd(t5, tok3, clip).clip_embeds is clip                      # the positional signature stands
    fe = SD3TextFrontEnd(t5, tok3, **enc)
    prompts = ["a cat", "a dog on a mat"]
    pe, npe, pp, npp = fe.encode_prompt(prompt=prompts, negative_prompt="x y")
    assert pe.shape == npe.shape == (2, 77 + 256, 16) and pp.shape == npp.shape == (2, 8)
    for k in (k1, k2):
        assert [c["texts"] for c in k.calls] == [prompts, ["x y", "x y"]]
        assert all(c["padding"] == "max_length" and c["max_length"] == 77 and c["truncation"] for c in k.calls)
    ids1, ids2 = fe.clip_ids(prompts)
    assert torch.equal(e1.seen[0], ids1) and torch.equal(e2.seen[0], ids2) and not torch.equal(ids1, ids2)
    col = 1000.0 * torch.arange(16)[None, None]
    assert torch.equal(pe[:, :77, :4], ids1.float()[:, :, None] + col[..., :4] + 0.25)              # CLIP-L columns first
    assert torch.equal(pe[:, :77, 4:10], ids2.float()[:, :, None] + col[..., :6] + 0.5)
    assert torch.all(pe[:, :77, 10:] == 0)                                                          # zero padding to d_model
    t5_ids = tok3(prompts, padding="max_length", max_length=256, truncation=True).input_ids
    assert torch.equal(pe[:, 77:, 0], t5_ids.float())                                               # T5 rows behind the CLIP rows
    assert torch.all(pp[:, :3] == 0.25) and torch.all(pp[:, 3:] == 0.5)
