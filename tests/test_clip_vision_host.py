"""Host-side checks of the CLIP vision tower and the Q16 classifier: the torch oracle against the transformers fixture, the
Pillow resize restatement against Pillow, the coefficient-table builder against the restatement, the plan's manifest for the real
ViT-L/14 config, the OpenAI key mapping, the Q16 head and load_prompts against the restated SimClassifier, and the configuration
refusals of the C entry points and the Python classes.  No GPU."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint, clip_vision as V
from tests_support import clip_vision_oracle as O

G = O.load_golden()
CFG = G["cfg"]


def test_oracle_reproduces_the_fixture():
    out = O.clip_vision_with_projection(O.golden_state_dict(G), torch.from_numpy(G["pixel_values"]), num_heads=CFG["num_attention_heads"],
                                        hidden_act=CFG["hidden_act"])
    errs = {q: O.rel_l2(getattr(out, q), torch.from_numpy(G[q])) for q in ("last_hidden_state", "image_embeds")}
    print(errs)
    assert tuple(out.last_hidden_state.shape) == (6, 17, 128) and tuple(out.image_embeds.shape) == (6, 64)
    assert max(errs.values()) <= 1e-5                          # fp32 summation order and nothing else (test_clip_proj_host.py's bound)
    # an applied post_layernorm would show in last_hidden_state: the class rows are far from their normed selves
    assert O.rel_l2(out.pooled, out.last_hidden_state[:, 0]) > 0.2


def test_fixture_is_what_the_issue_describes():
    assert G["images"].shape == (6, 80, 80, 3) and G["images"].dtype == np.uint8 and G["resized"].shape == (6, 56, 56, 3)
    assert torch.equal(O.preprocess(torch.from_numpy(G["resized"])), torch.from_numpy(G["pixel_values"]))
    head = O.SimClassifier(torch.from_numpy(G["prompts"]))
    with torch.no_grad():
        sim = head(torch.from_numpy(G["image_embeds"]))
    assert torch.allclose(sim, torch.from_numpy(G["similarity"]), rtol=0, atol=1e-4)
    assert sim.argmax(-1).tolist() == G["labels"].tolist() and 0 < int(G["labels"].sum()) < 6
    assert all(float(G[f"err_{t}_{q}"]) > 0 for t in ("bf16", "f16") for q in ("last_hidden_state", "image_embeds"))


def _test_image(size, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    img = np.stack([127 + 127 * np.sin(x / 7.0), 255.0 * y / size, 127 + 127 * np.cos((x + y) / 11.0)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("src,dst", [(80, 56), (512, 224), (300, 224), (160, 224)])
def test_resize_restatement_equals_pillow_byte_for_byte(src, dst, kind):
    img = _test_image(src, kind, src + dst)
    want = np.asarray(Image.fromarray(img).resize((dst, dst), Image.BICUBIC))
    assert np.array_equal(O.pillow_resize(img, dst), want)


def test_fixture_resized_bytes_are_the_restatements():
    for im, want in zip(G["images"], G["resized"]):
        assert np.array_equal(O.pillow_resize(im, 56), want)


@pytest.mark.parametrize("src,dst", [(80, 56), (512, 224), (300, 224), (160, 224), (1024, 224)])
def test_table_builder_equals_the_restatement(src, dst):
    coeffs, bounds, ksize = V.resize_tables(src, dst)
    assert coeffs.shape == (dst, ksize) and bounds.shape == (dst, 2) and coeffs.dtype == bounds.dtype == np.int32
    tables = O.pillow_tables(src, dst)
    assert len(tables) == dst
    for i, (xmin, k) in enumerate(tables):
        assert bounds[i, 0] == xmin and bounds[i, 1] == len(k) <= ksize
        assert coeffs[i, :len(k)].tolist() == k.tolist() and not coeffs[i, len(k):].any()
        assert 0 <= xmin and xmin + len(k) <= src
    assert abs(int(coeffs.sum(1).min()) - (1 << 22)) <= ksize and abs(int(coeffs.sum(1).max()) - (1 << 22)) <= ksize


def test_manifest_of_vit_l14_equals_transformers_on_the_meta_device():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    with torch.device("meta"):
        ref = CLIPVisionModelWithProjection(CLIPVisionConfig(**O.VIT_L14_CONFIG))
    want = {k: tuple(v.shape) for k, v in O.canonical(ref.state_dict()).items()}
    m = V.CLIPVisionModelWithProjection(dtype=torch.float16, **O.VIT_L14_CONFIG)
    assert m.state_dict_shapes() == want == O.expected_state_dict_shapes(O.VIT_L14_CONFIG)
    assert V.VIT_L14_CONFIG == O.VIT_L14_CONFIG and m.num_tokens == 257 and m._kpad() == 640
    total, attn = m.flops(2)
    c, i, L, n = 1024, 4096, 24, 257
    assert attn == L * 4.0 * 2 * 16 * n * n * 64
    assert total == L * 2.0 * 2 * n * (4 * c * c + 2 * c * i) + 2.0 * 2 * 256 * c * 640 + 2.0 * 2 * 768 * c + attn
    assert 0.14e12 < total / 2 < 0.18e12                       # "about 0.16 TFLOP per image"
    assert 0 < _lib.lib().sdn_unet_workspace_bytes(m._h, 2) < _lib.lib().sdn_unet_workspace_bytes(m._h, 8)
    assert m.max_batch == ((1 << 31) - 4096) // (2 * 4096 * 257)


def test_pack_places_the_patch_weight_zero_padded():
    sd = O.golden_state_dict(G)
    m = V.CLIPVisionModelWithProjection(dtype=torch.bfloat16, **checkpoint.clip_vision_kwargs(CFG))
    assert set(m.state_dict_shapes()) == set(O.canonical(sd))
    assert all(tuple(O.canonical(sd)[k].shape) == s for k, s in m.state_dict_shapes().items())
    buf = m.pack_state_dict(sd)                                # prefixed keys are accepted
    assert torch.equal(buf, m.pack_state_dict(O.canonical(sd)))
    p = next(q for q in m.manifest if q["name"] == m.PATCH_KEY)
    assert (p["rows"], p["cols"]) == (128, 640)
    got = buf[p["offset"]:p["offset"] + 2 * 128 * 640].view(torch.bfloat16).view(128, 640)
    assert torch.equal(got[:, :588], sd["vision_model.embeddings.patch_embedding.weight"].reshape(128, 588).bfloat16())
    assert not got[:, 588:].float().any()
    q = next(q for q in m.manifest if q["name"] == "embeddings.class_embedding")
    assert torch.equal(buf[q["offset"]:q["offset"] + 4 * 128].view(torch.float32), sd["vision_model.embeddings.class_embedding"])
    with pytest.raises(KeyError):
        m.pack_state_dict({k: v for k, v in sd.items() if "post_layernorm" not in k})
    with pytest.raises(sda.SdnError):
        m.pack_state_dict({**sd, "visual_projection.weight": sd["visual_projection.weight"].t()})


def test_openai_form_maps_back_to_the_same_tensors():
    sd = O.canonical(O.golden_state_dict(G))
    back = V.convert_openai_state_dict(O.to_openai_state_dict(sd))
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    with pytest.raises(KeyError):
        V.convert_openai_state_dict({"visual.conv1.weight": sd["embeddings.patch_embedding.weight"]})


def test_q16_head_and_load_prompts_agree_with_sim_classifier(tmp_path):
    prompts = torch.from_numpy(G["prompts"])
    emb = torch.from_numpy(G["image_embeds"]).to(torch.float16)
    with torch.no_grad():
        want = O.SimClassifier(prompts)(emb.float())
    assert torch.equal(V.q16_similarity(emb, prompts), want)
    one = V.q16_similarity(emb[:1], prompts)
    assert tuple(one.shape) == (1, 2)                          # the head keeps the batch axis; __call__ squeezes as the reference does
    torch.save(prompts, tmp_path / "prompts.pt")
    with open(tmp_path / "prompts.p", "wb") as f:
        pickle.dump(prompts.numpy(), f)
    a, b = V.Q16Classifier.load_prompts(str(tmp_path / "prompts.pt")), V.Q16Classifier.load_prompts(str(tmp_path / "prompts.p"))
    assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, prompts.to(torch.float16).float())
    vision = V.CLIPVisionModelWithProjection(**checkpoint.clip_vision_kwargs(CFG))
    assert torch.equal(V.Q16Classifier(vision, G["prompts"]).prompts, prompts)        # an ndarray is accepted
    with pytest.raises(sda.SdnError):
        V.Q16Classifier(vision, prompts[:, :32])
    with pytest.raises(sda.SdnError):
        V.Q16Classifier(vision, torch.zeros(3, 64))


def _cfg(**kw):
    base = dict(image_size=56, patch_size=14, hidden_size=128, intermediate_size=128, num_layers=2, num_heads=2, projection_dim=64, act=4, dtype=0)
    base.update(kw)
    return _lib.ClipVisionConfig(**base)


def test_create_and_forward_reject_bad_arguments_on_host():
    lib = sda.lib()
    h = C.c_void_p()
    for bad in (dict(num_heads=3), dict(hidden_size=192, num_heads=3), dict(act=0), dict(act=2), dict(act=3), dict(dtype=2), dict(dtype=3),
                dict(dtype=-1), dict(projection_dim=40), dict(image_size=60), dict(patch_size=0), dict(num_layers=0), dict(intermediate_size=96),
                dict(hidden_size=1408, num_heads=22)):
        assert lib.sdn_clip_vision_create(C.byref(_cfg(**bad)), C.byref(h)) == -1, bad
    assert lib.sdn_clip_vision_create(None, C.byref(h)) == -1
    for ok in (dict(), dict(act=7, dtype=1), dict(image_size=224, hidden_size=1024, num_heads=16, intermediate_size=4096, num_layers=24,
                                                 projection_dim=768, dtype=1)):
        assert lib.sdn_clip_vision_create(C.byref(_cfg(**ok)), C.byref(h)) == 0, ok
        lib.sdn_unet_destroy(h)
    assert lib.sdn_clip_vision_create(C.byref(_cfg()), C.byref(h)) == 0
    W, X, Hs, E, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    fwd = lambda x=X, hs=Hs, e=E, ws=1 << 30, hd=h, w=W: lib.sdn_clip_vision_forward(hd, w, x, hs, e, 1, WS, ws, None)
    assert fwd(e=None) == -1 and fwd(x=None) == -1 and fwd(w=None) == -1
    assert fwd(x=X + 4) == -1 and fwd(hs=Hs + 8) == -1 and fwd(e=E + 2) == -1        # misaligned
    assert fwd(ws=0) == -3 and fwd(hs=None, ws=0) == -3                                # last_hidden_state is nullable
    lib.sdn_unet_set_split_k(h, 1)                                                      # refused on this handle: the plans stand
    assert 0 < lib.sdn_unet_workspace_bytes(h, 2) < lib.sdn_unet_workspace_bytes(h, 8)
    assert lib.sdn_t5_workspace_bytes(h, 1, 16) == 0
    lib.sdn_unet_destroy(h)


def test_new_operators_reject_bad_arguments_on_host():
    lib = sda.lib()
    A, B_, Cc, D, E, F_ = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    pr = lambda dtype=0, pix=A, S=56, p=14, kpad=640, out=B_: lib.sdn_clip_patch_rows(dtype, pix, 2, S, p, kpad, out, None)
    assert pr(pix=None) == -1 and pr(out=None) == -1 and pr(dtype=2) == -1 and pr(S=60) == -1 and pr(kpad=584) == -1 and pr(kpad=590) == -1
    assert pr(out=B_ + 8) == -1 and pr(p=0) == -1
    assert lib.sdn_clip_patch_rows(0, A, 0, 56, 14, 640, B_, None) == 0
    em = lambda dtype=0, proj=A, cls=B_, pos=Cc, g=D, b=E, out=F_, n=17, c=128: lib.sdn_clip_vision_embed(dtype, proj, cls, pos, g, b, 2, n, c, 1e-5, out, None)
    assert em(proj=None) == -1 and em(cls=None) == -1 and em(pos=None) == -1 and em(out=None) == -1 and em(dtype=2) == -1
    assert em(c=130) == -1 and em(n=1) == -1 and em(proj=A + 4) == -1 and em(cls=B_ + 8) == -1
    assert lib.sdn_clip_vision_embed(0, A, B_, Cc, D, E, 0, 17, 128, 1e-5, F_, None) == 0
    cr = lambda dtype=0, x=A, g=D, b=E, out=F_, n=17, c=128: lib.sdn_clip_class_rows(dtype, x, g, b, 2, n, c, 1e-5, out, None)
    assert cr(x=None) == -1 and cr(out=None) == -1 and cr(dtype=2) == -1 and cr(c=126) == -1 and cr(n=0) == -1 and cr(g=D + 4) == -1
    assert lib.sdn_clip_class_rows(0, A, D, E, 0, 17, 128, 1e-5, F_, None) == 0
    rs = lambda src=A, S=80, T=56, co=B_, bo=Cc, ks=7, tmp=D, out=E: lib.sdn_image_resize_u8(src, 2, S, T, co, bo, ks, tmp, out, None)
    assert rs(src=None) == -1 and rs(co=None) == -1 and rs(bo=None) == -1 and rs(tmp=None) == -1 and rs(out=None) == -1
    assert rs(S=0) == -1 and rs(T=0) == -1 and rs(ks=0) == -1 and rs(co=B_ + 2) == -1
    assert lib.sdn_image_resize_u8(A, 0, 80, 56, B_, Cc, 7, D, E, None) == 0
    nz = lambda src=A, T=56, std=0.25, out=B_: lib.sdn_clip_normalize_u8(src, 2, T, 0.5, 0.5, 0.5, std, 0.25, 0.25, out, None)
    assert nz(src=None) == -1 and nz(out=None) == -1 and nz(T=0) == -1 and nz(std=0.0) == -1 and nz(out=B_ + 2) == -1
    assert lib.sdn_clip_normalize_u8(A, 0, 56, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, B_, None) == 0


FULL_CFG = dict(O.VIT_L14_CONFIG, architectures=["CLIPVisionModelWithProjection"], layer_norm_eps=1e-5, attention_dropout=0.0, num_channels=3,
                model_type="clip_vision_model")


def test_clip_vision_kwargs_accepts_and_refuses():
    assert checkpoint.clip_vision_kwargs(FULL_CFG) == O.VIT_L14_CONFIG
    assert checkpoint.clip_vision_kwargs(CFG) == CFG
    whole = dict(architectures=["CLIPModel"], projection_dim=768, text_config=dict(hidden_size=768),
                 vision_config={k: v for k, v in O.VIT_L14_CONFIG.items() if k != "projection_dim"})
    assert checkpoint.clip_vision_kwargs(whole) == O.VIT_L14_CONFIG
    for bad in (dict(hidden_act="relu"), dict(hidden_act="gelu_new"), dict(architectures=["CLIPTextModelWithProjection"]),
                dict(num_attention_heads=8), dict(projection_dim=None), dict(layer_norm_eps=1e-6), dict(attention_dropout=0.1),
                dict(num_channels=1)):
        with pytest.raises(NotImplementedError):
            checkpoint.clip_vision_kwargs({**FULL_CFG, **bad})
    with pytest.raises(sda.SdnError):
        V.CLIPVisionModelWithProjection(hidden_act="relu")
    with pytest.raises(sda.SdnError):
        V.CLIPVisionModelWithProjection(dtype=torch.float32)
    with pytest.raises(sda.SdnError):
        V.CLIPVisionModelWithProjection(hidden_size=1024, num_attention_heads=8)      # head dim 128
    assert sda.CLIPVisionModelWithProjection is V.CLIPVisionModelWithProjection and sda.Q16Classifier is V.Q16Classifier
    assert sda.clip_preprocess is V.clip_preprocess


def test_preprocess_refuses_what_it_does_not_implement():
    with pytest.raises(sda.SdnError):
        V._as_u8_batches(torch.zeros(2, 80, 64, 3, dtype=torch.uint8), "cpu")          # not square
    with pytest.raises(sda.SdnError):
        V._as_u8_batches(torch.zeros(2, 80, 80, 3), "cpu")                              # not uint8
    with pytest.raises(sda.SdnError):
        V._as_u8_batches([Image.new("RGB", (80, 64))], "cpu")
    with pytest.raises(sda.SdnError):
        V._as_u8_batches([np.zeros((8, 8, 3), np.uint8)], "cpu")
    parts = V._as_u8_batches([Image.new("RGB", (8, 8)), Image.new("L", (8, 8)), Image.new("RGB", (16, 16))], "cpu")
    assert [tuple(p.shape) for p in parts] == [(2, 8, 8, 3), (1, 16, 16, 3)]
