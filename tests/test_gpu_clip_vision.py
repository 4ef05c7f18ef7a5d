"""CLIP vision tower and Q16 classifier on the GPU: libsdn's plan against the transformers fixture, every new kernel alone at the
smallest shapes that can break it (Pillow's resize byte for byte, the normalise map, patch rows, the embedding and class-row
LayerNorms against float64, the d = 64 attention at 257 tokens), full-size ViT-L/14 against the torch oracle, the Q16 chain from
uint8 images to labels, handle kinds, and from_pretrained.  Measured distances go to profiles/clip_vision_parity.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint, clip_vision as V
from tests_support import clip_vision_oracle as O
from tests_support import exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "clip_vision_parity.json")
G = O.load_golden()
CFG = G["cfg"]
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"bf16": 0, "f16": 1}
U16 = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}                   # unit roundoff of the storage formats


def record(key, value, bound):
    data = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            data = json.load(f)
    data[key] = {"measured": value, "bound": bound}
    with open(PARITY, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def small(dtype):
    m = V.CLIPVisionModelWithProjection(dtype=dtype, **checkpoint.clip_vision_kwargs(CFG))
    m.load_state_dict(O.golden_state_dict(G))
    return m


def gold(name):
    return torch.from_numpy(G[name])


def guarded_u8(shape, pad=512):
    """(buffer, view): a contiguous uint8 view of `shape` between two bands of 0xA5."""
    n = int(np.prod(shape))
    buf = torch.full((2 * pad + n,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[pad:pad + n].view(*shape)


def bands_intact(buf, view, pad=512):
    return bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + view.numel():] == 0xA5).all())


# ---------------------------------------------------------------------------------------------- 1. engine vs fixture
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_engine_matches_the_transformers_fixture(tag):
    """Bound = 2 x the distance of transformers' own run at that storage width from its fp32 run (recorded in the fixture)."""
    m = small(DT[tag])
    out = m(gold("pixel_values"))
    h, e = out.last_hidden_state, out.image_embeds
    assert out[0] is e and out[1] is h and h.dtype == e.dtype == DT[tag]
    assert tuple(h.shape) == (6, 17, 128) and tuple(e.shape) == (6, 64)
    assert torch.isfinite(h.float()).all() and torch.isfinite(e.float()).all()
    for q, got in (("last_hidden_state", h), ("image_embeds", e)):
        err, bound = O.rel_l2(got.float(), gold(q)), 2.0 * float(G[f"err_{tag}_{q}"])
        print(f"clip vision {tag} {q}: rel L2 {err:.3e} (transformers at this width {bound / 2:.3e}, bound {bound:.3e})")
        record(f"fixture/{tag}/{q}", err, bound)
        assert err <= bound
    # without a last_hidden_state buffer: the same embeddings, bit for bit
    lean = m(gold("pixel_values"), output_hidden_state=False)
    assert lean.last_hidden_state is None and torch.equal(lean.image_embeds, e)


def test_hidden_state_buffer_given_then_withheld_then_given_again():
    """One handle through the C interface: a forward with a last_hidden_state buffer, one without, one with again, every output buffer
    filled with NaN beforehand.  image_embeds are identical across the three and the third hidden state equals the first.  (Without
    a buffer nothing in the plan names the hidden-state operand, so there is no substitute address whose bytes could be checked.)"""
    m = small(torch.float16)
    pv = gold("pixel_values")[:2].cuda().contiguous()
    ws = m._workspace(2, pv.device)
    hid = [torch.full((2, 17, 128), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2)]
    emb = [torch.full((2, 64), float("nan"), dtype=torch.float16, device="cuda") for _ in range(3)]
    for e, h in zip(emb, (hid[0], None, hid[1])):
        assert sda.lib().sdn_clip_vision_forward(m._h, m._weights.data_ptr(), pv.data_ptr(), None if h is None else h.data_ptr(), e.data_ptr(),
                                                 2, ws.data_ptr(), ws.numel(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(emb[0].float()).all() and torch.isfinite(hid[0].float()).all()
    assert torch.equal(emb[1], emb[0]) and torch.equal(emb[2], emb[0]) and torch.equal(hid[1], hid[0])
    want = m(pv)
    assert torch.equal(want.image_embeds, emb[0]) and torch.equal(want.last_hidden_state, hid[0])


# ---------------------------------------------------------------------------------------------- 2. preprocessing
def _images(size, n=2, seed=0):
    rng = np.random.default_rng(seed + size)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    smooth = np.clip(np.stack([127 + 127 * np.sin(x / 7.0), 255.0 * y / size, 127 + 127 * np.cos((x + y) / 11.0)], -1), 0, 255).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (size, size, 3), dtype=np.uint8), smooth][:n])


def _resize_guarded(imgs, dst):
    src = torch.from_numpy(imgs).cuda()
    b, s = src.shape[0], src.shape[1]
    coeffs, bounds, ksize = V.resize_tables(s, dst)
    cg, bg = torch.from_numpy(coeffs).cuda(), torch.from_numpy(bounds).cuda()
    tb, tmp = guarded_u8((b, s, dst, 3))
    ob, out = guarded_u8((b, dst, dst, 3))
    assert sda.lib().sdn_image_resize_u8(src.data_ptr(), b, s, dst, cg.data_ptr(), bg.data_ptr(), ksize, tmp.data_ptr(), out.data_ptr(),
                                         _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bands_intact(tb, tmp) and bands_intact(ob, out)
    return tmp.cpu().numpy(), out.cpu().numpy()


def test_resize_equals_pillow_on_the_fixture_images():
    tmp, out = _resize_guarded(G["images"], 56)
    diff = int((out != G["resized"]).sum())
    print(f"resize 80 -> 56: {diff} differing bytes of {out.size}")
    assert diff == 0
    # the uint8 intermediate is Pillow's horizontal pass (a resize of the width alone)
    want_h = np.stack([np.asarray(Image.fromarray(im).resize((56, 80), Image.BICUBIC)) for im in G["images"]])
    assert np.array_equal(tmp, want_h)
    assert torch.equal(V.resize_u8(torch.from_numpy(G["images"]).cuda(), 56).cpu(), gold("resized"))
    same = torch.from_numpy(G["resized"]).cuda()
    assert torch.equal(V.resize_u8(same, 56), same)              # same size: a copy


@pytest.mark.parametrize("src,dst", [(512, 224), (160, 224)])
def test_resize_equals_the_restatement(src, dst):
    imgs = _images(src)
    _, out = _resize_guarded(imgs, dst)
    want = np.stack([O.pillow_resize(im, dst) for im in imgs])
    diff = int((out != want).sum())
    print(f"resize {src} -> {dst}: {diff} differing bytes of {out.size}")
    assert diff == 0
    assert np.array_equal(out[0], np.asarray(Image.fromarray(imgs[0]).resize((dst, dst), Image.BICUBIC)))


def test_normalize_is_within_one_ulp_of_the_torch_expression():
    u8 = torch.from_numpy(np.concatenate([G["resized"], np.arange(256, dtype=np.uint8).repeat(3 * 49).reshape(4, 56, 56, 3)])).cuda()   # every byte value
    buf, view = X.guarded_like((u8.shape[0], 3, 56, 56), torch.float32, "cuda")
    assert sda.lib().sdn_clip_normalize_u8(u8.data_ptr(), u8.shape[0], 56, *O.CLIP_MEAN, *O.CLIP_STD, view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    # the torch expression on the GPU (true divisions: see O.preprocess) and the same expression on the CPU, where torchvision runs it
    for where, want in (("gpu", O.preprocess(u8)), ("cpu", O.preprocess(u8.cpu()).cuda())):
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        worst = float(((view - want).abs() / ulp).max())
        print(f"normalize vs torch on the {where}: max |error| {worst:.2f} ulp, {int((view != want).sum())} of {want.numel()} values differ")
        assert worst <= 1.0
    assert X.sentinels_intact(buf, view) == 0
    assert torch.equal(V.normalize_u8(u8), view)
    pv = V.clip_preprocess(torch.from_numpy(G["images"]).cuda(), 56)
    assert float(((pv.cpu() - gold("pixel_values")).abs() / (torch.nextafter(gold("pixel_values").abs(), torch.tensor(float("inf"))) - gold("pixel_values").abs())).max()) <= 1.0
    pil = V.clip_preprocess([Image.fromarray(im) for im in G["images"]], 56)
    assert torch.equal(pil, pv)
    with pytest.raises(sda.SdnError):
        V.clip_preprocess(torch.zeros(1, 80, 64, 3, dtype=torch.uint8, device="cuda"), 56)


# ---------------------------------------------------------------------------------------------- 3. patch rows
@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("B,S", [(3, 56), (2, 224)])
def test_patch_rows_are_unfold_and_one_rounding(B, S, tag):
    dt, p, kpad = DT[tag], 14, 640
    g = torch.Generator().manual_seed(S + B)
    pix = (torch.randn(B, 3, S, S, generator=g) * 1.7).cuda()
    P = (S // p) ** 2
    buf, view = X.guarded_like((B * P, kpad), dt, "cuda")
    assert sda.lib().sdn_clip_patch_rows(CODE[tag], pix.data_ptr(), B, S, p, kpad, view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    want = torch.nn.functional.unfold(pix, kernel_size=p, stride=p).transpose(1, 2).reshape(B * P, 3 * p * p).to(dt)
    assert torch.equal(view[:, :588].view(torch.int16), want.view(torch.int16))
    assert not view[:, 588:].view(torch.int16).any()             # exactly zero (+0)
    assert X.sentinels_intact(buf, view) == 0


# ---------------------------------------------------------------------------------------------- 4. the two row LayerNorms
@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("B,n,Cw", [(3, 17, 128), (2, 257, 1024), (2, 5, 1280)])
def test_embed_and_class_rows_against_float64(B, n, Cw, tag):
    dt = DT[tag]
    g = torch.Generator().manual_seed(n + Cw)
    proj = (torch.randn(B, n - 1, Cw, generator=g) * 2 + 0.5).to(dt)
    pos = (0.5 * torch.randn(n, Cw, generator=g)).to(dt)
    cls = 0.7 * torch.randn(Cw, generator=g)
    gam, bet = 0.5 + torch.rand(Cw, generator=g), 0.3 * torch.randn(Cw, generator=g)
    buf, view = X.guarded_like((B, n, Cw), dt, "cuda")
    pg, cg, og, gg, bg = proj.cuda(), cls.cuda(), pos.cuda(), gam.cuda(), bet.cuda()
    assert sda.lib().sdn_clip_vision_embed(CODE[tag], pg.data_ptr(), cg.data_ptr(), og.data_ptr(), gg.data_ptr(), bg.data_ptr(), B, n, Cw, 1e-5,
                                           view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    x = torch.cat([cls.double().expand(B, 1, Cw), proj.double()], dim=1) + pos.double()[None]
    ref = torch.nn.functional.layer_norm(x, (Cw,), gam.double(), bet.double(), 1e-5)
    # one storage rounding of the result + the f32 arithmetic (sum, mean, variance and the affine map: a few 2^-24 of the operands)
    tol = 0.5 * X.ulp(ref, dt) + 2.0 ** -20 * (ref.abs() + bet.double().abs() + 1.0)
    err = (view.cpu().double() - ref).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    assert bool((err[:, 0] <= tol[:, 0]).all()) and bool((err[:, -1] <= tol[:, -1]).all())      # the class row and the last patch row
    assert X.sentinels_intact(buf, view) == 0
    # post_layernorm on the class rows of a stream whose other rows are NaN: only row 0 of each sequence is read
    stream = torch.full((B, n, Cw), float("nan")).to(dt)
    stream[:, 0] = (torch.randn(B, Cw, generator=g) * 3 - 0.4).to(dt)
    cb, cview = X.guarded_like((B, Cw), dt, "cuda")
    sg = stream.cuda()
    assert sda.lib().sdn_clip_class_rows(CODE[tag], sg.data_ptr(), gg.data_ptr(), bg.data_ptr(), B, n, Cw, 1e-5, cview.data_ptr(),
                                         _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    cref = torch.nn.functional.layer_norm(stream[:, 0].double(), (Cw,), gam.double(), bet.double(), 1e-5)
    ctol = 0.5 * X.ulp(cref, dt) + 2.0 ** -20 * (cref.abs() + bet.double().abs() + 1.0)
    cerr = (cview.cpu().double() - cref).abs()
    assert bool((cerr <= ctol).all()), float((cerr / ctol).max())
    assert X.sentinels_intact(cb, cview) == 0


# ---------------------------------------------------------------------------------------------- 5. attention at 257 tokens
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_attention_at_257_tokens_against_float64(tag):
    """n = 257 = 4 x 64 + 1: a one-row query tail and a one-key tail tile, in the fused-qkv layout the plan uses.  Error budget per
    element, with A = softmax-weighted mean of |v| (float64): half an ulp of the stored result; 2 u A for the probabilities entering
    the second matrix product in the 16-bit format (numerator and row sum, worst case); 2^-13 A for the f32 score accumulation over 64
    products and the exponential's evaluation."""
    dt, B, H, n, d = DT[tag], 2, 2, 257, 64
    g = torch.Generator().manual_seed(257)
    qkv = torch.randn(B, n, 3 * H * d, generator=g)
    qkv[..., :H * d] *= 1.5                                        # sharper than uniform, well inside the f16 range
    qkv = qkv.to(dt)
    buf, view = X.guarded_like((B, n, H * d), dt, "cuda")
    qg = X.with_nan_tail(qkv.cuda().view(B * n, 3 * H * d), 8)
    fn = sda.lib().sdn_attention_bf16 if tag == "bf16" else sda.lib().sdn_attention_f16
    es = 2
    assert fn(qg.data_ptr(), qg.data_ptr() + H * d * es, qg.data_ptr() + 2 * H * d * es, view.data_ptr(), B, H, n, n, d, 3 * H * d, 3 * H * d,
              3 * H * d, H * d, d ** -0.5, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    q, k, v = (t.double().view(B, n, H, d).transpose(1, 2) for t in qkv.split(H * d, dim=-1))
    p = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
    ref = (p @ v).transpose(1, 2).reshape(B, n, H * d)
    a = (p @ v.abs()).transpose(1, 2).reshape(B, n, H * d)
    tol = 0.5 * X.ulp(ref, dt) + (2 * U16[tag] + 2.0 ** -13) * a
    err = (view.cpu().double() - ref).abs()
    worst = float((err / tol).max())
    print(f"attention n = 257 {tag}: max err / bound {worst:.3f}")
    record(f"attention_257/{tag}", worst, 1.0)
    assert worst <= 1.0
    assert float((err[:, -1] / tol[:, -1]).max()) <= 1.0          # the tail row
    assert X.sentinels_intact(buf, view) == 0


# ---------------------------------------------------------------------------------------------- 6. full size
def device_state_dict(m, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for name, shape in m.state_dict_shapes().items():
        if name.endswith("class_embedding"):
            sd[name] = 0.3 * torch.randn(shape, generator=g, device="cuda").to(m.dtype).float()
        elif len(shape) == 1:
            norm = "norm" in name
            base = 1.0 if (norm and name.endswith("weight")) else 0.0
            sd[name] = base + (0.2 if norm else 0.1) * (torch.rand(shape, generator=g, device="cuda") - 0.5)
        elif "position_embedding" in name:
            sd[name] = (0.3 * torch.randn(shape, generator=g, device="cuda")).to(m.dtype)
        else:
            fan_in = int(np.prod(shape[1:]))
            amp = (3.0 / fan_in) ** 0.5 * (2.0 if ".q_proj." in name else 1.0)
            sd[name] = ((torch.rand(shape, generator=g, device="cuda") * 2 - 1) * amp).to(m.dtype)
    return sd


@pytest.mark.parametrize("tag", ["f16", "bf16"])
def test_full_size_against_the_oracle_on_the_gpu(tag):
    """ViT-L/14 at 24 layers, synthetic weights, 3 images.  Reference: the tests_support oracle in fp32 on the same 16-bit weights;
    bound: 2 x the distance of the SAME oracle evaluated by torch in that 16-bit dtype (the reference's own loss)."""
    dt = DT[tag]
    m = V.CLIPVisionModelWithProjection(dtype=dt, **O.VIT_L14_CONFIG)
    sd = device_state_dict(m, 11)
    m.load_state_dict(sd)
    pv = V.clip_preprocess(torch.from_numpy(_images(300, 2, 5)).cuda())
    pv = torch.cat([pv, torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(3)).cuda()])
    kw = dict(num_heads=16, hidden_act="quick_gelu")
    with torch.no_grad():
        ref = O.clip_vision_with_projection({k: v.float() for k, v in sd.items()}, pv, **kw)
        low = O.clip_vision_with_projection({k: v.to(dt) for k, v in sd.items()}, pv, **kw)
        out = m(pv)
    assert tuple(out.last_hidden_state.shape) == (3, 257, 1024) and tuple(out.image_embeds.shape) == (3, 768)
    for q in ("last_hidden_state", "image_embeds"):
        got, r, l = getattr(out, q), getattr(ref, q), getattr(low, q)
        assert torch.isfinite(got.float()).all()
        err, bound = O.rel_l2(got.float(), r), 2.0 * O.rel_l2(l.float(), r)
        print(f"ViT-L/14 {tag} {q}: rel L2 vs fp32 oracle {err:.3e} (torch at this width {bound / 2:.3e}, bound {bound:.3e})")
        record(f"full_size/{tag}/{q}", err, bound)
        assert err <= bound


# ---------------------------------------------------------------------------------------------- 7. Q16 through the whole chain
@pytest.mark.parametrize("tag", ["f16", "bf16"])
def test_q16_labels_from_uint8_images(tag):
    vision = small(DT[tag])
    q16 = V.Q16Classifier(vision, gold("prompts"))
    u8 = torch.from_numpy(G["images"]).cuda()
    labels, sim = q16.classify(u8)
    assert tuple(labels.shape) == (6,) and tuple(sim.shape) == (6, 2) and sim.dtype == torch.float32
    print(f"q16 {tag}: similarities {sim.cpu().tolist()} (fp32 fixture {G['similarity'].tolist()})")
    assert labels.cpu().tolist() == G["labels"].tolist()          # all six, none left out
    pil = [Image.fromarray(im) for im in G["images"]]
    for i in (0, 1):
        unsafe, pred = q16([pil[i]], threshold=0.6)
        assert isinstance(unsafe, bool) and isinstance(pred, float)
        assert unsafe == bool(G["labels"][i]) and abs(pred - float(sim[i].max())) <= 0.1 * float((sim[i, 1] - sim[i, 0]).abs())
    unsafe, pred = q16(pil)
    assert unsafe is True and isinstance(pred, np.ndarray) and pred.shape == (6,) and np.array_equal(pred, sim.max(-1)[0].cpu().numpy())
    assert q16(pil[2:5])[0] is False                              # three safe images
    # rows of a batch do not see each other: a permuted batch gives the permuted embeddings, bit for bit
    perm = torch.tensor([4, 0, 5, 2, 1, 3], device="cuda")
    pv = V.clip_preprocess(u8, 56)
    a, b = vision(pv), vision(pv[perm])
    assert torch.equal(b.image_embeds, a.image_embeds[perm]) and torch.equal(b.last_hidden_state, a.last_hidden_state[perm])


# ---------------------------------------------------------------------------------------------- 8. handle kinds
def test_forwards_refuse_each_others_handles():
    import tests.test_abi as ta                                    # its small handle of each existing kind, read and not edited
    lib = sda.lib()
    raw = C.create_string_buffer(8 * 256 + 16)
    base = (C.addressof(raw) + 15) & ~15                           # 16-byte aligned host memory; nothing is dereferenced
    W, Xp, T, P, O_, E, WS = (base + 256 * i for i in range(7))
    vis_fwd = lambda h: lib.sdn_clip_vision_forward(h, W, Xp, O_, E, 1, WS, 0, None)
    others = [lambda h: lib.sdn_unet_forward(h, W, Xp, 500.0, T, O_, 1, WS, 0, None),
              lambda h: lib.sdn_mmdit_forward(h, W, Xp, 500.0, T, P, O_, 1, WS, 0, None),
              lambda h: lib.sdn_vae_decode(h, W, Xp, 1.0, O_, 1, WS, 0, None),
              lambda h: lib.sdn_vae_encode(h, W, Xp, O_, 1, WS, 0, None),
              lambda h: lib.sdn_clip_forward(h, W, Xp, T, O_, 1, WS, 0, None),
              lambda h: lib.sdn_clip_proj_forward(h, W, Xp, O_, 77 * 128, 128, E, 64, 1, WS, 0, None),
              lambda h: lib.sdn_t5_forward(h, W, Xp, T, 16, O_, 1, WS, 0, None)]
    handles = ta._small_handles(lib)
    vh = C.c_void_p()
    c = _lib.ClipVisionConfig(image_size=56, patch_size=14, hidden_size=128, intermediate_size=128, num_layers=2, num_heads=2,
                              projection_dim=64, act=4, dtype=0)
    assert lib.sdn_clip_vision_create(C.byref(c), C.byref(vh)) == 0
    try:
        assert len(handles) == len(others) == 7
        for j, h in enumerate(handles):
            assert vis_fwd(h) == -1, f"sdn_clip_vision_forward accepted handle kind {j}"
            assert others[j](h) == -3                              # (each still reaches the plan runner on its own handle)
        for j, fwd in enumerate(others):
            assert fwd(vh) == -1, f"forward {j} accepted a vision handle"
        assert vis_fwd(vh) == -3                                   # SDN_E_WORKSPACE: its own handle, a zero-byte workspace
    finally:
        lib.sdn_unet_destroy(vh)
        for h in handles:
            lib.sdn_unet_destroy(h)


# ---------------------------------------------------------------------------------------------- 9. from_pretrained
def test_from_pretrained_on_a_written_directory(tmp_path):
    from safetensors.torch import save_file
    sd = O.golden_state_dict(G)
    (tmp_path / "config.json").write_text(json.dumps(dict(CFG, architectures=["CLIPVisionModelWithProjection"], layer_norm_eps=1e-5)))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m = V.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), dtype=torch.float16)
    hand = small(torch.float16)
    assert m.config.hidden_act == "quick_gelu" and m.config.projection_dim == 64 and torch.equal(m._weights, hand._weights)
    a, b = m(gold("pixel_values")), hand(gold("pixel_values"))
    assert torch.equal(a.image_embeds, b.image_embeds) and torch.equal(a.last_hidden_state, b.last_hidden_state)
    # the OpenAI form of the same checkpoint gives the same model
    oa = V.CLIPVisionModelWithProjection.from_openai_state_dict(O.to_openai_state_dict(sd), dtype=torch.float16)
    assert vars(oa.config) == vars(hand.config) and torch.equal(oa._weights, hand._weights)
    (tmp_path / "config.json").write_text(json.dumps(dict(CFG, hidden_act="relu")))
    with pytest.raises(NotImplementedError):
        V.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path))
