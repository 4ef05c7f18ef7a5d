"""Host-side checks of the COCO driver's CLIP-score evaluator (CLIP ViT-H/14): the create gate for heads of 80, the ViT-H manifest,
the two oracles against a randomly initialised transformers CLIPModel with heads of 80, the crop tables of clip_preprocess_any
against Pillow and against transformers' image processor, the CLIPModel config readers, parse_coco_args, the COCO branch of
RunArtifacts, and the refusals of the new entry points.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint, clip_vision as V, coco_eval as E, driver
from safe_denoiser_amd.clip import CLIPTextModelWithProjection
from tests_support import clip_proj_oracle as OP
from tests_support import clip_vision_oracle as OV
from tests_support import refset_oracle as RO
from tests_support.coco_support import pillow_crop, sample_image as _image

SIZES = [(227, 301), (301, 227), (224, 224), (225, 640), (480, 640)]        # (h, w)
SMALL_VISION = dict(image_size=56, patch_size=14, hidden_size=640, intermediate_size=256, num_hidden_layers=2, num_attention_heads=8,
                    projection_dim=64, hidden_act="gelu")
SMALL_TEXT = dict(vocab_size=99, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                  max_position_embeddings=77, hidden_act="gelu", projection_dim=64, eos_token_id=2)


def _cfg(**kw):
    base = dict(image_size=56, patch_size=14, hidden_size=640, intermediate_size=256, num_layers=2, num_heads=8, projection_dim=64, act=7, dtype=0)
    base.update(kw)
    return _lib.ClipVisionConfig(**base)


# ------------------------------------------------------------------------------------------------------------ the gate and the plan
def test_create_accepts_heads_of_80_and_still_refuses_the_rest():
    """Fails on the parent commit, whose create demanded hidden_size == 64 * num_heads."""
    lib = sda.lib()
    h = C.c_void_p()
    vith = dict(image_size=224, hidden_size=1280, num_heads=16, intermediate_size=5120, num_layers=32, projection_dim=1024)
    for ok in (dict(dtype=0), dict(dtype=1), dict(dtype=0, **vith), dict(dtype=1, **vith)):
        assert lib.sdn_clip_vision_create(C.byref(_cfg(**ok)), C.byref(h)) == 0, ok
        lib.sdn_unet_destroy(h)
    for bad in (dict(hidden_size=1024, num_heads=8), dict(hidden_size=640, num_heads=5), dict(dtype=2), dict(dtype=3),
                dict(hidden_size=1408, num_heads=22), dict(hidden_size=720, num_heads=9), dict(num_heads=0)):
        assert lib.sdn_clip_vision_create(C.byref(_cfg(**bad)), C.byref(h)) == -1, bad


def test_vit_h14_manifest_and_batch_arithmetic():
    assert V.VIT_H14_CONFIG == dict(image_size=224, patch_size=14, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32,
                                    num_attention_heads=16, projection_dim=1024, hidden_act="gelu")
    assert sda.VIT_H14_CONFIG is V.VIT_H14_CONFIG
    m = V.CLIPVisionModelWithProjection(dtype=torch.float16, **V.VIT_H14_CONFIG)
    assert m.state_dict_shapes() == OV.expected_state_dict_shapes(V.VIT_H14_CONFIG)
    assert m.num_tokens == 257 and m._kpad() == 640
    assert m.max_batch == ((1 << 31) - 4096) // (2 * 5120 * 257) and m.max_batch >= 1
    ws = [_lib.lib().sdn_unet_workspace_bytes(m._h, b) for b in (1, 2, 8, 64)]
    assert 0 < ws[0] < ws[1] < ws[2] < ws[3]
    total, attn = m.flops(2)
    assert attn == 32 * 4.0 * 2 * 16 * 257 * 257 * 80
    small = V.CLIPVisionModelWithProjection(dtype=torch.bfloat16, **SMALL_VISION)
    assert small.num_tokens == 17 and small.max_batch > V.CLIPVisionModelWithProjection(dtype=torch.bfloat16, **V.VIT_H14_CONFIG).max_batch
    with pytest.raises(sda.SdnError):
        V.CLIPVisionModelWithProjection(hidden_size=1024, num_attention_heads=8)      # head dim 128 stays refused
    with pytest.raises(sda.SdnError):
        V.CLIPVisionModelWithProjection(dtype=torch.float32, **V.VIT_H14_CONFIG)


# ------------------------------------------------------------------------------------- the oracles against transformers at heads of 80
def reference_clip_score(image_features, text_features):
    """What the reference's Eval.clip_score does with the two feature matrices: unit rows, every image against every prompt, the mean."""
    a = image_features / image_features.norm(dim=-1, keepdim=True)
    b = text_features / text_features.norm(dim=-1, keepdim=True)
    return float((a @ b.T).mean())


def _features(out):
    return out if isinstance(out, torch.Tensor) else out.pooler_output


@pytest.fixture(scope="module")
def hf_model():
    tr = pytest.importorskip("transformers")
    cfg = tr.CLIPConfig(vision_config={k: v for k, v in SMALL_VISION.items() if k != "projection_dim"},
                        text_config={**{k: v for k, v in SMALL_TEXT.items() if k != "projection_dim"}, "bos_token_id": 0, "pad_token_id": 1},
                        projection_dim=64)
    torch.manual_seed(20)
    model = tr.CLIPModel(cfg).eval()
    with torch.no_grad():                                        # biases and norms away from their trivial initial values
        g = torch.Generator().manual_seed(21)
        for k, p in model.named_parameters():
            if p.dim() == 1 and k != "logit_scale":
                p.add_(0.1 * (torch.rand(p.shape, generator=g) - 0.5))
    return model


def test_oracles_reproduce_transformers_clip_model_with_heads_of_80(hf_model):
    g = torch.Generator().manual_seed(22)
    pixels = torch.randn(3, 3, 56, 56, generator=g)
    ids = torch.randint(3, 98, (4, 77), generator=g)
    for i, n in enumerate((5, 12, 40, 77)):                      # the end-of-text id is the highest: the legacy pooling rule
        ids[i, n - 1] = 98
        ids[i, n:] = 1
    sd = hf_model.state_dict()
    with torch.no_grad():
        want_i = _features(hf_model.get_image_features(pixel_values=pixels))
        want_t = _features(hf_model.get_text_features(input_ids=ids, attention_mask=(ids != 1).long()))
        got_i = OV.clip_vision_with_projection(sd, pixels, num_heads=8, hidden_act="gelu").image_embeds
        got_t = OP.clip_text_with_projection(sd, ids, num_heads=2, hidden_act="gelu", eos_token_id=2).text_embeds
    assert tuple(want_i.shape) == (3, 64) and tuple(want_t.shape) == (4, 64)
    errs = (OV.rel_l2(got_i, want_i), OV.rel_l2(got_t, want_t))
    print(errs)
    assert max(errs) <= 1e-5                                     # tests/test_clip_vision_host.py's bound for its transformers fixture
    # the padding argument of coco_eval.coco_ids: the features of a row do not depend on what follows its end-of-text token
    with torch.no_grad():
        short = _features(hf_model.get_text_features(input_ids=ids[:2, :12], attention_mask=(ids[:2, :12] != 1).long()))
    assert OV.rel_l2(short, want_t[:2]) <= 1e-5
    # the head, on oracle features: the reference expression against the factored form the kernel computes
    want = reference_clip_score(got_i, got_t)
    xi = (got_i.double() / got_i.double().norm(dim=-1, keepdim=True)).sum(0)
    yt = (got_t.double() / got_t.double().norm(dim=-1, keepdim=True)).sum(0)
    assert abs(float(xi @ yt) / 12 - want) <= 1e-6
    assert abs(reference_clip_score(got_i[:1], got_t[:1]) - float(torch.nn.functional.cosine_similarity(got_i[:1], got_t[:1]))) <= 1e-6


def test_clip_model_config_readers(hf_model, tmp_path):
    with open(tmp_path / "config.json", "w") as f:
        f.write(hf_model.config.to_json_string(use_diff=False))
    cfg = checkpoint.read_config(str(tmp_path))
    cfg.setdefault("architectures", ["CLIPModel"])
    if cfg["architectures"] is None:
        cfg["architectures"] = ["CLIPModel"]
    assert checkpoint.clip_vision_kwargs(cfg) == SMALL_VISION
    assert checkpoint.clip_model_text_kwargs(cfg) == SMALL_TEXT
    text = CLIPTextModelWithProjection(dtype=torch.float16, **checkpoint.clip_model_text_kwargs(cfg))
    assert text.state_dict_shapes() == OP.expected_state_dict_shapes(SMALL_TEXT)
    sd = hf_model.state_dict()
    vision = V.CLIPVisionModelWithProjection(dtype=torch.float16, **checkpoint.clip_vision_kwargs(cfg))
    vision.pack_state_dict(sd)                                   # a whole CLIPModel state dict serves both towers
    text.pack_state_dict(sd)
    # refusals: head dim 128, a text-only config, a stand-alone text encoder's reader on a CLIPModel
    for bad in (dict(num_attention_heads=5), dict(num_attention_heads=4), dict(hidden_size=1024, num_attention_heads=8)):
        with pytest.raises(NotImplementedError):
            checkpoint.clip_vision_kwargs({**cfg, "vision_config": {**cfg["vision_config"], **bad}})
    with pytest.raises(NotImplementedError):
        checkpoint.clip_model_text_kwargs({k: v for k, v in cfg.items() if k != "text_config"})
    with pytest.raises(NotImplementedError):
        checkpoint.clip_model_text_kwargs({**cfg, "architectures": ["CLIPTextModelWithProjection"]})
    with pytest.raises(NotImplementedError):
        checkpoint.clip_projection_kwargs({**cfg["text_config"], "architectures": ["CLIPModel"]})
    with pytest.raises(NotImplementedError):
        checkpoint.clip_model_text_kwargs({**cfg, "text_config": {**cfg["text_config"], "hidden_act": "relu"}})


# ---------------------------------------------------------------------------------------------------------------- preprocessing
def _pass_with(img, coeffs, bounds):
    """One pass along axis 1 with tables in the engine's format, through refset_oracle's restatement of Pillow's pass."""
    return RO._pass(img, [(int(lo), coeffs[i, :int(n)].astype(np.int64)) for i, (lo, n) in enumerate(bounds)])


def cpu_crop(img, size, crop):
    """The uint8 crop assembled on the host from crop_tables: what sdn_image_resize_rect_u8 computes from the same tables."""
    h, w = img.shape[:2]
    rh, rw = V.resized_shape(h, w, size)
    top, left = V.crop_offset(rh, size, crop), V.crop_offset(rw, size, crop)
    tx, ty = V.crop_tables(w, rw, left, size), V.crop_tables(h, rh, top, size)
    cur = img
    if tx is not None:
        cur = _pass_with(cur, tx[0], tx[1])
    if ty is not None:
        cur = _pass_with(np.ascontiguousarray(cur.transpose(1, 0, 2)), ty[0], ty[1]).transpose(1, 0, 2)
    return np.ascontiguousarray(cur), (rh, rw, top, left)


def test_crop_offsets_of_the_two_libraries():
    assert [V.crop_offset(224 + e, 224, "transformers") for e in range(6)] == [0, 0, 1, 1, 2, 2]
    assert [V.crop_offset(224 + e, 224, "torchvision") for e in range(6)] == [0, 0, 1, 2, 2, 2]      # round half to even
    assert V.resized_shape(227, 301, 224) == (224, 297) and V.resized_shape(301, 227, 224) == (297, 224)
    assert V.resized_shape(225, 640, 224) == (224, 637) and V.resized_shape(480, 640, 224) == (224, 298)
    assert V.resized_shape(224, 224, 224) == (224, 224)
    for bad in (lambda: V.crop_offset(100, 224), lambda: V.crop_offset(300, 224, "pillow")):
        with pytest.raises(sda.SdnError):
            bad()
    assert V.crop_tables(224, 224, 0, 224) is None
    c, b, k = V.crop_tables(301, 301, 38, 224)                    # an axis that is cropped and not resampled: the one-tap copy
    assert k == 1 and c.tolist() == [[1 << 22]] * 224 and b[:, 0].tolist() == list(range(38, 262)) and set(b[:, 1].tolist()) == {1}


@pytest.mark.parametrize("crop", ["transformers", "torchvision"])
@pytest.mark.parametrize("h,w", SIZES)
def test_cropped_tables_equal_pillow_resize_then_crop(h, w, crop):
    img = _image(h, w, h * 1000 + w)
    got, (rh, rw, top, left) = cpu_crop(img, 224, crop)
    assert got.shape == (224, 224, 3) and 0 <= top <= rh - 224 and 0 <= left <= rw - 224
    assert np.array_equal(got, pillow_crop(img, 224, crop))
    for n_in, n_res, off in ((w, rw, left), (h, rh, top)):        # every tap the kernel would follow lies inside the input
        t = V.crop_tables(n_in, n_res, off, 224)
        if t is not None:
            assert t[0].shape == (224, t[2]) and t[1].shape == (224, 2) and t[0].dtype == t[1].dtype == np.int32
            assert int(t[1][:, 0].min()) >= 0 and int((t[1][:, 0] + t[1][:, 1]).max()) <= n_in and int(t[1][:, 1].max()) <= t[2]


@pytest.mark.parametrize("h,w", SIZES)
def test_f32_pixels_equal_transformers_image_processor(h, w):
    """2^-21 absolute: u * (1 / 255) against u / 255 differs by at most one ulp at <= 1 (6e-8), divided by std >= 0.261, plus one
    rounding of the result at <= 2.7."""
    tr = pytest.importorskip("transformers")
    proc = tr.CLIPImageProcessorPil(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, resample=Image.BICUBIC)
    img = _image(h, w, h * 1000 + w + 1)
    want = torch.as_tensor(np.asarray(proc(images=Image.fromarray(img), return_tensors="np")["pixel_values"]))
    got = OV.preprocess(torch.from_numpy(cpu_crop(img, 224, "transformers")[0])[None])
    assert tuple(want.shape) == tuple(got.shape) == (1, 3, 224, 224) and want.dtype == torch.float32
    err = float((got - want).abs().max())                        # every pixel
    print(f"{h} x {w}: max |pixel_values - transformers| = {err:.3e}")
    assert err <= 2.0 ** -21


def test_groups_take_any_aspect_ratio():
    parts = V._as_u8_groups([Image.new("RGB", (80, 64)), Image.new("L", (80, 64)), Image.new("RGB", (16, 16))], "cpu")
    assert [tuple(p.shape) for p in parts] == [(2, 64, 80, 3), (1, 16, 16, 3)]
    assert tuple(V._as_u8_groups(torch.zeros(2, 80, 64, 3, dtype=torch.uint8), "cpu")[0].shape) == (2, 80, 64, 3)
    with pytest.raises(sda.SdnError):
        V._as_u8_groups(torch.zeros(2, 80, 64, 3), "cpu")
    with pytest.raises(sda.SdnError):
        V._as_u8_groups([np.zeros((8, 8, 3), np.uint8)], "cpu")
    with pytest.raises(sda.SdnError):                             # the square-only refusals stand
        V._as_u8_batches(torch.zeros(2, 80, 64, 3, dtype=torch.uint8), "cpu")


# ------------------------------------------------------------------------------------------------------------------- the driver
def _write_config(tmp_path, **kw):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(kw))
    return str(p)


def test_parse_coco_args_defaults_and_choices(tmp_path):
    cfg = _write_config(tmp_path, save_dir=str(tmp_path / "out"))
    a = driver.parse_coco_args(["--config", cfg])
    assert a.category == "coco" and a.save_dir == str(tmp_path / "out") and a.erase_id == "std" and a.nudity_thr == 0.6
    assert driver.parse_coco_args(["--config", cfg, "--category", "coco_open_clip"]).category == "coco_open_clip"
    assert driver.parse_coco_args(["--config", _write_config(tmp_path, category="coco_open_clip")]).category == "coco_open_clip"
    assert driver.parse_coco_args(["--config", _write_config(tmp_path, nudity="all")]).category == "coco"      # the key is "category" here
    for bad in ("nudity", "all", "artists-VanGogh"):
        with pytest.raises(SystemExit):
            driver.parse_coco_args(["--config", cfg, "--category", bad])
    with pytest.raises(SystemExit):                               # parse_args is what it was
        driver.parse_args(["--config", cfg, "--category", "coco"])
    assert driver.parse_args(["--config", cfg]).category == "all"


class StubEval:
    def __init__(self):
        self.calls = []

    def __call__(self, samples, threshold=0.6, org_samples=None, prompts=None):
        self.calls.append((len(samples), list(prompts)))
        return None, 0.125 * len(self.calls) + 0.0004


def test_run_artifacts_coco_branch(tmp_path, capsys):
    args = driver.parse_coco_args(["--config", _write_config(tmp_path, save_dir=str(tmp_path / "out"))])
    art = driver.RunArtifacts(args)
    ev = StubEval()
    cases = [dict(case_number=7, categories="coco", prompt="a cat", seed=1, row=0), dict(case_number=9, categories="coco", prompt="a dog", seed=2, row=1),
             dict(case_number=11, categories=["coco"], prompt="a bird", seed=3, row=2)]
    paths = [art.record(c, Image.new("RGB", (8, 8)), eval_func=ev) for c in cases[:2]]
    paths.append(art.record(cases[2], Image.new("RGB", (8, 8)), eval_func=ev, pred=0.5))       # a score the caller computed: no call
    art.finish(dataset_size=5)
    out = str(tmp_path / "out")
    assert paths == [os.path.join(out, "all", f"{n}.png") for n in (7, 9, 11)] and all(os.path.isfile(p) for p in paths)
    assert sorted(os.listdir(os.path.join(out, "all"))) == ["11.png", "7.png", "9.png"]
    assert os.listdir(os.path.join(out, "safe")) == [] and os.listdir(os.path.join(out, "unsafe")) == []
    assert ev.calls == [(1, ["a cat"]), (1, ["a dog"])]
    with open(os.path.join(out, "detect_dict.json")) as f:
        d = json.load(f)
    scores = [0.1254, 0.2504, 0.5]
    assert set(d) == {"avg_clip", "total_imgs"} and d["total_imgs"] == 3 and abs(d["avg_clip"] - sum(scores) / 3) < 1e-12
    with open(os.path.join(out, "logs.txt")) as f:
        log = f.read()
    for line in ("CLIP Score (Img, Prompt) is : 0.125", "CLIP Score (Img, Prompt) is : 0.250", "CLIP Score (Img, Prompt) is : 0.500",
                 "Avg_clip: 0.292", "Evaluated_num_imgs: 3", "Original data size: 5"):
        assert line in log, line
    assert "toxic" not in log and "unsafe" not in log
    assert os.path.isfile(os.path.join(out, "config.yaml"))


def test_run_artifacts_coco_branch_refuses_a_table_with_other_categories(tmp_path):
    """finish() averages the scores filed under 'coco' alone: a case of another category is refused by name when it is recorded, not
    with a KeyError after the last image."""
    args = driver.parse_coco_args(["--config", _write_config(tmp_path, save_dir=str(tmp_path / "out"))])
    art = driver.RunArtifacts(args)
    with pytest.raises(sda.SdnError, match="category 'coco'"):
        art.record(dict(case_number=3, categories=["nudity"], prompt="a cat", seed=1, row=0), Image.new("RGB", (8, 8)), eval_func=StubEval())
    art.logger.close()


# ------------------------------------------------------------------------------------------------------------------- refusals
def _evaluator():
    return E.CocoClipEval(V.CLIPVisionModelWithProjection(dtype=torch.float16, **SMALL_VISION),
                          CLIPTextModelWithProjection(dtype=torch.float16, **SMALL_TEXT))


def test_evaluator_refusals():
    ev = _evaluator()
    assert sda.CocoClipEval is E.CocoClipEval and sda.clip_preprocess_any is V.clip_preprocess_any
    with pytest.raises(sda.SdnError, match="78 tokens"):
        ev.text_features(torch.ones(1, 78, dtype=torch.int64))
    with pytest.raises(sda.SdnError):
        ev.clip_score([], [])
    with pytest.raises(sda.SdnError):
        ev.pair_scores([], [])
    with pytest.raises(sda.SdnError):
        ev.text_features(["a prompt"])                            # strings without a tokenizer
    with pytest.raises(sda.SdnError):
        ev.text_features(torch.ones(1, 20, dtype=torch.int64))    # short rows need the tokenizer's pad id
    with pytest.raises(sda.SdnError):
        E.CocoClipEval(ev.vision, CLIPTextModelWithProjection(dtype=torch.float16, **{**SMALL_TEXT, "projection_dim": 32}))
    tok = OP.FakeCLIPTokenizer(vocab_size=99, model_max_length=77)
    ids = E._pad_ids(torch.full((2, 20), 5, dtype=torch.int64), 77, tok.pad_token_id)
    assert tuple(ids.shape) == (2, 77) and bool((ids[:, 20:] == tok.pad_token_id).all()) and bool((ids[:, :20] == 5).all())


def test_cross_mean_rejects_bad_arguments_on_host():
    lib = sda.lib()
    X, Y, S, O_ = 0x10000, 0x20000, 0x30000, 0x40000
    f = lambda x=X, dx=1, ldx=64, rx=3, y=Y, dy=1, ldy=64, ry=5, dim=64, s=S, out=O_: lib.sdn_embed_cross_mean(
        x, dx, ldx, rx, y, dy, ldy, ry, dim, s, out, None)
    assert f(x=None) == -1 and f(y=None) == -1 and f(s=None) == -1 and f(out=None) == -1
    assert f(dim=0) == -1 and f(rx=0) == -1 and f(ry=0) == -1 and f(rx=-1) == -1
    assert f(ldx=63) == -1 and f(ldy=63) == -1
    assert f(dx=3) == -1 and f(dx=-1) == -1 and f(dy=3) == -1 and f(dy=-1) == -1
    assert f(x=X + 8) == -1 and f(y=Y + 2) == -1 and f(s=S + 2) == -1 and f(out=O_ + 1) == -1
