"""Host-side checks of the image metrics (safe_denoiser_amd/metrics.py): the aesthetic head composed into one affine map against a
layer-by-layer float64 evaluation and against the fixture captured from the reference's own AE_MLP, the CLIP score's token rule
with the stand-in tokenizer, the three evaluators over a directory of tiny PNGs with a stub scorer, and the argument validation of
sdn_embed_row_scores.  No GPU."""
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import safe_denoiser_amd as sda
from safe_denoiser_amd import metrics as M
from tests_support.fake_tokenizer import FakeCLIPTokenizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aes_golden.npz")
LINEARS = (0, 2, 4, 6, 7)


def layer_by_layer(sd, x):
    h = x.double()
    for i in LINEARS:
        h = h @ sd[f"layers.{i}.weight"].double().T + sd[f"layers.{i}.bias"].double()
    return h[:, 0]


def affine_bound(x, w_eff, b_eff):
    """(D + 16) 2^-24 (sum |x_i w_i| + |b_eff|) per row: the worst case of an f32 dot product of D terms in any order, plus slack
    for the normalisation -- the bound the GPU head is held to, here on the float64 evaluation of the f32 w_eff."""
    d = x.shape[1]
    return (d + 16) * 2.0 ** -24 * ((x.double().abs() * w_eff.double().abs()).sum(-1) + abs(b_eff))


def test_compose_affine_equals_the_five_linears_in_float64():
    g = torch.Generator().manual_seed(7)
    widths = (96, 1024, 128, 64, 16, 1)
    sd = {}
    for i, fan_in, fan_out in zip(LINEARS, widths[:-1], widths[1:]):
        sd[f"layers.{i}.weight"] = torch.randn(fan_out, fan_in, generator=g) * (1.5 / fan_in ** 0.5)
        sd[f"layers.{i}.bias"] = 0.1 * torch.randn(fan_out, generator=g)
    sd["layers.7.bias"] += 5.0                                     # scores of the real head's size
    w_eff, b_eff = M.compose_affine(sd)
    assert w_eff.dtype == torch.float32 and tuple(w_eff.shape) == (96,) and isinstance(b_eff, float)
    x = torch.randn(9, 96, generator=g, dtype=torch.float64)
    x = x / x.norm(dim=-1, keepdim=True)
    want = layer_by_layer(sd, x)
    got = x @ w_eff.double() + b_eff
    err, bound = (got - want).abs(), affine_bound(x, w_eff, b_eff)
    print(f"compose_affine: scores {want.tolist()}, max err / bound {float((err / bound).max()):.3f}")
    assert 2.0 < float(want.abs().mean()) < 10.0
    assert bool((err <= bound).all())
    # numpy arrays are taken too, a head that does not chain or does not end in one output is refused
    w2, b2 = M.compose_affine({k: v.numpy() for k, v in sd.items()})
    assert torch.equal(w2, w_eff) and b2 == b_eff
    with pytest.raises(sda.SdnError):
        M.compose_affine(dict(sd, **{"layers.4.weight": sd["layers.4.weight"][:, :100]}))
    with pytest.raises(sda.SdnError):
        M.compose_affine(dict(sd, **{"layers.7.weight": sd["layers.7.weight"].repeat(2, 1), "layers.7.bias": sd["layers.7.bias"].repeat(2)}))
    with pytest.raises(KeyError):
        M.compose_affine({k.replace("layers.2.", "layers.1."): v for k, v in sd.items()})


def test_compose_affine_on_the_reference_heads_own_keys_and_outputs():
    """tests/golden/aes_golden.npz: the state dict, inputs and outputs of the reference's AE_MLP class executed as it stands
    (make_aes_golden.py) -- pins the layers.{0,2,4,6,7} key layout and the absence of an activation."""
    assert os.path.getsize(GOLDEN) < 1 << 20
    g = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32)) for k in g.files if k.startswith("sd/")}
    assert sorted(sd) == sorted(f"layers.{i}.{p}" for i in LINEARS for p in ("weight", "bias"))
    assert all(g[k].dtype == np.float16 for k in g.files if k.startswith("sd/"))
    x, want = torch.from_numpy(g["inputs"]), torch.from_numpy(g["outputs"])
    assert tuple(x.shape) == (6, 64) and float((x.double().norm(dim=-1) - 1).abs().max()) < 1e-6
    w_eff, b_eff = M.compose_affine(sd)
    assert tuple(w_eff.shape) == (64,)
    err = (x.double() @ w_eff.double() + b_eff - want).abs()
    assert bool((err <= affine_bound(x, w_eff, b_eff)).all()), err.tolist()


def test_aesthetic_score_refuses_a_head_of_another_width():
    g = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32)) for k in g.files if k.startswith("sd/")}
    from types import SimpleNamespace
    with pytest.raises(sda.SdnError):
        M.AestheticScore(SimpleNamespace(config=SimpleNamespace(projection_dim=768, image_size=224)), sd)
    a = M.AestheticScore(SimpleNamespace(config=SimpleNamespace(projection_dim=64, image_size=56)), sd)
    assert a.state() == (0.0, 0) and a.scores.numel() == 0
    with pytest.raises(sda.SdnError):
        a.compute()
    with pytest.raises(sda.SdnError):                             # CLIPScore: towers of different projection widths
        M.CLIPScore(SimpleNamespace(config=SimpleNamespace(projection_dim=64)), SimpleNamespace(config=SimpleNamespace(projection_dim=512)))


def test_clip_score_ids_pads_short_prompts_and_cuts_long_ones_without_an_eos():
    tok = FakeCLIPTokenizer(vocab_size=1000)
    short, long_ = "a photo of a cat", " ".join(f"word{i}" for i in range(85))
    ids, cut = M.clip_score_ids(tok, [short], 77)
    assert tuple(ids.shape) == (1, 77) and ids.dtype == torch.int64 and cut == 0
    assert ids[0, 0] == tok.bos_token_id and ids[0, 6] == tok.eos_token_id and bool((ids[0, 7:] == tok.pad_token_id).all())
    assert ids[0, 1:6].tolist() == tok._ids(short)
    ids, cut = M.clip_score_ids(tok, [short, long_], 77)
    assert tuple(ids.shape) == (2, 77) and cut == 1
    assert ids[1].tolist() == [tok.bos_token_id] + tok._ids(long_)[:76]           # the first 77 ids of the uncut row ...
    assert tok.eos_token_id not in ids[1].tolist()                                 # ... which hold no end-of-text token
    assert ids[0, 6] == tok.eos_token_id and bool((ids[0, 7:] == tok.pad_token_id).all())
    # a prompt of exactly 77 tokens is not cut
    ids, cut = M.clip_score_ids(tok, " ".join(f"w{i}" for i in range(75)), 77)
    assert cut == 0 and ids[0, 76] == tok.eos_token_id
    # CLIPScore counts the cut prompts across updates; reset clears the count
    from types import SimpleNamespace
    tower = SimpleNamespace(config=SimpleNamespace(projection_dim=64, max_position_embeddings=77))
    cs = M.CLIPScore(tower, tower, tok)
    assert tuple(cs._ids([long_, short, long_]).shape) == (3, 77) and cs.n_truncated == 2
    cs._ids([long_])
    assert cs.n_truncated == 3
    cs.reset()
    assert cs.n_truncated == 0
    with pytest.raises(sda.SdnError):
        M.CLIPScore(tower, tower)._ids([short])                   # strings without a tokenizer
    with pytest.raises(sda.SdnError):
        cs._ids(torch.zeros(2, 60, dtype=torch.int64))


class StubScorer:
    """Records what the evaluators feed it; the score of an image is its red value at (0, 0)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.batches, self.values = [], []

    def update(self, images, text=None):
        assert all(im.mode == "RGB" for im in images)
        self.batches.append(([im.getpixel((0, 0))[0] for im in images], None if text is None else list(text)))
        self.values += [float(im.getpixel((0, 0))[0]) for im in images]

    def compute(self):
        return np.float32(sum(self.values) / len(self.values))    # not a Python float: the evaluators must convert


def _tree(tmp_path, names):
    d = tmp_path / "job" / "all"
    d.mkdir(parents=True)
    for name, red in names.items():
        Image.new("RGB", (4, 4), (red, 0, 0)).save(d / name)
    return str(d)


def test_evaluate_clip_score_matches_coco_ids_to_captions(tmp_path):
    import pandas as pd
    d = _tree(tmp_path, {"7.png": 70, "12.png": 120, "3.png": 30, "40.png": 40, "5.png": 50})
    frame = pd.DataFrame({"image_id": [3, 5, 7, 12, 40, 99], "caption": ["three", "five", "seven", "twelve", "forty", "unused"]})
    s = StubScorer()
    out = M.evaluate_clip_score(d, "coco", frame, 2, "cuda", scorer=s, filename="clip")
    # every file, in sorted-name order, in batches of two with a last batch of one, each image with its own caption
    assert s.batches == [([120, 30], ["twelve", "three"]), ([40, 50], ["forty", "five"]), ([70], ["seven"])]
    path = os.path.join(os.path.dirname(d), "clip.yaml")
    assert out == {"clip_score": pytest.approx(62.0)} and type(out["clip_score"]) is float
    assert yaml.safe_load(open(path)) == {"clip_score": pytest.approx(62.0)}
    with pytest.raises(TypeError):
        M.evaluate_clip_score(d, "coco", frame, 2)                # the scorer is required
    with pytest.raises(KeyError):
        M.evaluate_clip_score(d, prompts_csv=frame[frame.image_id != 7], batch_size=2, scorer=s)


def test_evaluate_clip_score_copro_parses_the_idx_prefix(tmp_path):
    import pandas as pd
    d = _tree(tmp_path, {"28731_n-u-d-i-t-y.png": 10, "28733_n-u-d-i-t-y.png": 30, "28732_hate.png": 20})
    frame = pd.DataFrame({"idx": [28733, 28731, 28732], "unsafe_prompt": ["c", "a", "b"], "safe_prompt": ["x", "y", "z"]})
    s = StubScorer()
    out = M.evaluate_clip_score_CoPro(sample_dir=d, prompts_csv=frame, batch_size=None, scorer=s)
    assert s.batches == [([10, 20, 30], ["a", "b", "c"])]        # batch_size None: one batch
    assert yaml.safe_load(open(os.path.join(os.path.dirname(d), "metrics.yaml"))) == {"clip_score": pytest.approx(20.0)} == out


def test_evaluate_aes_score_copro_scores_every_file(tmp_path):
    d = _tree(tmp_path, {"1_a.png": 10, "2_b.png": 20, "3_c.png": 60})
    s = StubScorer()
    out = M.evaluate_aes_score_CoPro(d, "sample", 2, None, "unused.pth", scorer=s, filename="aes")
    assert s.batches == [([10, 20], None), ([60], None)]
    assert out == {"aes_score": pytest.approx(30.0)} and type(out["aes_score"]) is float
    assert yaml.safe_load(open(os.path.join(os.path.dirname(d), "aes.yaml"))) == out
    assert 1 <= M.decode_workers() <= 16                            # the decode pool's size: data.py's cap


def test_embed_row_scores_rejects_bad_arguments_on_host():
    lib = sda.lib()
    X, Y, O_ = 0x10000, 0x20000, 0x30000
    f = lambda x=X, dx=1, ldx=64, y=Y, dy=1, ldy=64, y_rows=3, rows=3, dim=64, out=O_: lib.sdn_embed_row_scores(
        x, dx, ldx, y, dy, ldy, y_rows, rows, dim, 1, 100.0, 0.0, out, None)
    assert f(x=None) == -1 and f(y=None) == -1 and f(out=None) == -1
    assert f(dim=0) == -1
    assert f(y_rows=2) == -1
    assert f(ldx=63) == -1 and f(ldy=63) == -1
    assert f(dx=3) == -1 and f(dy=3) == -1 and f(dx=-1) == -1
    assert f(x=X + 8) == -1 and f(y=Y + 2) == -1 and f(out=O_ + 2) == -1       # misaligned pointers
    assert f(rows=0, y_rows=0) == 0 and f(rows=0, y_rows=1, x=None, y=None, out=None) == 0      # zero rows: a no-op
