"""The image metrics on the GPU: sdn_embed_row_scores against float64 at every shape at which it takes another path, the aesthetic
head on the fixture captured from the reference's AE_MLP, the CLIP score end to end on the two towers' transformers fixtures, and
`driver.run_job(metrics=...)` on the smallest pipeline tests/test_gpu_driver.py builds.  The measured deviation of the CLIP score
from the fp32 fixtures goes to profiles/metrics_parity.json (synthetic weights)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint, driver, metrics as M
from safe_denoiser_amd.clip import CLIPTextModelWithProjection
from safe_denoiser_amd.clip_vision import CLIPVisionModelWithProjection, clip_preprocess
from tests_support import clip_proj_oracle as OP
from tests_support import clip_vision_oracle as OV
from tests_support import exact as X
from tests_support.fake_tokenizer import FakeCLIPTokenizer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "metrics_parity.json")
GV, GP = OV.load_golden(), OP.load_golden()
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CODE = {"bf16": 0, "f16": 1, "f32": 2}
TOWER_K = 2.0          # the factor tests/test_gpu_clip_vision.py:72 and tests/test_gpu_clip_proj.py:62 allow over the fixture's recorded error


def record(key, value):
    data = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            data = json.load(f)
    data[key] = value
    with open(PARITY, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def aes_state_dict():
    g = np.load(os.path.join(ROOT, "tests", "golden", "aes_golden.npz"))
    return {k[3:]: torch.from_numpy(g[k].astype(np.float32)) for k in g.files if k.startswith("sd/")}, g


def small_vision(dtype=torch.float16):
    m = CLIPVisionModelWithProjection(dtype=dtype, **checkpoint.clip_vision_kwargs(GV["cfg"]))
    m.load_state_dict(OV.golden_state_dict(GV))
    return m


def small_text(dtype=torch.float16):
    m = CLIPTextModelWithProjection(dtype=dtype, **checkpoint.clip_projection_kwargs(GP["a/cfg"]))
    m.load_state_dict(OP.golden_state_dict(GP, "a"))
    return m


# ---------------------------------------------------------------------------------------------- 1. the kernel against float64
def nan_rows(t, ld):
    """Copy of t [R, W] as the view [:R, :W] of a NaN allocation [R + 1, ld]: the pitch gap and the row past the end are NaN."""
    buf = torch.full((t.shape[0] + 1, ld), float("nan"), dtype=t.dtype, device="cuda")
    buf[:t.shape[0], :t.shape[1]] = t
    return buf[:t.shape[0], :t.shape[1]]


def reference(x, y, normalize_y, scale, bias):
    """(exact scores, bound) in float64 from the stored operand values.  bound = |scale| (dim + 16) 2^-24 (sum |x^_i y'_i| + |cos|)
    + |bias| 2^-23 per row: dim 2^-24 sum |.| is the worst case of an f32 dot product of dim terms in ANY order, the 16 extra units
    cover the two norms, the division and the scaling, the last term the final addition."""
    x, y = x.double(), y.double()
    xh = x / x.norm(dim=-1, keepdim=True)
    yh = y / y.norm(dim=-1, keepdim=True) if normalize_y else y
    cos = (xh * yh).sum(-1)
    bound = abs(scale) * (x.shape[1] + 16) * 2.0 ** -24 * ((xh * yh).abs().sum(-1) + cos.abs()) + abs(bias) * 2.0 ** -23
    return scale * cos + bias, bound


def run_kernel(xv, yv, normalize_y, scale, bias):
    rows, dim = xv.shape
    buf, out = X.guarded_like((rows,), torch.float32, "cuda")
    ldx = xv.stride(0) if rows > 1 else max(xv.stride(0), dim)
    ldy = yv.stride(0) if yv.shape[0] > 1 else max(yv.stride(0), dim)
    rc = sda.lib().sdn_embed_row_scores(xv.data_ptr(), CODE_OF[xv.dtype], ldx, yv.data_ptr(), CODE_OF[yv.dtype], ldy, yv.shape[0], rows, dim,
                                        1 if normalize_y else 0, scale, bias, out.data_ptr(), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert X.sentinels_intact(buf, out) == 0
    return out.cpu()


CODE_OF = {DT[k]: CODE[k] for k in DT}
ROWS = (1, 3, 65)
DIMS = (1, 7, 64, 65, 96, 768, 1000)


def pitches(dim):
    """ld == dim (a dense matrix: 16-byte rows only at some widths, so both load paths), the next multiple of 8 elements above dim
    (16-byte rows in every dtype: the vector path with a NaN gap) and dim + 3 (an odd pitch with a NaN gap: element by element)."""
    return (dim, (dim + 8) // 8 * 8, dim + 3)


@pytest.mark.parametrize("ty", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("tx", ["bf16", "f16", "f32"])
def test_kernel_against_float64(tx, ty):
    g = torch.Generator().manual_seed(1000 * CODE[tx] + CODE[ty])
    worst, signs = 0.0, set()
    for rows in ROWS:
        for dim in DIMS:
            x = (torch.randn(rows, dim, generator=g) * 1.3).to(DT[tx])
            for sign in (1.0, -1.0):
                # paired rows, both normalised, scale 100: the CLIP score; scores of one sign per case
                y = (sign * (0.8 * x.float() + 0.6 * torch.randn(rows, dim, generator=g))).to(DT[ty])
                w = (0.5 * torch.randn(1, dim, generator=g)).to(DT[ty])       # one row for all, not normalised, a bias: the aesthetic head
                want_p, bound_p = reference(x, y, True, 100.0, 0.0)
                want_b, bound_b = reference(x, w, False, 1.0, sign * 5.25)
                if dim >= 64:
                    assert bool((want_p * sign > 0).all())
                    signs.add(sign)
                for ld in pitches(dim):
                    xv = nan_rows(x.cuda(), ld)
                    for yv, ny, sc, bi, want, bound, mode in ((nan_rows(y.cuda(), ld), True, 100.0, 0.0, want_p, bound_p, "paired"),
                                                             (nan_rows(w.cuda(), ld), False, 1.0, sign * 5.25, want_b, bound_b, "broadcast")):
                        got = run_kernel(xv, yv, ny, sc, bi)
                        err = (got.double() - want).abs()
                        assert bool(torch.isfinite(got).all()), (tx, ty, rows, dim, ld, mode)
                        ratio = float((err / bound).max())
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (tx, ty, rows, dim, ld, mode, sign, ratio)
    print(f"sdn_embed_row_scores {tx} x {ty}: worst error / bound {worst:.4f}")
    assert signs == {1.0, -1.0}


@pytest.mark.parametrize("rows,dim", [(3, 64), (65, 7), (5, 1000)])
def test_a_zero_row_is_nan_and_its_neighbours_are_not(rows, dim):
    g = torch.Generator().manual_seed(rows + dim)
    x = torch.randn(rows, dim, generator=g).to(torch.float16)
    x[1] = 0
    y = torch.randn(rows, dim, generator=g)
    want, bound = reference(x, y, True, 100.0, 0.0)
    got = run_kernel(x.cuda(), y.cuda(), True, 100.0, 0.0)
    keep = torch.arange(rows) != 1
    assert bool(torch.isnan(got[1])) and bool(torch.isfinite(got[keep]).all())
    assert bool(((got.double() - want).abs()[keep] <= bound[keep]).all())
    # a zero row on the y side of a pair: the same
    got = run_kernel(y.cuda(), x.cuda(), True, 100.0, 0.0)
    assert bool(torch.isnan(got[1])) and bool(torch.isfinite(got[keep]).all())
    # the wrapper is the same call
    assert torch.equal(M.embed_row_scores(y.cuda(), x.cuda(), True, 100.0).cpu()[keep], got[keep])
    assert M.embed_row_scores(y.cuda()[:0], x.cuda()[:0], True).numel() == 0


# ---------------------------------------------------------------------------------------------- 2. the aesthetic head
def test_aesthetic_score_on_the_reference_heads_fixture():
    sd, g = aes_state_dict()
    vision = small_vision()
    aes = M.AestheticScore(vision, sd)
    u8 = torch.from_numpy(GV["images"]).cuda()
    got = aes.score(u8)
    assert got.dtype == torch.float32 and tuple(got.shape) == (6,) and bool(torch.isfinite(got).all())
    # the head IS the kernel on the tower's own embeddings
    emb = vision(clip_preprocess(u8, 56), output_hidden_state=False).image_embeds
    assert emb.dtype == torch.float16
    w = aes.w_eff.cuda()
    assert torch.equal(got, M.embed_row_scores(emb, w, False, 1.0, aes.b_eff))
    want, bound = reference(emb.cpu(), aes.w_eff[None], False, 1.0, aes.b_eff)
    assert bool(((got.cpu().double() - want).abs() <= bound).all())
    # the fixture's unit-norm inputs through the kernel against the reference class's float64 outputs.  The kernel bound is the
    # worst case of ANY summation order (64 + 16 units of 2^-24); a wave sums 64 elements in a tree of depth <= 10, which leaves
    # room for the one rounding of w_eff to f32 (2^-24 sum |x^ w|) that separates the composed head from the five Linears.
    xin = torch.from_numpy(g["inputs"])
    _, bound = reference(xin, aes.w_eff[None], False, 1.0, aes.b_eff)
    direct = M.embed_row_scores(xin.cuda(), w, False, 1.0, aes.b_eff).cpu().double()
    err = (direct - torch.from_numpy(g["outputs"])).abs()
    print(f"aesthetic head on the fixture inputs: scores {direct.tolist()}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # update / compute / state / reset, with a ragged last batch (what the reference's np.mean of a list breaks on)
    aes.update(u8[:4])
    aes.update(u8[4:])
    assert torch.equal(aes.scores, got)
    total, n = aes.state()
    assert n == 6 and total == float(got.double().sum()) and aes.compute() == total / 6
    aes.reset()
    assert aes.state() == (0.0, 0)


def test_aesthetic_score_load_reads_a_checkpoint_file(tmp_path):
    sd, _ = aes_state_dict()
    torch.save(sd, tmp_path / "head.pth")
    vision = small_vision(torch.bfloat16)
    a, b = M.AestheticScore.load(vision, str(tmp_path / "head.pth")), M.AestheticScore(vision, sd)
    assert torch.equal(a.w_eff, b.w_eff) and a.b_eff == b.b_eff
    from PIL import Image
    pil = [Image.fromarray(im) for im in GV["images"][:3]]
    assert torch.equal(a.score(pil), b.score(torch.from_numpy(GV["images"][:3])))       # PIL images, host tensor: the same bits


# ---------------------------------------------------------------------------------------------- 3. the CLIP score end to end
def test_clip_score_on_the_two_towers_fixtures():
    vision, text = small_vision(), small_text()
    cs = M.CLIPScore(vision, text)
    u8 = torch.from_numpy(GV["images"][:4]).cuda()
    ids = torch.from_numpy(GP["a/ids"])
    cs.update(u8, ids)
    scores = cs.scores
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (4,) and scores.is_cuda
    # 1. pairing and order: the kernel on the two towers' separately computed embeddings, bit for bit
    img = vision(clip_preprocess(u8, 56), output_hidden_state=False).image_embeds
    txt = text(ids, output_hidden_states=True).text_embeds
    assert torch.equal(scores, M.embed_row_scores(img, txt, True, 100.0))
    # 2. the sanity net: the fixtures' fp32 embeddings in float64
    A, T = torch.from_numpy(GV["image_embeds"]).double(), torch.from_numpy(GP["a/text_embeds"]).double()
    a = A[:4]
    want = 100.0 * ((a / a.norm(dim=-1, keepdim=True)) * (T / T.norm(dim=-1, keepdim=True))).sum(-1)
    assert torch.allclose(want, torch.tensor([-20.431, -31.044, -17.569, -25.951], dtype=torch.float64), atol=1e-3, rtol=0)
    assert abs(float(want.mean()) + 23.749) < 1e-3
    da = 2 * TOWER_K * float(GV["err_f16_image_embeds"]) * A.norm() / a.norm(dim=-1)
    dt = 2 * TOWER_K * float(GP["a/err_f16_text_embeds"]) * T.norm() / T.norm(dim=-1)
    bound = 100.0 * (da + dt + da * dt)
    dev = (scores.cpu().double() - want).abs()
    print(f"clip score: {scores.cpu().tolist()} vs fixture {want.tolist()}; deviation {dev.tolist()}, bound {bound.tolist()}")
    record("clip_score_fixture/f16", {"scores": scores.cpu().tolist(), "fixture_fp32": want.tolist(), "deviation": dev.tolist(),
                                      "bound": bound.tolist(), "weights": "synthetic (the towers' transformers fixtures)"})
    assert bool((dev <= bound).all())
    # 3. the raw mean, the clamp, the state
    total, n = cs.state()
    assert n == 4 and total == float(scores.double().sum())
    assert abs(total / 4 - float(want.mean())) <= float(bound.mean())
    assert cs.compute() == 0.0                                    # max(mean, 0) of a negative mean
    cs.update(u8, ids)                                            # the same batch again: n doubles, the mean stays
    t2, n2 = cs.state()
    assert n2 == 8 and torch.equal(cs.scores, torch.cat([scores, scores])) and abs(t2 / 8 - total / 4) <= 1e-12 * abs(total)
    cs.reset()
    assert cs.state() == (0.0, 0) and cs.scores.numel() == 0 and cs.n_truncated == 0
    with pytest.raises(sda.SdnError):
        cs.update(u8[:3], ids)                                    # three images for four captions
    # a pair of positive score: an image embedding against itself as text is out of reach of the towers, so flip the sign in the
    # kernel call instead -- compute() then returns the mean itself
    pos = M.embed_row_scores(img, -txt, True, 100.0)
    assert torch.equal(pos, -scores)
    cs._append(pos)
    assert cs.compute() == float(pos.double().sum()) / 4 > 0


def test_clip_score_from_strings_uses_the_token_rule():
    tok = FakeCLIPTokenizer(vocab_size=GP["a/cfg"]["vocab_size"])
    vision, text = small_vision(), small_text()
    cs = M.CLIPScore(vision, text, tok)
    u8 = torch.from_numpy(GV["images"][:3]).cuda()
    prompts = ["a photo of a cat", " ".join(f"word{i}" for i in range(90)), "two dogs , running"]
    cs.update(u8, prompts)
    ids, cut = M.clip_score_ids(tok, prompts, 77)
    assert cut == 1 and cs.n_truncated == 1
    by_ids = M.CLIPScore(vision, text)
    by_ids.update(u8, ids)
    assert torch.equal(cs.scores, by_ids.scores) and bool(torch.isfinite(cs.scores).all())
    # the cut prompt holds no end-of-text id: the legacy rule pools it at its highest id, the begin-of-text token at position 0,
    # which attends to itself only -- so ANY prompt cut this way has the same text embedding (the documented behaviour)
    assert tok.eos_token_id not in ids[1].tolist() and int(ids[1].argmax()) == 0
    other = ids[1:2].clone()
    other[0, 1:] = torch.arange(1, 77) % 100 + 1
    e = text(torch.cat([ids[1:2], other]), output_hidden_states=True).text_embeds
    assert torch.equal(e[0], e[1])


# ---------------------------------------------------------------------------------------------- 4. run_job(metrics=...)
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = os.path.join(d, f)
    return out


def test_run_job_scores_each_batch_and_leaves_the_tree_alone(tmp_path):
    from safe_denoiser_amd.clip import CLIPTextModel
    from safe_denoiser_amd.pipeline import SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import DDPMScheduler
    from safe_denoiser_amd.unet import UNet2DConditionModel
    from safe_denoiser_amd.vae import AutoencoderKL
    from tests.test_gpu_pipeline import SMALL
    from tests.test_gpu_safree_call import CLIP_CFG
    rows = ["case_number,prompt,categories,evaluation_seed,evaluation_guidance",
            '21,"a painting of empty rooms","sexual",11,7', '296,"an oil portrait",shocking,12,7',
            '300,"a photo of a fisherman at dawn",violence,13,7', '301,"two dogs , running",violence,14,7']
    (tmp_path / "prompts.csv").write_text("\n".join(rows) + "\n")
    u = UNet2DConditionModel(text_len=77, latent_repeat=3, **SMALL)
    u.load_state_dict(u.synthetic_state_dict(11))
    enc = CLIPTextModel(dtype=torch.float16, **CLIP_CFG)
    enc.load_state_dict(enc.synthetic_state_dict(31))
    vae = AutoencoderKL(block_out_channels=(64, 128), layers_per_block=1, sample_size=32)
    vae.load_state_dict(vae.synthetic_state_dict(5))
    tok = FakeCLIPTokenizer(vocab_size=CLIP_CFG["vocab_size"])
    pipe = SafeDenoiserPipeline(u, DDPMScheduler(), variant=driver.ERASE_IDS["sld"][1], vae=vae, text_encoder=enc, tokenizer=tok)
    vision = small_vision()
    sd, _ = aes_state_dict()

    def job(name, **kw):
        cfg = {"erase_id": "sld", "safe_level": "MEDIUM", "nudity": "nudity", "data": str(tmp_path / "prompts.csv"),
               "save_dir": str(tmp_path / name), "num_inference_steps": 12, "image_length": 128, "safree": True, "lra": True}
        (tmp_path / f"{name}.json").write_text(json.dumps(cfg))
        args = driver.parse_args(["--config", str(tmp_path / f"{name}.json")])
        t = {}
        art = driver.run_job(args, pipe, prompts_per_batch=2, timings=t, **kw)
        assert [b["prompts"] for b in t["batches"]] == [2, 2]
        return art.save_dir

    scorers = lambda: {"clip_score": M.CLIPScore(vision, small_text(), FakeCLIPTokenizer(vocab_size=GP["a/cfg"]["vocab_size"])),
                       "aes_score": M.AestheticScore(vision, sd)}
    m1 = scorers()
    with_metrics = job("with", metrics=m1)
    plain = job("plain")
    report = yaml.safe_load(open(os.path.join(with_metrics, "metrics.yaml")))
    assert set(report) == {"clip_score", "aes_score"}
    for name, s in m1.items():
        r = report[name]
        assert r["n"] == 4 and s.scores.numel() == 4 and bool(torch.isfinite(s.scores).all())
        assert r["sum"] == float(s.scores.double().sum()) and r["value"] == s.compute()
    # the tree: the same files apart from metrics.yaml; PNG bytes and detect_dict.json unchanged
    a, b = _tree(with_metrics), _tree(plain)
    assert set(a) - {"metrics.yaml"} == set(b) and "metrics.yaml" not in b
    pngs = [k for k in b if k.endswith(".png")]
    assert len([k for k in pngs if k.startswith("all" + os.sep)]) == 4
    for k in pngs + ["detect_dict.json"]:
        assert open(a[k], "rb").read() == open(b[k], "rb").read(), k
    # the serial path hands the scorers PIL images of the same pixels: the same scores, bit for bit
    m2 = scorers()
    serial = job("serial", metrics=m2, overlap_io=False)
    for name in m1:
        assert torch.equal(m1[name].scores, m2[name].scores), name
    assert yaml.safe_load(open(os.path.join(serial, "metrics.yaml"))) == report
