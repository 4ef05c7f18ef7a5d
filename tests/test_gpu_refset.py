"""The negative reference set on the GPU: sdn_image_resize_rect_u8 against Pillow byte for byte at every shape of
tests_support.refset_oracle.SHAPES, its f32 planes against the existing normalise kernel, the data module's transform on PIL
images of several modes, and driver.build_repellency (eager, lazy, and assembled by hand) down to the proj_ref bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import safe_denoiser_amd as sda
from safe_denoiser_amd import clip_vision as V, data as D, driver
from safe_denoiser_amd.pipeline import make_scheduler
from safe_denoiser_amd.repellency import repellency_methods_fast as fast, repellency_methods_threshold as thr
from safe_denoiser_amd.vae import AutoencoderKL
from tests_support import refset_oracle as R

pytestmark = pytest.mark.gpu
G = R.load_golden()
NAMES = [s[0] for s in R.SHAPES]
BY_NAME = {s[0]: s for s in R.SHAPES}
HALF = (0.5, 0.5, 0.5)


def normalize_any(u8: torch.Tensor) -> torch.Tensor:
    """The existing normalise kernel on uint8 [B, H, W, 3] of any aspect ratio: it maps pixel by pixel, so a non-square image goes
    through it as B H W images of one pixel."""
    b, h, w, _ = u8.shape
    if h == w:
        return V.normalize_u8(u8, mean=HALF, std=HALF)
    flat = V.normalize_u8(u8.reshape(b * h * w, 1, 1, 3), mean=HALF, std=HALF)
    return flat.reshape(b, h, w, 3).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("name", NAMES)
def test_rect_resize_equals_pillow_byte_for_byte(name):
    _, w, h, ow, oh, b = BY_NAME[name]
    src = G["img_" + name]
    got = V.resize_rect_u8(torch.from_numpy(src).cuda(), (oh, ow), "bilinear")
    assert got.shape == (b, oh, ow, 3) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    assert np.array_equal(got, G["out_" + name])                                                   # the committed fixture
    live = np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR)) for im in src])
    assert np.array_equal(got, live)                                                               # this machine's Pillow
    assert np.array_equal(got, np.stack([R.resample(im, (oh, ow)) for im in src]))
    cub = V.resize_rect_u8(torch.from_numpy(src).cuda(), (oh, ow), "bicubic").cpu().numpy()
    assert np.array_equal(cub, np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), Image.BICUBIC)) for im in src]))


def test_square_entry_point_and_rect_entry_point_agree():
    img = torch.from_numpy(R.images_for("munch")[:, :75]).cuda()                                   # 75 x 75
    assert torch.equal(V.resize_rect_u8(img, (48, 48), "bicubic"), V.resize_u8(img, 48))


@pytest.mark.parametrize("name", NAMES)
def test_f32_planes_are_the_normalise_kernel_of_the_u8_result(name):
    _, w, h, ow, oh, b = BY_NAME[name]
    src = torch.from_numpy(G["img_" + name]).cuda()
    u8_only, none = V.resize_rect(src, (oh, ow), "bilinear")
    assert none is None
    none, f32_only = V.resize_rect(src, (oh, ow), "bilinear", mean=HALF, std=HALF, want_u8=False)
    assert none is None and f32_only.shape == (b, 3, oh, ow) and f32_only.dtype == torch.float32
    u8_both, f32_both = V.resize_rect(src, (oh, ow), "bilinear", mean=HALF, std=HALF)
    assert torch.equal(u8_both, u8_only) and torch.equal(f32_both, f32_only)
    assert torch.equal(f32_only, normalize_any(u8_only))
    # per-channel constants reach the right plane
    mean, std = (0.1, 0.4, 0.7), (0.2, 0.5, 1.5)
    got = V.resize_rect(src, (oh, ow), "bilinear", mean=mean, std=std, want_u8=False)[1]
    x = u8_only.permute(0, 3, 1, 2).float() / torch.full((1,), 255.0, device="cuda")
    want = (x - torch.tensor(mean, device="cuda").view(1, 3, 1, 1)) / torch.tensor(std, device="cuda").view(1, 3, 1, 1)
    assert torch.equal(got, want)


def test_a_table_that_names_taps_outside_the_input_is_clamped():
    """Horizontal-only 40 x 16 -> 16 x 16 with a table whose rows start before the line and run past its end: the kernel reads what
    the clamped table names.  The input sits inside a larger buffer, and the output between guard bands."""
    name = "horizontal_only"
    _, w, h, ow, oh, b = BY_NAME[name]
    coeffs, bounds, ksize = V.resize_tables(w, ow, "bilinear")
    bad = bounds.copy()
    bad[0] = (-3, ksize + 9)                                            # starts before the line, longer than ksize
    bad[-1, 1] = ksize                                                  # runs past the end of the line
    clamped = []
    for i, (lo, cnt) in enumerate(bad):
        lo = max(int(lo), 0)
        cnt = min(int(cnt), ksize, w - lo)
        clamped.append((lo, coeffs[i, :cnt].astype(np.int64)))
    want = np.stack([R._pass(im, clamped) for im in G["img_" + name]])
    pad = 4096
    src = torch.from_numpy(G["img_" + name])
    buf = torch.full((2 * pad + src.numel(),), 0x5A, dtype=torch.uint8, device="cuda")
    buf[pad:pad + src.numel()] = src.reshape(-1).cuda()
    obuf = torch.full((2 * pad + b * oh * ow * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    out = obuf[pad:pad + b * oh * ow * 3]
    cd, bd = torch.from_numpy(coeffs).cuda(), torch.from_numpy(bad).cuda()
    rc = sda.lib().sdn_image_resize_rect_u8(buf.data_ptr() + pad, b, h, w, oh, ow, cd.data_ptr(), bd.data_ptr(), ksize, None, None, 0, None,
                                            out.data_ptr(), None, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert np.array_equal(out.view(b, oh, ow, 3).cpu().numpy(), want)
    assert bool((obuf[:pad] == 0xA5).all()) and bool((obuf[pad + out.numel():] == 0xA5).all())


def _mode_images():
    rng = np.random.default_rng(77)
    rgb = Image.fromarray(rng.integers(0, 256, (45, 61, 3), dtype=np.uint8))
    gray = Image.fromarray(rng.integers(0, 256, (70, 33), dtype=np.uint8))
    rgba = Image.fromarray(rng.integers(0, 256, (32, 50, 4), dtype=np.uint8))
    pal = Image.fromarray(rng.integers(0, 256, (45, 61, 3), dtype=np.uint8)).convert("P", palette=Image.Palette.ADAPTIVE, colors=64)
    same = Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8))
    assert [im.mode for im in (rgb, gray, rgba, pal, same)] == ["RGB", "L", "RGBA", "P", "RGB"]
    return [rgb, gray, rgba, pal, pal.copy(), same]                     # two neighbours of one size share a launch


def test_transform_on_pil_images_of_every_mode():
    tf = D.get_transform(name="nudity", root="unused", class_info="unused", size=32)
    imgs = _mode_images()
    pil = [np.array(im.convert("RGB").resize((32, 32), Image.BILINEAR)) for im in imgs]          # Pillow, on the CPU
    want = torch.cat([V.normalize_u8(torch.from_numpy(p)[None].cuda(), mean=HALF, std=HALF) for p in pil])
    one_by_one = torch.stack([tf(im) for im in imgs])
    assert one_by_one.shape == (len(imgs), 3, 32, 32) and one_by_one.dtype == torch.float32 and one_by_one.is_cuda
    assert torch.equal(one_by_one, want)
    assert torch.equal(tf.batch(imgs), want)
    # torchvision's ToTensor + Normalize on the CPU, within one f32 ulp
    cpu = torch.stack([torch.from_numpy(p).permute(2, 0, 1).float().div(255).sub(.5).div(.5) for p in pil])
    got = one_by_one.cpu()
    lo, hi = torch.nextafter(cpu, torch.full_like(cpu, -4.0)), torch.nextafter(cpu, torch.full_like(cpu, 4.0))
    differing = int((got != cpu).sum())
    print(f"transform vs torch CPU ToTensor+Normalize: {differing} of {cpu.numel()} values differ")
    assert bool(((got >= lo) & (got <= hi)).all())


# ---- build_repellency -----------------------------------------------------------------------------------------------------------
SMALL = dict(block_out_channels=(64, 128), layers_per_block=1)
SIZES = [(41, 57), (41, 57), (64, 48), (32, 32), (90, 35)]             # (w, h); the first two share a launch, one needs no resize


@pytest.fixture(scope="module")
def image_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("refset")
    d = root / "cls"
    d.mkdir()
    rng = np.random.default_rng(5)
    for i, (w, h) in enumerate(SIZES):
        im = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        if i % 2:
            im.save(str(d / f"img{i}.jpg"), quality=90)
        else:
            im.save(str(d / f"img{i}.png"))
    return str(root)


@pytest.fixture(scope="module")
def pipe32():
    v = AutoencoderKL(sample_size=32, **SMALL)
    v.load_state_dict(v.synthetic_state_dict(3, with_encoder=True))
    return SimpleNamespace(vae=v, scheduler=make_scheduler("ddpm"))


def _task(root, path, n_embed, size=32, method="kernel_fast", **params):
    return {"mean_processor": {"method": "unused"},
            "data": {"name": "nudity", "root": root, "class_info": "cls", "size": size},
            "repellency": {"method": method, "n_embed": n_embed, "guidance_scale": 7.5,
                           "params": dict(proj_ref_path=path, cache_proj_ref=False, scale=0.03, sigma=1.0, epsilon=1e-8, **params)}}


@pytest.mark.parametrize("n_embed", [2, 8])
def test_build_repellency_eager_lazy_and_by_hand_give_the_same_bits(image_tree, pipe32, tmp_path, n_embed):
    args = SimpleNamespace(num_inference_steps=3)
    procs, paths = [], []
    for tag, kw in (("eager", dict(eager=True)), ("lazy", dict())):
        paths.append(str(tmp_path / f"{tag}.pt"))
        torch.manual_seed(11)
        procs.append(driver.build_repellency(args, pipe32, _task(image_tree, paths[-1], n_embed), **kw))
    # by hand, as a user of the parent commit would: CPU Pillow -> tensor -> the engine's embed_fn -> get_repellency_method
    import glob
    files = sorted(glob.glob(image_tree + "/cls/*.png") + glob.glob(image_tree + "/cls/*.jpg"))
    assert [f.rsplit("/", 1)[-1] for f in files] == ["img0.png", "img1.jpg", "img2.png", "img3.jpg", "img4.png"]
    pil = [np.asarray(Image.open(f).convert("RGB").resize((32, 32), Image.BILINEAR)) for f in files]
    ref_imgs = V.normalize_u8(torch.from_numpy(np.stack(pil)).cuda(), mean=HALF, std=HALF)
    s = pipe32.scheduler
    paths.append(str(tmp_path / "hand.pt"))
    torch.manual_seed(11)
    procs.append(thr.get_repellency_method("kernel_fast", ref_data=ref_imgs, embed_fn=pipe32.vae.embed_fn(), forward_fn=s.add_noise,
                                           num_timesteps=3, max_idx=len(s.betas), beta_min=s.beta_start, beta_max=s.beta_end,
                                           n_embed=n_embed, scheduler=s, proj_ref_path=paths[-1], cache_proj_ref=False, scale=0.03,
                                           sigma=1.0, epsilon=1e-8))
    refs = [p.proj_refs for p in procs]
    assert refs[0].shape == (5, 4, 16, 16) and refs[0].is_cuda
    assert torch.equal(refs[0], refs[2]) and torch.equal(refs[1], refs[2])
    for p, path in zip(procs, paths):
        assert torch.equal(torch.load(path), p.proj_refs.cpu())
    norm = refs[1].double().norm(dim=1)
    assert float((norm - 1).abs().max()) <= 4 * 2.0 ** -24              # x / ||x||, both f32-rounded: a few units of 2^-24
    assert procs[0].beta_threshold == procs[1].beta_threshold == procs[2].beta_threshold
    x = torch.randn(1, 4, 16, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    outs = [p.conditioning(x.clone()) for p in procs[:2]]
    assert torch.equal(outs[0]["x_0_hat"], outs[1]["x_0_hat"]) and bool(torch.isfinite(outs[1]["x_0_hat"]).all())


def test_build_repellency_takes_another_front_end_and_requires_mean_processor(image_tree, pipe32, tmp_path):
    args = SimpleNamespace(num_inference_steps=3)
    task = _task(image_tree, str(tmp_path / "fast.pt"), 2)
    torch.manual_seed(11)
    p_fast = driver.build_repellency(args, pipe32, task, get_repellency_method=fast.get_repellency_method)
    torch.manual_seed(11)
    p_thr = driver.build_repellency(args, pipe32, _task(image_tree, str(tmp_path / "thr.pt"), 2))
    assert type(p_fast).__module__.endswith("repellency_methods_fast") and torch.equal(p_fast.proj_refs, p_thr.proj_refs)
    del task["mean_processor"]
    with pytest.raises(KeyError):
        driver.build_repellency(args, pipe32, task)


def test_lazy_set_slices_are_the_eager_rows(image_tree):
    cfg = {"name": "nudity", "root": image_tree, "class_info": "cls"}
    tf = D.get_transform(**cfg, size=32)
    ds = D.get_dataset(**cfg, transforms=tf)
    eager = D.get_all_imgs(D.get_dataloader(ds, batch_size=1, num_workers=0, train=False))
    assert eager.shape == (5, 3, 32, 32)
    by_batches = torch.cat(list(D.get_dataloader(ds, batch_size=2, num_workers=0, train=False, decode_threads=1)))
    assert torch.equal(by_batches, eager)
    lazy = D.get_all_imgs(D.get_dataloader(ds, batch_size=1, num_workers=0, train=False), lazy=True)
    assert len(lazy) == 5 and lazy.device.type == eager.device.type == "cuda" and lazy.dtype == torch.float32
    assert torch.equal(lazy[1:4], eager[1:4]) and torch.equal(lazy[3:99], eager[3:]) and torch.equal(lazy[0:5], eager)
    assert torch.equal(lazy[-1], eager[-1]) and lazy[2:2].shape == (0, 3, 32, 32)
    assert torch.equal(ds[2], eager[2])


def test_lazy_set_never_holds_the_whole_stack(tmp_path):
    m, size, n_embed = 12, 64, 2
    d = tmp_path / "root" / "cls"
    d.mkdir(parents=True)
    rng = np.random.default_rng(9)
    for i in range(m):
        w, h = 70 + 3 * (i % 4), 90 - 5 * (i % 3)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(d / f"{i:02d}.png"))
    v = AutoencoderKL(sample_size=size, **SMALL)
    v.load_state_dict(v.synthetic_state_dict(3, with_encoder=True))
    pipe = SimpleNamespace(vae=v, scheduler=make_scheduler("ddpm"))
    task = _task(str(tmp_path / "root"), str(tmp_path / "refs.pt"), n_embed, size=size, beta_threshold=1.0)
    proc = driver.build_repellency(SimpleNamespace(num_inference_steps=3), pipe, task)      # the warm-up: tables, workspaces, pool
    lazy = proc.ref_data
    assert isinstance(lazy, D.LazyRefImages) and len(lazy) == m
    eager_bytes = m * 3 * size * size * 4
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = proc.project(lazy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"lazy project: peak {peak} bytes above the baseline; the eager stack alone is {eager_bytes} bytes")
    assert out.shape[0] == m and peak < eager_bytes


def test_other_ranks_build_around_the_broadcast_and_touch_no_file(image_tree, pipe32, tmp_path, monkeypatch):
    """Rank 1 of 2 with the collective replaced by rank 0's tensor: no image directory is read (it does not exist here), no cache
    file is written, and the processor carries rank 0's proj_ref and calibrates to the same threshold."""
    import os
    from safe_denoiser_amd import dist as sdist
    args = SimpleNamespace(num_inference_steps=3)
    torch.manual_seed(11)
    p0 = driver.build_repellency(args, pipe32, _task(image_tree, str(tmp_path / "rank0.pt"), 2), rank=0, world=1)
    seen = []

    def fake_broadcast(refs, device, src=0):
        seen.append(refs)
        return p0.proj_refs.clone() if refs is None else refs
    monkeypatch.setattr(sdist, "broadcast_proj_ref", fake_broadcast)
    never = str(tmp_path / "rank1" / "never.pt")
    p1 = driver.build_repellency(args, pipe32, _task(str(tmp_path / "no_such_root"), never, 2), rank=1, world=2)
    assert seen == [None] and torch.equal(p1.proj_refs, p0.proj_refs) and p1.beta_threshold == p0.beta_threshold
    assert not os.path.exists(never) and not os.path.exists(os.path.dirname(never))
    torch.manual_seed(11)
    p0b = driver.build_repellency(args, pipe32, _task(image_tree, str(tmp_path / "rank0b.pt"), 2), rank=0, world=2)
    assert len(seen) == 2 and seen[1] is p0b.proj_refs and torch.equal(p0b.proj_refs, p0.proj_refs) and os.path.exists(str(tmp_path / "rank0b.pt"))
