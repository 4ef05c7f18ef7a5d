"""Host-side checks of the negative-reference-set loader: the bilinear coefficient tables and the numpy restatement of the two-pass
resample against Pillow itself and against the committed fixture, the generalised table builder against the bicubic tables it
replaces, the argument refusals of sdn_image_resize_rect_u8, and the dataset listing / registry of safe_denoiser_amd.data.  No GPU."""
import numpy as np
import pytest
from PIL import Image

import safe_denoiser_amd as sda
from safe_denoiser_amd import clip_vision as V, data as D
from tests_support import clip_vision_oracle as CO, refset_oracle as R

G = R.load_golden()
NAMES = [s[0] for s in R.SHAPES]
BY_NAME = {s[0]: s for s in R.SHAPES}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_holds_the_seeded_images_and_what_pillow_makes_of_them(name):
    _, w, h, ow, oh, b = BY_NAME[name]
    imgs = R.images_for(name)
    assert G["img_" + name].shape == (b, h, w, 3) and G["img_" + name].dtype == np.uint8 and np.array_equal(G["img_" + name], imgs)
    assert G["out_" + name].shape == (b, oh, ow, 3)
    for im, want in zip(imgs, G["out_" + name]):
        assert np.array_equal(np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR)), want)


@pytest.mark.parametrize("name", NAMES)
def test_numpy_oracle_equals_pillow(name):
    _, w, h, ow, oh, b = BY_NAME[name]
    for im, want in zip(G["img_" + name], G["out_" + name]):
        assert np.array_equal(R.resample(im, (oh, ow), "bilinear"), want)
        bic = np.asarray(Image.fromarray(im).resize((ow, oh), Image.BICUBIC))
        assert np.array_equal(R.resample(im, (oh, ow), "bicubic"), bic)


def _apply_tables(img, size):
    """The two passes from safe_denoiser_amd's own tables (what the kernel is given), skipping an axis that keeps its length."""
    oh, ow = size
    cur = img
    for axis_in, axis_out, horizontal in ((img.shape[1], ow, True), (img.shape[0], oh, False)):
        if axis_in == axis_out:
            continue
        coeffs, bounds, ksize = V.resize_tables(axis_in, axis_out, "bilinear")
        assert coeffs.shape == (axis_out, ksize) and bounds.shape == (axis_out, 2) and coeffs.dtype == bounds.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= axis_in).all() and (bounds[:, 1] <= ksize).all()
        tabs = [(int(lo), coeffs[i, :n].astype(np.int64)) for i, (lo, n) in enumerate(bounds)]
        assert all(not coeffs[i, n:].any() for i, (_, n) in enumerate(bounds))
        cur = R._pass(cur, tabs) if horizontal else R._pass(np.ascontiguousarray(cur.transpose(1, 0, 2)), tabs).transpose(1, 0, 2)
    return np.ascontiguousarray(cur)


@pytest.mark.parametrize("name", NAMES)
def test_bilinear_tables_equal_pillow(name):
    _, w, h, ow, oh, b = BY_NAME[name]
    for im, want in zip(G["img_" + name], G["out_" + name]):
        assert np.array_equal(_apply_tables(im, (oh, ow)), want)


def test_bilinear_ksize_follows_the_axis_scale():
    assert V.resize_tables(53, 16, "bilinear")[2] == 9 and V.resize_tables(37, 16, "bilinear")[2] == 7      # ceil(scale) * 2 + 1
    assert V.resize_tables(5, 16, "bilinear")[2] == 3 and V.resize_tables(1, 4, "bilinear")[2] == 3           # upscale: support 1


@pytest.mark.parametrize("src,dst", [(80, 56), (512, 224), (300, 224), (160, 224), (37, 16), (7, 16)])
def test_generalised_builder_keeps_the_bicubic_tables(src, dst):
    """Positional call = the old signature = bicubic; equal to the independent restatement of the bicubic tables, bit for bit."""
    coeffs, bounds, ksize = V.resize_tables(src, dst)
    c2, b2, k2 = V.resize_tables(src, dst, "bicubic")
    assert ksize == k2 and np.array_equal(coeffs, c2) and np.array_equal(bounds, b2)
    tables = CO.pillow_tables(src, dst)
    assert len(tables) == dst
    for i, (xmin, k) in enumerate(tables):
        assert bounds[i, 0] == xmin and bounds[i, 1] == len(k) <= ksize
        assert coeffs[i, :len(k)].tolist() == k.tolist() and not coeffs[i, len(k):].any()
    with pytest.raises(sda.SdnError):
        V.resize_tables(src, dst, "lanczos")


def test_rect_resize_rejects_bad_arguments_on_host():
    lib = sda.lib()
    A, CX, BX, CY, BY, T, U, F = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000

    def rs(src=A, b=2, ih=53, iw=37, oh=16, ow=24, cx=CX, bx=BX, kx=7, cy=CY, by=BY, ky=9, tmp=T, u8=U, f32=F, std=0.5):
        return lib.sdn_image_resize_rect_u8(src, b, ih, iw, oh, ow, cx, bx, kx, cy, by, ky, tmp, u8, f32, 0.5, 0.5, 0.5, std, 0.5, 0.5, None)
    assert rs(src=None) == -1 and rs(u8=None, f32=None) == -1 and rs(b=-1) == -1
    assert rs(ih=0) == -1 and rs(iw=0) == -1 and rs(oh=0) == -1 and rs(ow=0) == -1
    assert rs(ih=16385) == -1 and rs(iw=16385) == -1 and rs(oh=16385) == -1 and rs(ow=16385) == -1
    assert rs(kx=0) == -1 and rs(ky=0) == -1 and rs(kx=4097) == -1 and rs(ky=4097) == -1
    assert rs(cx=None) == -1 and rs(bx=None) == -1 and rs(cy=None) == -1 and rs(by=None) == -1       # a changing axis needs its tables
    assert rs(cx=CX + 2) == -1 and rs(bx=BX + 1) == -1 and rs(cy=CY + 2) == -1 and rs(by=BY + 3) == -1 and rs(f32=F + 2) == -1
    assert rs(tmp=None) == -1                                                                        # both passes run
    assert rs(std=0.0) == -1 and rs(std=-1.0) == -1 and rs(std=float("nan")) == -1
    assert rs(iw=24) == -1 and rs(ih=16) == -1                          # an axis that keeps its length takes NULL tables, not identity taps
    # batch == 0 returns OK without a launch, for every combination of passes and outputs
    assert rs(b=0) == 0 and rs(b=0, u8=None) == 0 and rs(b=0, f32=None) == 0
    assert rs(b=0, iw=24, cx=None, bx=None, kx=0, tmp=None) == 0 and rs(b=0, ih=16, cy=None, by=None, ky=0, tmp=None) == 0
    assert rs(b=0, iw=24, ih=16, cx=None, bx=None, cy=None, by=None, tmp=None) == 0
    # the square entry point stands as it was
    assert lib.sdn_image_resize_u8(A, 0, 80, 56, CX, BX, 7, T, U, None) == 0 and lib.sdn_image_resize_u8(None, 2, 80, 56, CX, BX, 7, T, U, None) == -1


# ---- datasets -------------------------------------------------------------------------------------------------------------------
def _write(path, size=(5, 4), fmt=None):
    Image.fromarray(np.full((size[1], size[0], 3), 90, np.uint8)).save(path, format=fmt)


def _tree(tmp_path, names):
    d = tmp_path / "root" / "cls"
    d.mkdir(parents=True)
    for n in names:
        _write(str(d / n))
    return str(tmp_path / "root")


def _base(ds):
    return [p.rsplit("/", 1)[-1] for p in ds.fpaths]


def test_nudity_listing_is_one_sort_over_both_extensions(tmp_path):
    root = _tree(tmp_path, ["b.png", "a.jpg", "d.jpg", "c.png", "e.jpeg", "f.txt.png"])
    for name in ("nudity", "inappropriate"):
        ds = D.get_dataset(name, root, class_info="cls")
        assert _base(ds) == ["a.jpg", "b.png", "c.png", "d.jpg", "f.txt.png"] and len(ds) == 5       # not pngs first; .jpeg is not listed
    im = ds[0]                                                          # no transform: the PIL image, converted
    assert im.mode == "RGB" and im.size == (5, 4)


def test_artists_listing_ignores_jpg_and_has_no_cap(tmp_path, monkeypatch):
    root = _tree(tmp_path, ["b.png", "a.jpg", "c.png", "a.png"])
    monkeypatch.setattr(D, "MAX_NUDITY_FILES", 2)
    assert _base(D.get_dataset("artists", root, class_info="cls")) == ["a.png", "b.png", "c.png"]


def test_nudity_listing_is_cut_to_the_first_files(tmp_path, monkeypatch):
    assert D.MAX_NUDITY_FILES == 3200                                   # dataloader.py:64
    root = _tree(tmp_path, ["e.png", "a.jpg", "d.jpg", "c.png", "b.png"])
    monkeypatch.setattr(D, "MAX_NUDITY_FILES", 3)
    assert _base(D.get_dataset("nudity", root, class_info="cls")) == ["a.jpg", "b.png", "c.png"]
    monkeypatch.setattr(D, "MAX_NUDITY_FILES", 5)
    assert len(D.get_dataset("nudity", root, class_info="cls")) == 5


def test_empty_directory_asserts_with_the_reference_message(tmp_path):
    root = _tree(tmp_path, [])
    for name in ("nudity", "inappropriate", "artists"):
        with pytest.raises(AssertionError, match="File list is empty. Check the root."):
            D.get_dataset(name, root, class_info="cls")
    root2 = _tree(tmp_path / "x", ["only.jpg"])
    with pytest.raises(AssertionError, match="File list is empty"):
        D.get_dataset("artists", root2, class_info="cls")


def test_registry_name_errors():
    with pytest.raises(NameError, match="Dataset coco is not defined."):
        D.get_dataset("coco", "/nowhere", class_info="x")
    with pytest.raises(NameError, match="Name nudity is already registered!"):
        D.register_dataset("nudity")(object)
    assert sorted(D.__DATASET__) == ["artists", "inappropriate", "nudity"]
    assert D.__DATASET__["nudity"] is D.__DATASET__["inappropriate"] is not D.__DATASET__["artists"]


def test_get_transform_swallows_the_data_section(tmp_path):
    cfg = {"name": "nudity", "root": _tree(tmp_path, ["a.png"]), "class_info": "cls"}
    tf = D.get_transform(**cfg)
    assert callable(tf) and tf.size == 512
    assert D.get_transform(**cfg, size=32).size == 32
    ds = D.get_dataset(**cfg, transforms=tf)
    assert ds.transforms is tf and len(ds) == 1
    loader = D.get_dataloader(ds, batch_size=1, num_workers=0, train=False)
    assert len(loader) == 1
    lazy = D.get_all_imgs(loader, lazy=True)                            # nothing is decoded or launched yet
    assert len(lazy) == 1 and lazy.shape == (1, 3, 512, 512) and str(lazy.device).startswith("cuda")
    with pytest.raises(NotImplementedError):
        D.get_dataloader(ds, batch_size=1, num_workers=0, train=True)


def test_decode_pool_is_capped(monkeypatch):
    import os
    monkeypatch.setattr(os, "cpu_count", lambda: 384)
    assert D.decode_workers() == 16 and D.decode_workers(64) == 16 and D.decode_workers(1) == 1
    monkeypatch.setattr(os, "cpu_count", lambda: 4)
    assert D.decode_workers() == 4 and D.decode_workers(16) == 4
    monkeypatch.setattr(os, "cpu_count", lambda: None)
    assert D.decode_workers() == 1
