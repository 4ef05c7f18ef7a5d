"""Host-side restatement of PIL.Image.resize((out_w, out_h), BILINEAR | BICUBIC) for RGB uint8 images of any aspect ratio, in
numpy integers, and the shapes and seeded images the negative-reference-set tests share.  Checked against Pillow itself in
tests/test_refset_host.py, so that GPU tests may use it for shapes the fixture does not hold."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tests", "golden", "refset_golden.npz")

# (name, in_w, in_h, out_w, out_h, batch): the smallest that reach every branch of the two-pass resample
SHAPES = [
    ("down_tall", 37, 53, 16, 16, 1),            # non-integer downscale, ksize differs per axis
    ("down_wide", 53, 37, 16, 16, 1),
    ("munch", 75, 100, 48, 48, 1),               # the 3:4 aspect of the shipped set
    ("up", 7, 5, 16, 16, 1),                     # upscale: the support stays 1
    ("vertical_only", 16, 40, 16, 16, 1),        # horizontal pass skipped
    ("horizontal_only", 40, 16, 16, 16, 1),      # vertical pass skipped
    ("copy", 16, 16, 16, 16, 1),
    ("one_pixel_axis", 1, 9, 4, 4, 1),
    ("rect_out", 33, 21, 24, 40, 1),
    ("batched", 37, 53, 16, 16, 3),
]


def images_for(name: str) -> np.ndarray:
    """The seeded uint8 batch [B, in_h, in_w, 3] of one SHAPES row: noise with a smooth ramp mixed in."""
    i = [s[0] for s in SHAPES].index(name)
    _, w, h, _, _, b = SHAPES[i]
    rng = np.random.default_rng(1000 + i)
    noise = rng.integers(0, 256, (b, h, w, 3)).astype(np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 127 + 127 * np.cos((x + y) / 5.0)], -1)
    return np.clip(0.6 * noise + 0.4 * ramp[None], 0, 255).astype(np.uint8)


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


_FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def tables(n_in: int, n_out: int, filter: str = "bilinear"):
    """Per output index: (xmin, integer taps scaled by 2^22) -- everything in double, the taps summed in tap order and each
    divided by the sum, then rounded half away from zero."""
    fn, radius = _FILTERS[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = radius * fs
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = [fn((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax - xmin)]
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = [v / tot for v in w]
        k = [int((-0.5 if v < 0 else 0.5) + v * 2.0 ** 22) for v in w]
        out.append((xmin, np.asarray(k, dtype=np.int64)))
    return out


def _pass(img: np.ndarray, tabs) -> np.ndarray:
    """One pass along axis 1 of img [rows, n_in, ch] uint8 -> [rows, n_out, ch] uint8."""
    out = np.empty((img.shape[0], len(tabs), img.shape[2]), dtype=np.uint8)
    src = img.astype(np.int64)
    for i, (xmin, k) in enumerate(tabs):
        acc = (src[:, xmin:xmin + len(k)] * k[None, :, None]).sum(axis=1) + (1 << 21)
        out[:, i] = np.clip(acc >> 22, 0, 255)
    return out


def resample(img: np.ndarray, size, filter: str = "bilinear") -> np.ndarray:
    """Image.resize of one uint8 image [H, W, 3] to size = (out_h, out_w): the horizontal pass (only when the width changes),
    rounded to uint8, then the vertical pass (only when the height changes) over that intermediate."""
    out_h, out_w = size
    h, w = img.shape[:2]
    cur = img
    if w != out_w:
        cur = _pass(cur, tables(w, out_w, filter))
    if h != out_h:
        cur = _pass(np.ascontiguousarray(cur.transpose(1, 0, 2)), tables(h, out_h, filter)).transpose(1, 0, 2)
    return np.array(cur, dtype=np.uint8, order="C")


def load_golden():
    return np.load(GOLDEN)
