"""Writes refset_golden.npz: for every row of tests_support.refset_oracle.SHAPES the seeded synthetic uint8 batch (`img_<name>`,
[B, in_h, in_w, 3]) and what Pillow itself makes of it, `Image.resize((out_w, out_h), BILINEAR)` (`out_<name>`, [B, out_h, out_w, 3]),
plus the Pillow version that produced them.  CPU only:  python tests/golden/make_refset_golden.py"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests_support import refset_oracle as R  # noqa: E402


def main():
    out = {"pillow_version": np.asarray(PIL.__version__)}
    for name, w, h, ow, oh, b in R.SHAPES:
        imgs = R.images_for(name)
        assert imgs.shape == (b, h, w, 3)
        out["img_" + name] = imgs
        out["out_" + name] = np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR)) for im in imgs])
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
