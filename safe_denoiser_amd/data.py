"""The negative reference images of a repellency job: the reference's data/dataloader.py under its own names and call shapes
(run_nudity.py:299-305 reads unchanged), without torchvision.

    transform = get_transform(**data_config)                        # data_config = the task YAML's `data:` section
    dataset = get_dataset(**data_config, transforms=transform)
    loader = get_dataloader(dataset, batch_size=1, num_workers=0, train=False)
    ref_imgs = get_all_imgs(loader)                                 # f32 [M, 3, 512, 512] on the GPU, in file order

The transform there is torchvision's Resize((512, 512)) + ToTensor + Normalize(.5, .5) on a PIL image, i.e.
`Image.resize((512, 512), BILINEAR)` followed by ((u8 / 255) - .5) / .5.  JPEG / PNG decoding stays on the CPU with PIL (a small
thread pool; PIL releases the GIL while it decodes); the resize and the affine map run on the GPU in one entry point
(sdn_image_resize_rect_u8), bit for bit what Pillow and sdn_clip_normalize_u8 produce.  Images keep their own sizes until then:
neighbours of one size share a launch, every other image has its own.

`get_all_imgs(loader, lazy=True)` returns the same set as an object that decodes and transforms only the slice it is asked for:
RepellencyEngine.project slices its `ref_data` in chunks of `n_embed`, so the [M, 3, 512, 512] stack (about 10 GB for the
reference's cap of 3200 images) is never resident, and `proj_ref` has the same bits as with the eager tensor.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from .clip_vision import resize_rect

MAX_NUDITY_FILES = 3200                                            # "VRAM out of memory" cap of the reference (dataloader.py:63-65)
MAX_DECODE_WORKERS = 16
DECODE_WINDOW = 64                                                 # images decoded ahead of the GPU transform

__DATASET__ = {}


def register_dataset(name: str):
    def wrapper(cls):
        if __DATASET__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        __DATASET__[name] = cls
        return cls
    return wrapper


def get_dataset(name: str, root: str, **kwargs):
    if __DATASET__.get(name, None) is None:
        raise NameError(f"Dataset {name} is not defined.")
    return __DATASET__[name](root=root, **kwargs)


def decode_workers(requested: Optional[int] = None) -> int:
    """Threads of the decode pool: at most 16 and at most the CPUs there are (the machine may have many more than this
    process may use, so the count alone never sizes it)."""
    cap = max(1, min(MAX_DECODE_WORKERS, os.cpu_count() or 1))
    return cap if not requested or requested < 0 else min(int(requested), cap)


# ---- transform ------------------------------------------------------------------------------------------------------------------
class RefTransform:
    """PIL image -> f32 [3, size, size] on the GPU: `.convert('RGB')` (a no-op for what the datasets hand over), Resize((size, size))
    with Pillow's bilinear filter, ToTensor, Normalize(.5, .5).  `batch` takes several images at once."""

    mean = (0.5, 0.5, 0.5)
    std = (0.5, 0.5, 0.5)

    def __init__(self, size: int = 512, device="cuda"):
        self.size, self.device = int(size), torch.device(device)

    @staticmethod
    def to_array(img) -> np.ndarray:
        return np.asarray(img.convert("RGB"), dtype=np.uint8)

    def arrays(self, arrays) -> torch.Tensor:
        """uint8 [H, W, 3] host arrays of any sizes -> f32 [n, 3, size, size], in order; one launch per run of equal sizes."""
        _lib.require_gpu()
        parts, run = [], []

        def flush():
            u8 = torch.from_numpy(np.stack(run)).to(self.device)
            parts.append(resize_rect(u8, (self.size, self.size), "bilinear", mean=self.mean, std=self.std, want_u8=False)[1])
        for a in arrays:
            if run and run[-1].shape != a.shape:
                flush()
                run = []
            run.append(a)
        if run:
            flush()
        if not parts:
            return torch.empty((0, 3, self.size, self.size), dtype=torch.float32, device=self.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def batch(self, images) -> torch.Tensor:
        return self.arrays([self.to_array(im) for im in images])

    def __call__(self, img) -> torch.Tensor:
        return self.batch([img])[0]


def get_transform(name: str, size: int = 512, device="cuda", **kwargs):
    """`get_transform(**data_config)`: `name` and every other key of the section (`root`, `class_info`) are accepted and unused, as
    in the reference.  `size` and `device` are the engine's own (the reference's side is fixed at 512)."""
    return RefTransform(size=size, device=device)


# ---- datasets -------------------------------------------------------------------------------------------------------------------
class _ImageFiles:
    def __init__(self, root: str, transforms: Optional[Callable] = None):
        self.root, self.transforms = root, transforms
        self.fpaths = []

    def __len__(self):
        return len(self.fpaths)

    def load(self, index: int):
        from PIL import Image
        with Image.open(self.fpaths[index]) as im:
            return im.convert("RGB")

    def __getitem__(self, index: int):
        img = self.load(index)
        if self.transforms is not None:
            img = self.transforms(img)
        return img


@register_dataset(name="nudity")
@register_dataset(name="inappropriate")
class NudityDataset(_ImageFiles):
    def __init__(self, root: str, class_info: str, transforms: Optional[Callable] = None):
        super().__init__(root, transforms)
        root_path = os.path.join(root, class_info)
        # ONE sort over both lists (dataloader.py:60-61): a.jpg comes before b.png
        self.fpaths = sorted(glob(f"{root_path}/*.png", recursive=True) + glob(f"{root_path}/*.jpg", recursive=True))
        if len(self.fpaths) > MAX_NUDITY_FILES:
            self.fpaths = self.fpaths[:MAX_NUDITY_FILES]
        assert len(self.fpaths) > 0, "File list is empty. Check the root."


@register_dataset(name="artists")
class ArtistsDataset(_ImageFiles):
    def __init__(self, root: str, class_info: str, transforms: Optional[Callable] = None):
        super().__init__(root, transforms)
        root_path = os.path.join(root, class_info)
        self.fpaths = sorted(glob(f"{root_path}/*.png", recursive=True))
        assert len(self.fpaths) > 0, "File list is empty. Check the root."


# ---- loader ---------------------------------------------------------------------------------------------------------------------
class RefLoader:
    """`DataLoader(dataset, batch_size, shuffle=False, drop_last=False)`: batches [b, 3, size, size] in file order.  `images(lo, hi)`
    is what both the iterator and the lazy set are made of: decode on the pool, consume in order, transform on the GPU."""

    def __init__(self, dataset, batch_size: int = 1, workers: Optional[int] = None):
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        self.dataset, self.batch_size, self.workers = dataset, int(batch_size), decode_workers(workers)
        self._pool = None

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def _map(self, fn, items):
        if self.workers <= 1 or len(items) <= 1:
            return [fn(i) for i in items]
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="sdn-decode")
        return list(self._pool.map(fn, items))                     # results in the order of `items`

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def images(self, lo: int, hi: int) -> torch.Tensor:
        ds, tf = self.dataset, self.dataset.transforms
        idx = list(range(lo, hi))
        if isinstance(tf, RefTransform) and hasattr(ds, "load"):
            # a window of decoded images at a time: the host never holds more than DECODE_WINDOW full-size images
            def window(w):
                return tf.arrays(self._map(lambda i: tf.to_array(ds.load(i)), idx[w:w + DECODE_WINDOW]))
            if len(idx) <= DECODE_WINDOW:
                return window(0)
            out = torch.empty((len(idx), 3, tf.size, tf.size), dtype=torch.float32, device=tf.device)
            for w in range(0, len(idx), DECODE_WINDOW):
                out[w:w + DECODE_WINDOW] = window(w)
            return out
        if tf is None:
            raise _lib.SdnError("the dataset has no transform: pass transforms=get_transform(...) to get_dataset")
        return torch.stack([ds[i] for i in idx])                   # a foreign transform: whatever it returns, stacked

    def __iter__(self):
        n = len(self.dataset)
        for lo in range(0, n, self.batch_size):
            yield self.images(lo, min(lo + self.batch_size, n))


def get_dataloader(dataset, batch_size: int, num_workers: int, train: bool, decode_threads: Optional[int] = None):
    """`num_workers` is the reference's DataLoader argument (process workers; the drivers pass 0) and is accepted and unused: decoding
    runs on `decode_threads` threads (default: min(16, CPUs))."""
    if train:
        raise NotImplementedError("train=True (shuffle + drop_last) is not implemented: the drivers only read the set in order")
    return RefLoader(dataset, batch_size, decode_threads)


class LazyRefImages:
    """The set `get_all_imgs` would return, not materialised: len(), .device / .dtype / .shape, and slices that decode and
    transform only the images they cover."""

    dtype = torch.float32

    def __init__(self, loader: RefLoader):
        tf = loader.dataset.transforms
        if not isinstance(tf, RefTransform):
            raise _lib.SdnError("a lazy set needs the dataset's transform to be get_transform(...)'s")
        self.loader, self.device = loader, tf.device
        self.shape = (len(loader.dataset), 3, tf.size, tf.size)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        n = len(self)
        if isinstance(key, slice):
            lo, hi, step = key.indices(n)
            if step != 1:
                raise IndexError("only contiguous slices are implemented")
            return self.loader.images(lo, max(lo, hi))
        i = int(key)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(f"index {key} out of range for {n} images")
        return self.loader.images(i, i + 1)[0]


def get_all_imgs(dataloader, lazy: bool = False):
    """f32 [M, 3, size, size] on the GPU in file order; with lazy=True a LazyRefImages over the same files."""
    if lazy:
        return LazyRefImages(dataloader)
    if isinstance(dataloader, RefLoader):
        # one pass over the whole set: the pool decodes ahead across batch boundaries, the result is the concatenation of the batches
        out = dataloader.images(0, len(dataloader.dataset))
        dataloader.close()
        return out
    return torch.cat([images for images in dataloader], dim=0)
