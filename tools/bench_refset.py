#!/usr/bin/env python3
"""Wall time of building the negative reference set from an image directory: N synthetic 800 x 1067 JPEGs (the size of the
reference's munch set) written to a temporary directory, then `ref_imgs` f32 [N, 3, 512, 512] on the GPU built three ways --
Pillow's resize + a numpy normalise on one CPU thread (what there was before safe_denoiser_amd.data), the engine's transform with
one decode thread, and with the decode pool -- plus the parts on their own (JPEG decode alone, the GPU transform alone on decoded
arrays) and the whole driver.build_repellency with an SD-v1.4-sized VAE encoder on synthetic weights.  Every timed region follows a
warm-up run and sits between two device synchronisations.  Recorded, not gated: writes profiles/refset_build.json."""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_denoiser_amd import data as D, driver  # noqa: E402
from safe_denoiser_amd.pipeline import make_scheduler  # noqa: E402
from safe_denoiser_amd.vae import AutoencoderKL  # noqa: E402


def write_jpegs(root, n, w, h):
    d = os.path.join(root, "cls")
    os.makedirs(d)
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    for i in range(n):
        base = np.stack([127 + 120 * np.sin(x / (17.0 + i % 7)), 255 * y / h, 127 + 120 * np.cos((x + y) / (29.0 + i % 5))], -1)
        img = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)          # photograph-like: smooth + grain
        Image.fromarray(img).save(os.path.join(d, f"{i:04d}.jpg"), quality=90)
    return d


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def cpu_pillow(paths, size):
    out = np.empty((len(paths), 3, size, size), dtype=np.float32)
    for i, p in enumerate(paths):
        a = np.asarray(Image.open(p).convert("RGB").resize((size, size), Image.BILINEAR), dtype=np.float32)
        out[i] = ((a / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)
    return torch.from_numpy(out).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=1067)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--n-embed", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refset_build.json"))
    args = ap.parse_args()
    res = {"images": args.images, "source": [args.width, args.height], "size": args.size, "n_embed": args.n_embed,
           "device": torch.cuda.get_device_name(0), "decode_threads_pooled": D.decode_workers()}
    with tempfile.TemporaryDirectory(prefix="sdn_refset_") as root:
        t0 = time.perf_counter()
        write_jpegs(root, args.images, args.width, args.height)
        res["write_jpegs_s"] = time.perf_counter() - t0
        cfg = {"name": "nudity", "root": root, "class_info": "cls", "size": args.size}
        tf = D.get_transform(**cfg)
        ds = D.get_dataset("nudity", root, class_info="cls", transforms=tf)
        paths = ds.fpaths

        def engine(threads, n=None):
            loader = D.get_dataloader(ds, batch_size=1, num_workers=0, train=False, decode_threads=threads)
            out = loader.images(0, len(ds) if n is None else n)
            loader.close()
            return out

        # warm-up: page cache, tables, allocator, pool start-up
        cpu_pillow(paths[:16], args.size)
        engine(1, 16)
        engine(None, 16)
        res["cpu_pillow_1thread_s"], a = wall(lambda: cpu_pillow(paths, args.size))
        res["engine_decode_1thread_s"], b = wall(lambda: engine(1))
        res["engine_decode_pooled_s"], c = wall(lambda: engine(None))
        res["engine_equals_cpu_pillow"] = bool(torch.equal(a, b)) and bool(torch.equal(b, c))
        res["max_abs_diff_vs_cpu_pillow"] = float((a - b).abs().max())
        del a, b, c
        # the parts: decode alone on one thread; the GPU transform alone on the decoded arrays
        t0 = time.perf_counter()
        arrays = [tf.to_array(ds.load(i)) for i in range(len(ds))]
        res["decode_only_1thread_s"] = time.perf_counter() - t0
        tf.arrays(arrays[:16])
        res["gpu_transform_only_s"] = wall(lambda: tf.arrays(arrays))[0]
        t0 = time.perf_counter()
        for arr in arrays:
            Image.fromarray(arr).resize((args.size, args.size), Image.BILINEAR)
        res["cpu_resize_only_1thread_s"] = time.perf_counter() - t0
        del arrays
        # the whole build: images -> VAE encoder -> proj_ref, lazy and eager
        vae = AutoencoderKL()
        vae._encoder().load_synthetic_on_device(4321, device="cuda")       # only the encoder half runs here
        pipe = SimpleNamespace(vae=vae, scheduler=make_scheduler("ddpm"))
        margs = SimpleNamespace(num_inference_steps=50)

        def task(path):
            return {"mean_processor": {}, "data": cfg,
                    "repellency": {"method": "kernel_fast", "n_embed": args.n_embed,
                                   "params": dict(proj_ref_path=path, cache_proj_ref=False, scale=0.03, sigma=1.0, beta_threshold=1.0)}}
        old_cap = D.MAX_NUDITY_FILES
        D.MAX_NUDITY_FILES = 2 * args.n_embed                          # warm-up on two chunks: encoder workspace, first-launch costs
        driver.build_repellency(margs, pipe, task(os.path.join(root, "warm.pt")))
        D.MAX_NUDITY_FILES = old_cap
        for tag, eager in (("lazy", False), ("eager", True)):
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            res[f"build_repellency_{tag}_s"], proc = wall(
                lambda: driver.build_repellency(margs, pipe, task(os.path.join(root, f"{tag}.pt")), eager=eager))
            res[f"build_repellency_{tag}_peak_bytes_above_start"] = torch.cuda.max_memory_allocated() - base
            assert proc.proj_refs.shape[0] == args.images
            del proc
    print(json.dumps(res, indent=1, sort_keys=True))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
