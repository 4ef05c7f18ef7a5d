#!/usr/bin/env python3
"""Generates the CLIP vision / Q16 fixture: a small randomly initialised transformers.CLIPVisionModelWithProjection (third party;
arithmetically the OpenAI ViT tower the reference's Q16 classifier calls as `clip_model.encode_image`): hidden 128, 2 heads, 2
layers, 56 x 56 images in 14 x 14 patches (17 tokens), projection_dim 64, quick_gelu.  Stored: the state dict, 6 uint8 images
[6, 80, 80, 3] (noise, gradients, blobs), their Pillow-resized 56 x 56 bytes, pixel_values, the fp32 last_hidden_state and
image_embeds, the distance of transformers' OWN bf16 / fp16 runs from those (the error a 16-bit implementation is allowed), and two
"prompt" vectors with their fp32 similarities.  The prompt vectors are searched so that every image's fp32 gap |s1 - s0| is at least
10 x the largest change of that gap in transformers' own fp16 run (asserted here) and both labels occur.
LayerNorm gains / biases are randomised (an applied or missing norm shows) and the q projections are scaled by 4 (fresh-init attention
is near-uniform, where a wrong attention pattern hides in 16-bit noise).  Three files, each below the repository's 1 MiB limit.
Run on the CPU where transformers 5.x and Pillow are installed: python tests/golden/make_clip_vision_golden.py"""
import json
import os
import sys

import numpy as np
import torch
from PIL import Image
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests_support.clip_vision_oracle import SimClassifier, preprocess, rel_l2  # noqa: E402

CFG = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
           projection_dim=64, hidden_act="quick_gelu")
SRC = 80


def build(sd=None, dtype=torch.float32):
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(attention_dropout=0.0, **CFG))
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dtype).eval()


def randomise(sd, g):
    out = {}
    for k, v in sd.items():
        if "norm" in k:                                            # pre_layrnorm (sic), layer_norm1 / 2, post_layernorm
            v = (0.5 + torch.rand(v.shape, generator=g)) if k.endswith("weight") else 0.3 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            v = 0.1 * torch.randn(v.shape, generator=g)
        elif "class_embedding" in k or "position_embedding" in k:
            v = 0.5 * torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * (v.numel() // v.shape[0]) ** -0.5
        if ".q_proj." in k:
            v = v * 4
        out[k] = v
    return out


def make_images(g):
    yy, xx = torch.meshgrid(torch.arange(SRC, dtype=torch.float32), torch.arange(SRC, dtype=torch.float32), indexing="ij")
    imgs = [torch.randint(0, 256, (SRC, SRC, 3), generator=g).float(),                                    # noise: the resize's ringing clips
            torch.stack([xx * 3.1, yy * 3.1, (xx + yy) * 1.6], -1),                                       # smooth ramps
            torch.stack([127 + 127 * torch.sin(xx / 3.0), 127 + 127 * torch.cos(yy / 5.0), 255 - xx * 3], -1)]
    for cx, cy, r in ((20, 30, 12), (55, 50, 20), (40, 40, 33)):                                         # hard-edged discs on flat grounds
        disc = ((xx - cx) ** 2 + (yy - cy) ** 2 < r * r).float()
        col = torch.randint(0, 256, (2, 3), generator=g).float()
        imgs.append(disc[..., None] * col[0] + (1 - disc[..., None]) * col[1])
    return torch.stack(imgs).clamp(0, 255).to(torch.uint8)


g = torch.Generator().manual_seed(0)
torch.manual_seed(1)
sd = randomise(build().state_dict(), g)
images = make_images(g)
resized = np.stack([np.asarray(Image.fromarray(im).resize((CFG["image_size"],) * 2, Image.BICUBIC)) for im in images.numpy()])
pixel_values = preprocess(torch.from_numpy(resized))
main = {"images": images.numpy(), "resized": resized, "pixel_values": pixel_values.numpy(),
        "cfg_json": np.array(json.dumps(CFG, sort_keys=True))}       # a string array: the files load with allow_pickle=False
with torch.no_grad():
    o32 = build(sd)(pixel_values=pixel_values)
    ref = {"last_hidden_state": o32.last_hidden_state, "image_embeds": o32.image_embeds}
    o64 = build(sd, torch.float64)(pixel_values=pixel_values.double())
    print("fp32 vs fp64:", rel_l2(ref["last_hidden_state"], o64.last_hidden_state), rel_l2(ref["image_embeds"], o64.image_embeds))
    low = {}
    for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        o16 = build(sd, dt)(pixel_values=pixel_values.to(dt))
        low[tag] = o16.image_embeds
        for q, got in (("last_hidden_state", o16.last_hidden_state), ("image_embeds", o16.image_embeds)):
            main[f"err_{tag}_{q}"] = np.float64(rel_l2(got.float(), ref[q]))
            print(f"err_{tag}_{q} = {float(main[f'err_{tag}_{q}']):.3e}")
    # the two prompt vectors: the first seed whose gaps are all decided by a wide margin in fp16 and whose labels are mixed
    for seed in range(1, 10000):
        prompts = torch.randn(2, CFG["projection_dim"], generator=torch.Generator().manual_seed(seed))
        head = SimClassifier(prompts)
        s32, s16 = head(ref["image_embeds"]), head(low["f16"].float())
        gap32, gap16 = s32[:, 1] - s32[:, 0], s16[:, 1] - s16[:, 0]
        labels = s32.argmax(-1)
        if float(gap32.abs().min()) >= 10.0 * float((gap16 - gap32).abs().max()) and 2 <= int(labels.sum()) <= 4:
            break
    else:
        raise SystemExit("no prompt pair found")
    assert float(gap32.abs().min()) >= 10.0 * float((gap16 - gap32).abs().max())
    print("prompt seed", seed, "labels", labels.tolist(), "gaps", [round(v, 3) for v in gap32.tolist()], "largest fp16 change of a gap",
          float((gap16 - gap32).abs().max()))
main.update({k: v.numpy() for k, v in ref.items()})
main.update(prompts=prompts.numpy(), similarity=s32.numpy(), labels=labels.numpy())
halves, size = ({}, {}), 0
total = sum(v.numel() for v in sd.values())
for k, v in sd.items():
    halves[0 if size < total // 2 else 1][f"sd/{k}"] = v.numpy()
    size += v.numel()
for i, d in enumerate(halves):
    name = f"clip_vision_golden_sd_{i}.npz"
    np.savez_compressed(os.path.join(HERE, name), **d)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")
    assert os.path.getsize(os.path.join(HERE, name)) < (1 << 20), name
path = os.path.join(HERE, "clip_vision_golden.npz")
np.savez_compressed(path, **main)
print("wrote clip_vision_golden.npz", os.path.getsize(path), "bytes")
assert os.path.getsize(path) < (1 << 20)
