#!/usr/bin/env python3
"""Generates the projected-CLIP fixture: two small randomly initialised transformers.CLIPTextModelWithProjection models (the
third-party class the SD-v3 reference pipeline calls as text_encoder and text_encoder_2), their state dicts, ids, the fp32
hidden_states[-2], hidden_states[-3] and text_embeds, the pooling positions, and the distance of transformers' OWN bf16 / fp16
runs of the same model from those outputs (the error a 16-bit implementation is allowed).
  arm a: quick_gelu, eos_token_id = 2 (the legacy rule: pool at the highest id), projection_dim != hidden_size;
  arm b: gelu (exact erf), eos_token_id = 100 with pad id 120 and start id 126 above it, so the first-match rule and the
         highest-id rule give different positions; one sequence holds two end tokens.
Norm gains / biases are randomised (an applied or missing final_layer_norm shows) and the q projections are scaled by 4 (fresh-init
attention is near-uniform, where a wrong mask hides in 16-bit noise).  Written as five files, each below the repository's 1 MiB
limit: clip_proj_golden.npz (ids, outputs, positions, every err_*), clip_proj_golden_sd_{a,b}{0,1}.npz (the state dicts).
Run on the CPU where transformers 5.x is installed: python tests/golden/make_clip_proj_golden.py"""
import json
import os
import sys

import numpy as np
import torch
from transformers import CLIPTextConfig, CLIPTextModelWithProjection

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests_support.clip_proj_oracle import rel_l2  # noqa: E402

BASE = dict(vocab_size=128, hidden_size=128, intermediate_size=128, num_hidden_layers=3, num_attention_heads=2,
            max_position_embeddings=77)
ARMS = {"a": dict(BASE, hidden_act="quick_gelu", projection_dim=64, eos_token_id=2, pad_token_id=127, bos_token_id=126),
        "b": dict(BASE, hidden_act="gelu", projection_dim=128, eos_token_id=100, pad_token_id=120, bos_token_id=126)}
REAL = (9, 30, 75, 3)                                     # body tokens per sequence


def build(cfg, sd=None, dtype=torch.float32):
    m = CLIPTextModelWithProjection(CLIPTextConfig(attention_dropout=0.0, **cfg))
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dtype).eval()


def randomise(sd, g):
    out = {}
    for k, v in sd.items():
        if "layer_norm" in k:
            v = (0.5 + torch.rand(v.shape, generator=g)) if k.endswith("weight") else 0.3 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            v = 0.1 * torch.randn(v.shape, generator=g)
        elif "embedding" in k:
            v = 0.5 * torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * v.shape[1] ** -0.5
        if ".q_proj." in k:
            v = v * 4
        out[k] = v
    return out


def make_ids(cfg, g):
    end = cfg["eos_token_id"] if cfg["eos_token_id"] != 2 else 127          # arm a: the end token is the highest id, as in CLIP's vocabulary
    ids = torch.full((len(REAL), 77), cfg["pad_token_id"], dtype=torch.int64)
    for i, r in enumerate(REAL):
        ids[i, 0] = cfg["bos_token_id"]
        ids[i, 1:1 + r] = torch.randint(3, 100, (r,), generator=g)
        ids[i, 1 + r] = end
    if cfg["eos_token_id"] != 2:
        ids[1, 50] = end                                                      # a second end token further on: the FIRST one pools
    return ids


g = torch.Generator().manual_seed(0)
main = {}
for arm, cfg in ARMS.items():
    torch.manual_seed(1)
    sd = randomise(build(cfg).state_dict(), g)
    ids = make_ids(cfg, g)
    with torch.no_grad():
        o32 = build(cfg, sd)(ids, output_hidden_states=True)
        ref = {"h2": o32.hidden_states[-2], "h3": o32.hidden_states[-3], "text_embeds": o32.text_embeds}
        o64 = build(cfg, sd, torch.float64)(ids, output_hidden_states=True)
        print(arm, "fp32 vs fp64:", rel_l2(ref["h2"], o64.hidden_states[-2]), rel_l2(ref["text_embeds"], o64.text_embeds))
        for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            o16 = build(cfg, sd, dt)(ids, output_hidden_states=True)
            got = {"h2": o16.hidden_states[-2], "h3": o16.hidden_states[-3], "text_embeds": o16.text_embeds}
            for q in ref:
                main[f"{arm}/err_{tag}_{q}"] = np.float64(rel_l2(got[q].float(), ref[q]))
                print(f"{arm}/err_{tag}_{q} = {float(main[f'{arm}/err_{tag}_{q}']):.3e}")
    if cfg["eos_token_id"] == 2:
        pos = ids.argmax(-1)
    else:
        pos = (ids == cfg["eos_token_id"]).int().argmax(-1)
    print(arm, "pooling positions", pos.tolist(), "highest-id positions", ids.argmax(-1).tolist())
    main.update({f"{arm}/{q}": v.numpy() for q, v in ref.items()})
    main[f"{arm}/ids"], main[f"{arm}/positions"] = ids.numpy(), pos.numpy()
    main[f"{arm}/cfg_json"] = np.array(json.dumps(cfg, sort_keys=True))      # a string array: the files load with allow_pickle=False
    halves, size = ({}, {}), 0
    total = sum(v.numel() for v in sd.values())
    for k, v in sd.items():
        halves[0 if size < total // 2 else 1][f"{arm}/sd/{k}"] = v.numpy()
        size += v.numel()
    for i, d in enumerate(halves):
        main_name = f"clip_proj_golden_sd_{arm}{i}.npz"
        np.savez_compressed(os.path.join(HERE, main_name), **d)
        print("wrote", main_name, os.path.getsize(os.path.join(HERE, main_name)), "bytes")
        assert os.path.getsize(os.path.join(HERE, main_name)) < (1 << 20), main_name
path = os.path.join(HERE, "clip_proj_golden.npz")
np.savez_compressed(path, **main)
print("wrote clip_proj_golden.npz", os.path.getsize(path), "bytes")
assert os.path.getsize(path) < (1 << 20)
