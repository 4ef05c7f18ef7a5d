#!/usr/bin/env python3
"""Throughput of the two image-metric scorers (safe_denoiser_amd/metrics.py) at batch 64: uint8 images [B, 512, 512, 3] on the GPU
-> AestheticScore on the CLIP ViT-L/14 tower, and -> CLIPScore on the ViT-B/32 geometry (vision hidden 768 / 12 heads / patch 32 /
projection 512, text hidden 512 / 8 heads) against 77-token id rows.  SYNTHETIC weights throughout: the figures are times, the
scores mean nothing.  Recorded, not gated: writes profiles/metrics_bench.json -- images per second of each chain, and the share of
the chain's time spent in sdn_embed_row_scores (the scoring head timed alone on the chain's own embeddings, launched back to back:
at 64 rows it is one 16-block launch, so its figure is the launch rate, an upper bound of the kernel's own time)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_denoiser_amd import metrics as M  # noqa: E402
from safe_denoiser_amd.clip import CLIPTextModelWithProjection  # noqa: E402
from safe_denoiser_amd.clip_vision import CLIPVisionModelWithProjection, clip_preprocess  # noqa: E402

VIT_B32_VISION = dict(image_size=224, patch_size=32, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                      projection_dim=512, hidden_act="quick_gelu")
VIT_B32_TEXT = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                    max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=512, eos_token_id=2)
AE_WIDTHS = (768, 1024, 128, 64, 16, 1)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def synthetic_head(seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, fan_in, fan_out in zip(M.AE_LINEARS, AE_WIDTHS[:-1], AE_WIDTHS[1:]):
        sd[f"layers.{i}.weight"] = torch.randn(fan_out, fan_in, generator=g) / fan_in ** 0.5
        sd[f"layers.{i}.bias"] = 0.1 * torch.randn(fan_out, generator=g)
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    args = ap.parse_args()
    b = args.batch
    u8 = torch.randint(0, 256, (b, args.side, args.side, 3), generator=torch.Generator(device="cuda").manual_seed(0), device="cuda",
                       dtype=torch.uint8)
    ids = torch.randint(1, 49406, (b, 77), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, 20], ids[:, 21:] = 49406, 49407, 49407
    result = {"batch": b, "side": args.side, "iters": args.iters, "device": torch.cuda.get_device_name(0), "weights": "synthetic",
              "storage": "fp16 (both towers; torchmetrics runs the CLIP model in fp32)"}

    vision = CLIPVisionModelWithProjection(dtype=torch.float16)                    # ViT-L/14
    vision.load_synthetic_on_device(7)
    aes = M.AestheticScore(vision, synthetic_head(3))
    emb = vision(clip_preprocess(u8), output_hidden_state=False).image_embeds
    w = aes.w_eff.cuda()
    ms_chain = timed(lambda: aes.update(u8), args.warmup, args.iters)
    ms_head = timed(lambda: M.embed_row_scores(emb, w, False, 1.0, aes.b_eff), args.warmup, 100 * args.iters)
    result["aesthetic_vit_l14"] = {"chain_ms": ms_chain, "images_per_s": 1e3 * b / ms_chain, "embed_row_scores_ms": ms_head,
                                   "embed_row_scores_share": ms_head / ms_chain}
    print("aesthetic_vit_l14", result["aesthetic_vit_l14"])
    del aes, vision

    vision = CLIPVisionModelWithProjection(dtype=torch.float16, **VIT_B32_VISION)
    vision.load_synthetic_on_device(8)
    text = CLIPTextModelWithProjection(dtype=torch.float16, **VIT_B32_TEXT)
    text.load_synthetic_on_device(9)
    cs = M.CLIPScore(vision, text)
    img = vision(clip_preprocess(u8), output_hidden_state=False).image_embeds
    txt = text(ids, output_hidden_states=True).text_embeds
    ms_chain = timed(lambda: cs.update(u8, ids), args.warmup, args.iters)
    ms_head = timed(lambda: M.embed_row_scores(img, txt, True, 100.0), args.warmup, 100 * args.iters)
    result["clip_score_vit_b32"] = {"chain_ms": ms_chain, "images_per_s": 1e3 * b / ms_chain, "embed_row_scores_ms": ms_head,
                                    "embed_row_scores_share": ms_head / ms_chain}
    print("clip_score_vit_b32", result["clip_score_vit_b32"])
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
