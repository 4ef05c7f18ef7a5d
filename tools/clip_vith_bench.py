#!/usr/bin/env python3
"""CLIP ViT-H/14 (the COCO driver's CLIP-score evaluator) at full size on one GPU, synthetic weights, one process:

  parity     32-layer vision tower and 24-layer text tower at B = 2 against the fp32 torch oracle on the same 16-bit weights:
             rel L2 of image_embeds / text_embeds and the largest |cosine - oracle cosine| over the image-prompt pairs;
  towers     milliseconds per forward at B = 64 of the ViT-H/14 vision and text towers, next to ViT-L/14's vision tower and the
             CLIP-L projected text tower in the same run (median, min and max of `--repeats` windows of `--iters` forwards each);
  fc1        the share of the erf-GELU fc1 launches (N = 5120, K = 1280) in one profiled ViT-H forward -- the engine's own per-launch
             profile (sdn_unet_profile_next) -- next to fc2 (the same FLOPs, no activation) and to the same tower built with quick-GELU;
  evaluator  images per second of CocoClipEval.pair_scores on a decoded uint8 batch against clip_score called per image.

Recorded, not gated: writes profiles/clip_vith.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import safe_denoiser_amd as sda  # noqa: E402
from safe_denoiser_amd import clip_vision as V, coco_eval as E  # noqa: E402
from safe_denoiser_amd.clip import SD3_CLIP_L_CONFIG, CLIPTextModelWithProjection  # noqa: E402
from tests_support import clip_proj_oracle as OP  # noqa: E402
from tests_support import clip_vision_oracle as OV  # noqa: E402
from tests_support.coco_support import device_state_dict  # noqa: E402

VITH_TEXT = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                 max_position_embeddings=77, hidden_act="gelu", projection_dim=1024, eos_token_id=2)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [window(fn, iters) for _ in range(repeats)]
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def prompt_ids(b, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 2, (b, 77), generator=g)
    for i in range(b):
        n = 5 + (7 * i) % 70
        ids[i, 0], ids[i, n - 1], ids[i, n:] = vocab - 2, vocab - 1, vocab - 1
    return ids


def per_op(m, run):
    """[(label, M, N, K, ms)] of one profiled forward, in plan order."""
    lib = sda.lib()
    lib.sdn_debug_profile_ops.restype = C.c_int
    lib.sdn_debug_profile_ops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    m.profile_next()
    run()
    torch.cuda.synchronize()
    out = (C.c_double * (6 * 4096))()
    lab = C.create_string_buffer(24 * 4096)
    n = lib.sdn_debug_profile_ops(m._h, out, lab, 4096)
    if n < 0:
        raise RuntimeError(f"sdn_debug_profile_ops returned {n}")
    return [(lab.raw[i * 24:(i + 1) * 24].split(b"\0")[0].decode(), int(out[i * 6 + 3]), int(out[i * 6 + 4]), int(out[i * 6 + 5]), out[i * 6])
            for i in range(n)]


def fc_split(m, pv, reps=3):
    c, i = m.config.hidden_size, m.config.intermediate_size
    acc = {"total_ms": [], "fc1_ms": [], "fc2_ms": [], "fc1_launches": 0}
    for _ in range(reps):
        rows = per_op(m, lambda: m(pv))                            # with last_hidden_state: every op of the plan runs and is timed
        fc1 = [r for r in rows if r[0].startswith("k_gemm") and r[2] == i and r[3] == c]
        fc2 = [r for r in rows if r[0].startswith("k_gemm") and r[2] == c and r[3] == i]
        acc["total_ms"].append(sum(r[4] for r in rows))
        acc["fc1_ms"].append(sum(r[4] for r in fc1))
        acc["fc2_ms"].append(sum(r[4] for r in fc2))
        acc["fc1_launches"], acc["fc1_label"], acc["fc2_label"] = len(fc1), fc1[0][0], fc2[0][0]
    out = {k: (statistics.median(v) if isinstance(v, list) else v) for k, v in acc.items()}
    out["fc1_share"] = out["fc1_ms"] / out["total_ms"]
    out["fc1_over_fc2"] = out["fc1_ms"] / out["fc2_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--per-image", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vith.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_vith_bench needs an MI355X: nothing is measured without one")
    t = (args.warmup, args.iters, args.repeats)
    B = args.batch
    result = {"batch": B, "side": args.side, "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
              "weights": "synthetic (seeded)"}
    g = torch.Generator(device="cuda").manual_seed(0)
    u8 = torch.randint(0, 256, (B, args.side, args.side, 3), generator=g, device="cuda", dtype=torch.uint8)
    ids = prompt_ids(B, 49408, 1)
    for tag, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        r = {}
        vision = V.CLIPVisionModelWithProjection(dtype=dt, **V.VIT_H14_CONFIG)
        text = CLIPTextModelWithProjection(dtype=dt, **VITH_TEXT)
        vsd, tsd = device_state_dict(vision, 11), device_state_dict(text, 12)
        vision.load_state_dict(vsd)
        text.load_state_dict(tsd)
        ev = E.CocoClipEval(vision, text)
        # ---- parity at B = 2
        pv2 = V.clip_preprocess_any(u8[:2], 224)
        with torch.no_grad():
            ri = OV.clip_vision_with_projection({k: v.float() for k, v in vsd.items()}, pv2, num_heads=16, hidden_act="gelu").image_embeds
            li = OV.clip_vision_with_projection({k: v.to(dt) for k, v in vsd.items()}, pv2, num_heads=16, hidden_act="gelu").image_embeds
            rt = OP.clip_text_with_projection({k: v.float() for k, v in tsd.items()}, ids[:2].cuda(), num_heads=16, hidden_act="gelu",
                                              eos_token_id=2).text_embeds
            lt = OP.clip_text_with_projection({k: v.to(dt) for k, v in tsd.items()}, ids[:2].cuda(), num_heads=16, hidden_act="gelu",
                                              eos_token_id=2).text_embeds
        gi, gt = vision(pv2, output_hidden_state=False).image_embeds, text(ids[:2]).text_embeds
        cos = lambda a, b: torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)
        r["parity"] = {"image_embeds_rel_l2": OV.rel_l2(gi.float(), ri), "image_embeds_rel_l2_torch_at_this_width": OV.rel_l2(li.float(), ri),
                       "text_embeds_rel_l2": OV.rel_l2(gt.float(), rt), "text_embeds_rel_l2_torch_at_this_width": OV.rel_l2(lt.float(), rt),
                       "cosine_oracle_fp32": cos(ri, rt).tolist(), "cosine_engine": ev.pair_scores(u8[:2], ids[:2]).tolist(),
                       "cosine_max_abs_diff": float((ev.pair_scores(u8[:2], ids[:2]).double() - cos(ri, rt)).abs().max()),
                       "cosine_max_abs_diff_torch_at_this_width": float((cos(li, lt) - cos(ri, rt)).abs().max())}
        del vsd, tsd, ri, li, rt, lt
        # ---- tower times at B
        pv = V.clip_preprocess_any(u8, 224)
        r["vit_h14_vision"] = dict(timed(lambda: vision(pv, output_hidden_state=False), *t), tflop_per_forward=vision.flops(B)[0] / 1e12)
        r["vit_h14_text"] = dict(timed(lambda: text(ids), *t), tflop_per_forward=text.flops(B)[0] / 1e12)
        r["preprocess_any_512_to_224"] = timed(lambda: V.clip_preprocess_any(u8, 224), *t)
        # ---- fc1 share
        r["vit_h14_fc"] = fc_split(vision, pv)
        # ---- evaluator: batched against per image
        k = min(args.per_image, B)
        r["evaluator_batched"] = timed(lambda: ev.pair_scores(u8, ids), *t)
        r["evaluator_batched"]["images_per_s"] = 1e3 * B / r["evaluator_batched"]["ms_median"]

        def one_by_one():
            for i in range(k):
                ev.clip_score(u8[i:i + 1], ids[i:i + 1])           # reads the score back, as the per-image driver path does
        r["evaluator_per_image"] = timed(one_by_one, 1, 1, args.repeats)
        r["evaluator_per_image"]["images"] = k
        r["evaluator_per_image"]["images_per_s"] = 1e3 * k / r["evaluator_per_image"]["ms_median"]
        del ev, vision, text
        torch.cuda.empty_cache()
        # ---- the same tower with quick-GELU: what the erf epilogue costs over the sigmoid one
        quick = V.CLIPVisionModelWithProjection(dtype=dt, **dict(V.VIT_H14_CONFIG, hidden_act="quick_gelu"))
        quick.load_synthetic_on_device(7)
        r["vit_h14_vision_quick_gelu"] = timed(lambda: quick(pv, output_hidden_state=False), *t)
        r["vit_h14_fc_quick_gelu"] = fc_split(quick, pv)
        del quick
        # ---- ViT-L/14 and the CLIP-L projected text tower, same run
        vl = V.CLIPVisionModelWithProjection(dtype=dt)
        vl.load_synthetic_on_device(7)
        r["vit_l14_vision"] = dict(timed(lambda: vl(pv, output_hidden_state=False), *t), tflop_per_forward=vl.flops(B)[0] / 1e12)
        tl = CLIPTextModelWithProjection(dtype=dt, hidden_act="quick_gelu", projection_dim=768, **SD3_CLIP_L_CONFIG)
        tl.load_synthetic_on_device(8)
        r["clip_l_text"] = dict(timed(lambda: tl(ids), *t), tflop_per_forward=tl.flops(B)[0] / 1e12)
        del vl, tl
        torch.cuda.empty_cache()
        result[tag] = r
        print(tag, json.dumps(r))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
