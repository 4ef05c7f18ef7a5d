#!/usr/bin/env python3
"""Generates the T5 fixture: one small randomly initialised transformers.T5EncoderModel (the third-party module the SD-v3
reference pipeline calls as text_encoder_3), its state_dict, inputs, fp32 outputs, and the distance of transformers' OWN bf16 /
fp16 runs of the same model from those outputs (the error a 16-bit implementation is allowed).  A second, PEAKED arm scales
relative_attention_bias by 8 and every q projection by 4: fresh-init scores are near zero, where a wrong bias or softmax base
hides inside 16-bit noise.  Written as four files, each below the repository's 1 MiB limit per file:
  t5_golden.npz (ids, masks, plain-arm outputs, every err_*), t5_golden_peaked.npz (peaked-arm outputs),
  t5_golden_sd0.npz / t5_golden_sd1.npz (the state dict).
Run on the CPU where transformers 5.x is installed: python tests/golden/make_t5_golden.py"""
import json
import os
import sys

import numpy as np
import torch
from transformers import T5Config, T5EncoderModel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests_support.t5_oracle import peak, rel_l2  # noqa: E402

CFG = dict(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=2, relative_attention_num_buckets=32,
           relative_attention_max_distance=128, layer_norm_epsilon=1e-6)


def build(sd=None, dtype=torch.float32):
    m = T5EncoderModel(T5Config(feed_forward_proj="gated-gelu", is_encoder_decoder=False, use_cache=False, dropout_rate=0.0,
                                pad_token_id=0, eos_token_id=1, **CFG))
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dtype).eval()


torch.manual_seed(0)
base = build()
sd = {k: v.clone() for k, v in base.state_dict().items()}
real = [20, 200, 256]
ids = torch.randint(2, 512, (3, 256))
for i, r in enumerate(real):
    ids[i, r - 1] = 1
    ids[i, r:] = 0
mask = (torch.arange(256)[None] < torch.tensor(real)[:, None]).long()
ids13 = torch.randint(2, 512, (1, 13))
ids13[0, 12] = 1

main, peaked = {}, {}
for arm, store, weights in (("", main, sd), ("peaked_", peaked, peak(sd))):
    m32 = build(weights)
    cases = {"plain": (ids, None), "masked": (ids, mask), "n13": (ids13, None)}
    with torch.no_grad():
        ref = {c: m32(i, attention_mask=a)[0] for c, (i, a) in cases.items()}
        m64 = build(weights, torch.float64)
        print(arm or "plain_", "fp32 vs fp64:", {c: rel_l2(ref[c], m64(i, attention_mask=a)[0]) for c, (i, a) in cases.items()})
        for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            m16 = build(weights, dt)
            for c, (i, a) in cases.items():
                main[f"err_{tag}_{arm}{c}"] = np.float64(rel_l2(m16(i, attention_mask=a)[0].float(), ref[c]))
                print(f"err_{tag}_{arm}{c} = {float(main[f'err_{tag}_{arm}{c}']):.3e}")
    store.update({f"{arm}{c}": v.numpy() for c, v in ref.items()})
main.update(ids=ids.numpy(), mask=mask.numpy(), ids13=ids13.numpy(), cfg_json=np.array(json.dumps(CFG, sort_keys=True)))   # a string array: the files load with allow_pickle=False
stored = {k: v for k, v in sd.items() if k != "shared.weight"}       # (tied to encoder.embed_tokens.weight: stored once)
assert torch.equal(sd["shared.weight"], sd["encoder.embed_tokens.weight"])
first = {"sd/" + k: v.numpy() for k, v in stored.items() if ".block.1." not in k and "final_layer_norm" not in k}
second = {"sd/" + k: v.numpy() for k, v in stored.items() if "sd/" + k not in first}
for name, d in (("t5_golden.npz", main), ("t5_golden_peaked.npz", peaked), ("t5_golden_sd0.npz", first), ("t5_golden_sd1.npz", second)):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **d)
    print("wrote", name, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20), name
