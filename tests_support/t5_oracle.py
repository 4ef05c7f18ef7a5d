"""A plain-torch restatement of transformers' T5EncoderModel (T5-v1.1: RMS layer norm, bidirectional self-attention with a
learned relative-position bias and no 1/sqrt(d) scale, gelu_new-gated feed-forward, no biases), used as the oracle at sizes
the golden fixture does not cover.  Runs in whatever dtype / device the state dict has.  The relative-position bias is kept
as the engine keeps it: one vector of 2n - 1 values per head (it is Toeplitz), expanded by indexing only inside this oracle."""
import json
import math
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
GOLDEN_PARTS = ("t5_golden.npz", "t5_golden_peaked.npz", "t5_golden_sd0.npz", "t5_golden_sd1.npz")   # each below the 1 MiB file limit


def load_golden() -> dict:
    out = {}
    for name in GOLDEN_PARTS:
        with np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    out["cfg"] = json.loads(str(out.pop("cfg_json")))
    return out


def golden_state_dict(g: dict, peaked: bool = False) -> dict:
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")}
    return peak(sd) if peaked else sd


def peak(sd: dict) -> dict:
    """The fixture's peaked arm: relative_attention_bias x 8 and every q projection x 4 (scores far from zero)."""
    out = {}
    for k, v in sd.items():
        if k.endswith("relative_attention_bias.weight"):
            v = v * 8
        elif k.endswith("SelfAttention.q.weight"):
            v = v * 4
        out[k] = v
    return out


def relative_position_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """T5Attention._relative_position_bucket, bidirectional (rel = key position - query position)."""
    num_buckets //= 2
    buckets = (rel > 0).to(torch.long) * num_buckets
    rel = torch.abs(rel)
    max_exact = num_buckets // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rel, large)


def bias_vector(table: torch.Tensor, n: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """[heads, 2n - 1]: entry d + n - 1 is the bias of key j = i + d seen from query i.  table = relative_attention_bias.weight."""
    rel = torch.arange(-(n - 1), n, device=table.device)
    return table[relative_position_bucket(rel, num_buckets, max_distance)].t().contiguous()


def expand_bias(vec: torch.Tensor, n: int) -> torch.Tensor:
    """[heads, 2n - 1] -> [heads, n, n] (oracle only: the engine never forms this)."""
    i = torch.arange(n, device=vec.device)
    return vec[:, (i[None, :] - i[:, None]) + n - 1]


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    var = x.float().pow(2).mean(-1, keepdim=True)
    return w * (x.float() * torch.rsqrt(var + eps)).to(w.dtype)


def gelu_new(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def biased_attention(q, k, v, bias_vec, key_mask=None, scale: float = 1.0):
    """q / k / v [B, H, n, d]; bias_vec [H, 2n - 1]; key_mask [B, n] (1 = attend).  softmax in f32."""
    n = q.shape[2]
    s = torch.matmul(q, k.transpose(-1, -2)).float() * scale + expand_bias(bias_vec.float(), n)[None]
    if key_mask is not None:
        s = s.masked_fill(key_mask[:, None, None, :] == 0, torch.finfo(torch.float32).min)
    return torch.matmul(torch.softmax(s, dim=-1).to(v.dtype), v)


def t5_encoder(sd: dict, input_ids: torch.Tensor, attention_mask=None, num_heads: int = 2, d_kv: int = 64, num_buckets: int = 32,
               max_distance: int = 128, eps: float = 1e-6) -> torch.Tensor:
    sd = {(k[len("encoder."):] if k.startswith("encoder.") else k): v for k, v in sd.items()}
    emb = sd["embed_tokens.weight"] if "embed_tokens.weight" in sd else sd["shared.weight"]
    x = emb[input_ids]
    b, n, _ = x.shape
    vec = bias_vector(sd["block.0.layer.0.SelfAttention.relative_attention_bias.weight"], n, num_buckets, max_distance)
    layer = 0
    while f"block.{layer}.layer.0.layer_norm.weight" in sd:
        p = f"block.{layer}.layer"
        h = rms_norm(x, sd[p + ".0.layer_norm.weight"], eps)
        q, k, v = (torch.nn.functional.linear(h, sd[p + f".0.SelfAttention.{t}.weight"]).view(b, n, num_heads, d_kv).transpose(1, 2)
                   for t in "qkv")
        a = biased_attention(q, k, v, vec, attention_mask).transpose(1, 2).reshape(b, n, num_heads * d_kv)
        x = x + torch.nn.functional.linear(a, sd[p + ".0.SelfAttention.o.weight"])
        h = rms_norm(x, sd[p + ".1.layer_norm.weight"], eps)
        g = gelu_new(torch.nn.functional.linear(h, sd[p + ".1.DenseReluDense.wi_0.weight"]))
        h = g * torch.nn.functional.linear(h, sd[p + ".1.DenseReluDense.wi_1.weight"])
        x = x + torch.nn.functional.linear(h, sd[p + ".1.DenseReluDense.wo.weight"])
        layer += 1
    return rms_norm(x, sd["final_layer_norm.weight"], eps)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


class FakeT5Tokenizer:
    """A stand-in for transformers' T5 tokenizer (no sentencepiece vocabulary is available): whitespace words -> deterministic
    ids, ONE end token (id 1) and no start token, padding with id 0, the call options the SD-v3 front end uses."""

    def __init__(self, vocab_size=32128, model_max_length=512):
        self.vocab_size, self.model_max_length = vocab_size, model_max_length
        self.eos_token_id, self.pad_token_id = 1, 0

    def _ids(self, text):
        import zlib
        return [2 + zlib.crc32(w.encode()) % (self.vocab_size - 2) for w in text.lower().replace(",", " , ").split()]

    def __call__(self, texts, padding="max_length", max_length=None, truncation=False, add_special_tokens=True, return_tensors="pt"):
        from types import SimpleNamespace
        texts = [texts] if isinstance(texts, str) else list(texts)
        rows = [self._ids(t) + [self.eos_token_id] for t in texts]
        cap = max_length or self.model_max_length
        if truncation:
            rows = [r if len(r) <= cap else r[:cap - 1] + [self.eos_token_id] for r in rows]
        n = cap if padding == "max_length" else max(len(r) for r in rows)
        ids = torch.full((len(rows), n), self.pad_token_id, dtype=torch.int64)
        mask = torch.zeros((len(rows), n), dtype=torch.int64)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r[:n])
            mask[i, :min(len(r), n)] = 1
        return SimpleNamespace(input_ids=ids, attention_mask=mask)
