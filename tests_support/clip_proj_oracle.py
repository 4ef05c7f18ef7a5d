"""A plain-torch restatement of transformers' CLIPTextModelWithProjection (token + position embeddings, pre-LN layers with causal
self-attention, a quick-GELU or exact-erf GELU MLP, final LayerNorm on the pooled row, bias-free text_projection), used as the
oracle at sizes the golden fixture does not cover.  Runs in whatever dtype / device the state dict has.  Returns every hidden
state (index 0 = the embeddings, index l = the output of layer l - 1, none of them final-normed), the pooling positions and the
projected pooled vector, as SD-v3 reads them (models/sdv3/safe_denoiser_pipeline.py:382-386)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
# each below the 1 MiB file limit: outputs + errors of both arms, then each arm's state dict in two halves
GOLDEN_PARTS = ("clip_proj_golden.npz", "clip_proj_golden_sd_a0.npz", "clip_proj_golden_sd_a1.npz", "clip_proj_golden_sd_b0.npz",
                "clip_proj_golden_sd_b1.npz")
ARMS = ("a", "b")

# text_encoder/config.json and text_encoder_2/config.json of SD-v3 (CLIP-L and OpenCLIP bigG), the fields the engine reads
CLIP_L_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                     max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768, eos_token_id=2)
CLIP_G_CONFIG = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                     max_position_embeddings=77, hidden_act="gelu", projection_dim=1280, eos_token_id=2)


def load_golden() -> dict:
    out = {}
    for name in GOLDEN_PARTS:
        with np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    for arm in ARMS:
        out[f"{arm}/cfg"] = json.loads(str(out.pop(f"{arm}/cfg_json")))
    return out


def golden_state_dict(g: dict, arm: str) -> dict:
    pre = f"{arm}/sd/"
    return {k[len(pre):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre)}


def canonical(sd: dict) -> dict:
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}


def expected_state_dict_shapes(cfg: dict) -> dict:
    """CLIPTextModelWithProjection.state_dict()'s keys (without `text_model.`) -> shapes, from the config alone."""
    c, i, v = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    n, p = cfg["max_position_embeddings"], cfg["projection_dim"]
    out = {"embeddings.token_embedding.weight": (v, c), "embeddings.position_embedding.weight": (n, c),
           "final_layer_norm.weight": (c,), "final_layer_norm.bias": (c,), "text_projection.weight": (p, c)}
    for l in range(cfg["num_hidden_layers"]):
        q = f"encoder.layers.{l}."
        for t in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[q + f"self_attn.{t}.weight"] = (c, c)
            out[q + f"self_attn.{t}.bias"] = (c,)
        for t in ("layer_norm1", "layer_norm2"):
            out[q + t + ".weight"] = (c,)
            out[q + t + ".bias"] = (c,)
        out[q + "mlp.fc1.weight"], out[q + "mlp.fc1.bias"] = (i, c), (i,)
        out[q + "mlp.fc2.weight"], out[q + "mlp.fc2.bias"] = (c, i), (c,)
    return out


def pool_positions(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """transformers' two rules: the highest id (legacy configs, eos_token_id == 2), else the first eos_token_id (0 when absent)."""
    if eos_token_id == 2:
        return input_ids.to(torch.int).argmax(dim=-1)
    return (input_ids == eos_token_id).to(torch.int).argmax(dim=-1)


def activation(x: torch.Tensor, hidden_act: str) -> torch.Tensor:
    if hidden_act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if hidden_act == "gelu":
        return F.gelu(x)
    raise ValueError(hidden_act)


def clip_text_with_projection(sd: dict, input_ids: torch.Tensor, *, num_heads: int, hidden_act: str, eos_token_id: int,
                              eps: float = 1e-5):
    sd = canonical(sd)
    b, n = input_ids.shape
    x = sd["embeddings.token_embedding.weight"][input_ids] + sd["embeddings.position_embedding.weight"][:n][None]
    c = x.shape[-1]
    d = c // num_heads
    causal = torch.full((n, n), float("-inf"), device=x.device).triu_(1)
    hidden = [x]
    layer = 0
    while f"encoder.layers.{layer}.layer_norm1.weight" in sd:
        p = f"encoder.layers.{layer}."
        h = F.layer_norm(x, (c,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps)
        q, k, v = (F.linear(h, sd[p + f"self_attn.{t}_proj.weight"], sd[p + f"self_attn.{t}_proj.bias"]).view(b, n, num_heads, d)
                   .transpose(1, 2) for t in "qkv")
        s = torch.matmul(q, k.transpose(-1, -2)).float() * d ** -0.5 + causal
        a = torch.matmul(torch.softmax(s, dim=-1).to(v.dtype), v).transpose(1, 2).reshape(b, n, c)
        x = x + F.linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (c,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps)
        h = activation(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]), hidden_act)
        x = x + F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        hidden.append(x)
        layer += 1
    pos = pool_positions(input_ids, eos_token_id).long()
    rows = x[torch.arange(b, device=x.device), pos]
    pooled = F.layer_norm(rows, (c,), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], eps)
    text_embeds = F.linear(pooled, sd["text_projection.weight"])
    return SimpleNamespace(text_embeds=text_embeds, hidden_states=tuple(hidden), positions=pos, pooled=pooled)


def final_norm(sd: dict, x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    sd = canonical(sd)
    return F.layer_norm(x, (x.shape[-1],), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], eps)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


class FakeCLIPTokenizer:
    """A stand-in for transformers' CLIPTokenizer (no vocabulary files are available): characters -> deterministic ids, a start
    token, ONE end token, padding with `pad_token_id`, the call options the SD-v3 front end uses."""

    def __init__(self, vocab_size=512, bos_token_id=None, eos_token_id=None, pad_token_id=None, model_max_length=77):
        self.vocab_size, self.model_max_length = vocab_size, model_max_length
        self.bos_token_id = vocab_size - 2 if bos_token_id is None else bos_token_id
        self.eos_token_id = vocab_size - 1 if eos_token_id is None else eos_token_id
        self.pad_token_id = self.eos_token_id if pad_token_id is None else pad_token_id
        self.calls = []

    def __call__(self, texts, padding=None, max_length=None, truncation=None, return_tensors=None):
        texts = [texts] if isinstance(texts, str) else list(texts)
        self.calls.append(dict(texts=texts, padding=padding, max_length=max_length, truncation=truncation))
        n = max_length or self.model_max_length
        low = min(self.bos_token_id, self.eos_token_id, self.pad_token_id)
        ids = torch.full((len(texts), n), self.pad_token_id, dtype=torch.int64)
        for i, t in enumerate(texts):
            body = [1 + (ord(ch) * 7 + j) % (low - 1) for j, ch in enumerate(t)][:n - 2]
            row = [self.bos_token_id] + body + [self.eos_token_id]
            ids[i, :len(row)] = torch.tensor(row)
        return SimpleNamespace(input_ids=ids)
