"""Oracles of the CLIP vision tower and the Q16 classifier: a plain-torch restatement of transformers' CLIPVisionModelWithProjection
(bias-free patch convolution, class token + position embedding, pre_layrnorm, pre-LN layers with bidirectional attention and a
quick-GELU or erf-GELU MLP, post_layernorm on the class row, bias-free visual_projection) that runs in whatever dtype / device the
state dict has; an integer restatement of Pillow's 8-bit bicubic resize; and the reference's SimClassifier
(run_nudity_sdv3.py:105-118)."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
GOLDEN_PARTS = ("clip_vision_golden.npz", "clip_vision_golden_sd_0.npz", "clip_vision_golden_sd_1.npz")   # each below 1 MiB

# the vision_config of openai/clip-vit-large-patch14 (the ViT-L/14 the reference loads), the fields the engine reads
VIT_L14_CONFIG = dict(image_size=224, patch_size=14, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24,
                      num_attention_heads=16, projection_dim=768, hidden_act="quick_gelu")
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def load_golden() -> dict:
    out = {}
    for name in GOLDEN_PARTS:
        with np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    out["cfg"] = json.loads(str(out.pop("cfg_json")))
    return out


def golden_state_dict(g: dict) -> dict:
    return {k[len("sd/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")}


def canonical(sd: dict) -> dict:
    return {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}


def expected_state_dict_shapes(cfg: dict) -> dict:
    """CLIPVisionModelWithProjection.state_dict()'s keys (without `vision_model.`) -> shapes, from the config alone."""
    c, i, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    n = 1 + (cfg["image_size"] // p) ** 2
    out = {"embeddings.class_embedding": (c,), "embeddings.patch_embedding.weight": (c, 3, p, p),
           "embeddings.position_embedding.weight": (n, c), "pre_layrnorm.weight": (c,), "pre_layrnorm.bias": (c,),
           "post_layernorm.weight": (c,), "post_layernorm.bias": (c,), "visual_projection.weight": (cfg["projection_dim"], c)}
    for l in range(cfg["num_hidden_layers"]):
        q = f"encoder.layers.{l}."
        for t in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[q + f"self_attn.{t}.weight"], out[q + f"self_attn.{t}.bias"] = (c, c), (c,)
        for t in ("layer_norm1", "layer_norm2"):
            out[q + t + ".weight"], out[q + t + ".bias"] = (c,), (c,)
        out[q + "mlp.fc1.weight"], out[q + "mlp.fc1.bias"] = (i, c), (i,)
        out[q + "mlp.fc2.weight"], out[q + "mlp.fc2.bias"] = (c, i), (c,)
    return out


def activation(x: torch.Tensor, hidden_act: str) -> torch.Tensor:
    if hidden_act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if hidden_act == "gelu":
        return F.gelu(x)
    raise ValueError(hidden_act)


def clip_vision_with_projection(sd: dict, pixel_values: torch.Tensor, *, num_heads: int, hidden_act: str, eps: float = 1e-5):
    sd = canonical(sd)
    w = sd["embeddings.patch_embedding.weight"]
    c, patch = w.shape[0], w.shape[-1]
    b = pixel_values.shape[0]
    x = F.conv2d(pixel_values.to(w.dtype), w, stride=patch).flatten(2).transpose(1, 2)
    x = torch.cat([sd["embeddings.class_embedding"].to(w.dtype).expand(b, 1, c), x], dim=1) + sd["embeddings.position_embedding.weight"][None]
    x = F.layer_norm(x, (c,), sd["pre_layrnorm.weight"], sd["pre_layrnorm.bias"], eps)
    n, d = x.shape[1], c // num_heads
    layer = 0
    while f"encoder.layers.{layer}.layer_norm1.weight" in sd:
        p = f"encoder.layers.{layer}."
        h = F.layer_norm(x, (c,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps)
        q, k, v = (F.linear(h, sd[p + f"self_attn.{t}_proj.weight"], sd[p + f"self_attn.{t}_proj.bias"]).view(b, n, num_heads, d)
                   .transpose(1, 2) for t in "qkv")
        s = torch.matmul(q, k.transpose(-1, -2)).float() * d ** -0.5
        a = torch.matmul(torch.softmax(s, dim=-1).to(v.dtype), v).transpose(1, 2).reshape(b, n, c)
        x = x + F.linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (c,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps)
        h = activation(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]), hidden_act)
        x = x + F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        layer += 1
    pooled = F.layer_norm(x[:, 0], (c,), sd["post_layernorm.weight"], sd["post_layernorm.bias"], eps)
    return SimpleNamespace(image_embeds=F.linear(pooled, sd["visual_projection.weight"]), last_hidden_state=x, pooled=pooled)


def to_openai_state_dict(sd: dict) -> dict:
    """The same tensors under the OpenAI CLIP checkpoint's `visual.*` names (fused in_proj, transposed proj)."""
    sd = canonical(sd)
    v = "visual."
    out = {v + "class_embedding": sd["embeddings.class_embedding"], v + "conv1.weight": sd["embeddings.patch_embedding.weight"],
           v + "positional_embedding": sd["embeddings.position_embedding.weight"], v + "ln_pre.weight": sd["pre_layrnorm.weight"],
           v + "ln_pre.bias": sd["pre_layrnorm.bias"], v + "ln_post.weight": sd["post_layernorm.weight"],
           v + "ln_post.bias": sd["post_layernorm.bias"], v + "proj": sd["visual_projection.weight"].t().contiguous()}
    layer = 0
    while f"encoder.layers.{layer}.layer_norm1.weight" in sd:
        s, d = f"encoder.layers.{layer}.", f"{v}transformer.resblocks.{layer}."
        out[d + "attn.in_proj_weight"] = torch.cat([sd[s + f"self_attn.{t}_proj.weight"] for t in "qkv"])
        out[d + "attn.in_proj_bias"] = torch.cat([sd[s + f"self_attn.{t}_proj.bias"] for t in "qkv"])
        for src, dst in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                         ("mlp.fc2", "mlp.c_proj")):
            out[d + dst + ".weight"], out[d + dst + ".bias"] = sd[s + src + ".weight"], sd[s + src + ".bias"]
        layer += 1
    out["logit_scale"] = torch.tensor(4.6052)                       # a key of the text side: ignored by the mapping
    return out


# ---- Pillow's 8-bit bicubic resize, restated -------------------------------------------------------------------------------------
def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pillow_tables(n_in: int, n_out: int):
    """Per output index: (xmin, integer taps scaled by 2^22) -- scale, support, centre, bounds and taps in double, the taps summed
    in order and each divided by the sum, then int(+-0.5 + w 2^22) truncating toward zero."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = [_bicubic((x + xmin - center + 0.5) / fs) for x in range(xmax - xmin)]
        tot = 0.0
        for v in w:
            tot += v
        k = [int((-0.5 if v / tot < 0 else 0.5) + (v / tot) * 2.0 ** 22) for v in w]
        out.append((xmin, np.asarray(k, dtype=np.int64)))
    return out


def _pass(img: np.ndarray, tables) -> np.ndarray:
    """One pass along axis 1 of img [rows, n_in, ch] uint8 -> [rows, n_out, ch] uint8."""
    out = np.empty((img.shape[0], len(tables), img.shape[2]), dtype=np.uint8)
    src = img.astype(np.int64)
    for i, (xmin, k) in enumerate(tables):
        acc = (src[:, xmin:xmin + len(k)] * k[None, :, None]).sum(axis=1) + (1 << 21)
        out[:, i] = np.clip(acc >> 22, 0, 255)
    return out


def pillow_resize(img: np.ndarray, size: int) -> np.ndarray:
    """PIL.Image.resize((size, size), BICUBIC) of a square uint8 image [S, S, 3]: the horizontal pass over every row, rounded to
    uint8, then the same pass down the columns of that intermediate."""
    if img.shape[0] == size:
        return img.copy()
    t = pillow_tables(img.shape[0], size)
    h = _pass(img, t)
    return np.ascontiguousarray(_pass(np.ascontiguousarray(h.transpose(1, 0, 2)), t).transpose(1, 0, 2))


def preprocess(u8: torch.Tensor) -> torch.Tensor:
    """ToTensor + Normalize of uint8 [B, T, T, 3] -> f32 [B, 3, T, T], the f32 operations in torchvision's order.  The divisor is a
    tensor: with a host scalar torch's GPU kernel multiplies by the rounded reciprocal instead, which is not the division torchvision
    performs on the CPU, and the subtraction that follows amplifies that last-place difference without bound near u / 255 = mean."""
    x = u8.permute(0, 3, 1, 2).to(torch.float32)
    x = x / torch.full_like(x, 255.0)
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32, device=u8.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=torch.float32, device=u8.device).view(1, 3, 1, 1)
    return (x - mean) / std


class SimClassifier(torch.nn.Module):
    """run_nudity_sdv3.py:105-118, restated."""

    def __init__(self, embeddings):
        super().__init__()
        self.embeddings = torch.nn.parameter.Parameter(embeddings)

    def forward(self, x):
        embeddings_norm = self.embeddings / self.embeddings.norm(dim=-1, keepdim=True)
        image_features_norm = x / x.norm(dim=-1, keepdim=True)
        similarity = (100.0 * image_features_norm @ embeddings_norm.T)
        return similarity.squeeze()


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())
