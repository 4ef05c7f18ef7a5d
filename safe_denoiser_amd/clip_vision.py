"""CLIP ViT vision tower and the Q16 classifier: what the reference asks of every generated image under `category == 'all'`
(run_nudity_sdv3.py:93-118,141-193 and the same code in the other drivers) -- `clip.preprocess(img)`, `clip_model.encode_image(x)`
of OpenAI CLIP ViT-L/14, and a cosine-similarity head against two learned prompt embeddings -- executed by libsdn
(sdn_clip_vision_create / sdn_clip_vision_forward, sdn_image_resize_u8, sdn_clip_normalize_u8).

CLIPVisionModelWithProjection takes a transformers CLIPVisionModelWithProjection state_dict (keys with or without the
`vision_model.` prefix; it is arithmetically the OpenAI tower) or, through from_openai_state_dict, the OpenAI checkpoint's own
`visual.*` keys.  Neither the OpenAI `clip` package nor torchvision is needed: for the SQUARE images the engine produces,
torchvision's Resize(224, BICUBIC) + CenterCrop + ToTensor + Normalize on a PIL image is PIL.Image.resize((224, 224), BICUBIC)
followed by ((u8 / 255) - mean) / std, and Pillow's 8-bit resize is integer arithmetic that sdn_image_resize_u8 reproduces bit for
bit from coefficient tables built here in double (resize_tables).  Non-square inputs are refused there; resize_rect /
resize_rect_u8 (sdn_image_resize_rect_u8) resample images of any aspect ratio with Pillow's bilinear or bicubic filter -- the
transform of the negative reference images (safe_denoiser_amd/data.py) -- and clip_preprocess_any is CLIP's preprocessing for any
aspect ratio (shortest side to 224, centre crop), computing only the crop window.
"""
from __future__ import annotations

import math
import pickle
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .clip import ACT_CODES
from ._model import HALF_DTYPES, EngineModel

VIT_L14_CONFIG = dict(image_size=224, patch_size=14, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24,
                      num_attention_heads=16, projection_dim=768, hidden_act="quick_gelu")
# laion/CLIP-ViT-H-14-laion2B-s32B-b79K, the COCO driver's evaluator (run_coco30k.py:177-182): 16 heads of 80
VIT_H14_CONFIG = dict(image_size=224, patch_size=14, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32,
                      num_attention_heads=16, projection_dim=1024, hidden_act="gelu")
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)                   # clip.preprocess's Normalize
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22                                                # Pillow: 32 - 8 - 2


# ---- preprocessing --------------------------------------------------------------------------------------------------------------
def _bicubic(x: float, a: float = -0.5) -> float:
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}      # Pillow's (filter, support)


def resize_tables(in_size: int, out_size: int, filter: str = "bicubic"):
    """Pillow's coefficient tables for one axis and one of its filters, in double (Python floats): (coeffs int32 [out, ksize] = the
    normalised taps times 2^22, rounded half away from zero; bounds int32 [out, 2] = (first input index, tap count); ksize)."""
    if filter not in FILTERS:
        raise _lib.SdnError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    fn, radius = FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = radius * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5))
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        total = 0.0
        for v in w:                                                # summed in tap order, as Pillow does
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        for x, v in enumerate(w):
            coeffs[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[i] = (xmin, xmax - xmin)
    return coeffs, bounds, ksize


_TABLES: dict = {}


def _device_tables(in_size: int, out_size: int, device, filter: str = "bicubic"):
    key = (in_size, out_size, filter, str(device))
    t = _TABLES.get(key)
    if t is None:
        coeffs, bounds, ksize = resize_tables(in_size, out_size, filter)
        t = (torch.from_numpy(coeffs).to(device), torch.from_numpy(bounds).to(device), ksize)
        _TABLES[key] = t
    return t


def _as_u8_batches(images, device):
    """uint8 device tensors [b, S, S, 3] in input order: the tensor itself, or the PIL images grouped by runs of equal size."""
    if isinstance(images, torch.Tensor):
        t = images
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise _lib.SdnError(f"images must be uint8 [B, S, S, 3], got {t.dtype} {tuple(t.shape)}")
        if t.shape[1] != t.shape[2]:
            raise _lib.SdnError(f"only square images are implemented, got {t.shape[2]} x {t.shape[1]}")
        return [t.to(device).contiguous()]
    out, run = [], []
    for im in list(images):
        if not hasattr(im, "size") or not hasattr(im, "convert"):
            raise _lib.SdnError("images must be a uint8 tensor [B, S, S, 3] or a list of PIL images")
        w, h = im.size
        if w != h:
            raise _lib.SdnError(f"only square images are implemented, got {w} x {h}")
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if run and run[-1].shape != a.shape:
            out.append(torch.from_numpy(np.stack(run)).to(device))
            run = []
        run.append(a)
    if run:
        out.append(torch.from_numpy(np.stack(run)).to(device))
    return out


def resize_u8(images_u8: torch.Tensor, size: int = 224) -> torch.Tensor:
    """PIL.Image.resize((size, size), BICUBIC) of every image of a uint8 GPU tensor [B, S, S, 3], bit for bit."""
    _lib.require_gpu()
    t = images_u8
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or not t.is_cuda:
        raise _lib.SdnError("images must be a uint8 GPU tensor [B, S, S, 3]")
    b, s = t.shape[0], t.shape[1]
    if t.shape[2] != s:
        raise _lib.SdnError(f"only square images are implemented, got {t.shape[2]} x {s}")
    t = t.contiguous()
    if s == size or b == 0:
        return t.clone()                                           # Image.resize to the same size is a copy
    coeffs, bounds, ksize = _device_tables(s, size, t.device)
    tmp = torch.empty((b, s, size, 3), dtype=torch.uint8, device=t.device)
    out = torch.empty((b, size, size, 3), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.lib().sdn_image_resize_u8(t.data_ptr(), b, s, size, coeffs.data_ptr(), bounds.data_ptr(), ksize, tmp.data_ptr(),
                                              out.data_ptr(), _lib.stream_ptr()), "sdn_image_resize_u8")
    return out


def resize_rect(images_u8: torch.Tensor, size, filter: str = "bilinear", mean=None, std=None, want_u8: bool = True):
    """PIL.Image.resize((out_w, out_h), filter) of every image of a uint8 GPU tensor [B, H, W, 3], any aspect ratio, for
    size = (out_h, out_w): (uint8 [B, out_h, out_w, 3] or None, f32 [B, 3, out_h, out_w] = ((u8 / 255) - mean) / std or None when
    mean is None).  The f32 planes are written by the resize's last pass; they are normalize_u8's bits of the uint8 result."""
    _lib.require_gpu()
    t = images_u8
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or not t.is_cuda:
        raise _lib.SdnError("images must be a uint8 GPU tensor [B, H, W, 3]")
    if filter not in FILTERS:
        raise _lib.SdnError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    out_h, out_w = (int(v) for v in size)
    want_f32 = mean is not None
    if not want_u8 and not want_f32:
        raise _lib.SdnError("nothing to compute: want_u8 is False and no mean / std is given")
    if want_f32 and std is None:
        raise _lib.SdnError("std is required with mean")
    t = t.contiguous()
    b, h, w = t.shape[0], t.shape[1], t.shape[2]
    dev = t.device
    cx, bx, kx = _device_tables(w, out_w, dev, filter) if w != out_w else (None, None, 0)      # an unchanged axis has no pass
    cy, by, ky = _device_tables(h, out_h, dev, filter) if h != out_h else (None, None, 0)
    tmp = torch.empty((b, h, out_w, 3), dtype=torch.uint8, device=dev) if cx is not None and cy is not None else None
    u8 = torch.empty((b, out_h, out_w, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    f32 = torch.empty((b, 3, out_h, out_w), dtype=torch.float32, device=dev) if want_f32 else None
    m = [float(v) for v in mean] if want_f32 else [0.0, 0.0, 0.0]
    s = [float(v) for v in std] if want_f32 else [1.0, 1.0, 1.0]
    _lib.check(_lib.lib().sdn_image_resize_rect_u8(t.data_ptr(), b, h, w, out_h, out_w, _lib.dptr(cx), _lib.dptr(bx), kx, _lib.dptr(cy),
                                                   _lib.dptr(by), ky, _lib.dptr(tmp), _lib.dptr(u8), _lib.dptr(f32), *m, *s,
                                                   _lib.stream_ptr()), "sdn_image_resize_rect_u8")
    return u8, f32


def resize_rect_u8(images_u8: torch.Tensor, size, filter: str = "bilinear") -> torch.Tensor:
    """PIL.Image.resize((out_w, out_h), BILINEAR | BICUBIC) of every image of a uint8 GPU tensor [B, H, W, 3], bit for bit;
    size = (out_h, out_w)."""
    return resize_rect(images_u8, size, filter)[0]


def normalize_u8(images_u8: torch.Tensor, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """f32 [B, 3, T, T] = ((u8 / 255) - mean) / std of a uint8 GPU tensor [B, T, T, 3]."""
    _lib.require_gpu()
    t = images_u8
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or t.shape[1] != t.shape[2] or not t.is_cuda:
        raise _lib.SdnError("images must be a uint8 GPU tensor [B, T, T, 3]")
    t = t.contiguous()
    out = torch.empty((t.shape[0], 3, t.shape[1], t.shape[2]), dtype=torch.float32, device=t.device)
    _lib.check(_lib.lib().sdn_clip_normalize_u8(t.data_ptr(), t.shape[0], t.shape[1], *[float(v) for v in mean], *[float(v) for v in std],
                                                out.data_ptr(), _lib.stream_ptr()), "sdn_clip_normalize_u8")
    return out


def clip_preprocess(images, size: int = 224, device="cuda") -> torch.Tensor:
    """`torch.stack([clip.preprocess(img) for img in images])` for square images: a uint8 tensor [B, S, S, 3] (the output of
    decode_latents_uint8) or a list of square PIL images -> pixel_values f32 [B, 3, size, size] on the GPU."""
    _lib.require_gpu()
    if isinstance(images, torch.Tensor) and images.is_cuda:
        device = images.device
    parts = [normalize_u8(resize_u8(t, size)) for t in _as_u8_batches(images, device)]
    if not parts:
        return torch.empty((0, 3, size, size), dtype=torch.float32, device=device)
    return parts[0] if len(parts) == 1 else torch.cat(parts)


# ---- any aspect ratio: shortest side to `size`, centre crop ------------------------------------------------------------------------
CROP_RULES = ("transformers", "torchvision")


def resized_shape(h: int, w: int, size: int) -> tuple:
    """(height, width) after `resize(shortest_edge=size)`: the short side becomes `size`, the long one int(size * long / short)
    (transformers' get_resize_output_image_size and torchvision's Resize(int) agree on this)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def crop_offset(length: int, size: int, crop: str = "transformers") -> int:
    """First kept index of a centre crop of `size` out of `length` >= size.  transformers' center_crop: (length - size) // 2.
    torchvision's CenterCrop: int(round((length - size) / 2.0)) with Python's round (half to even) -- written from its source;
    torchvision is not installed where this was developed, so that rule is UNVERIFIED against the library.  The two differ when
    the excess is odd and (excess - 1) / 2 is odd."""
    if crop not in CROP_RULES:
        raise _lib.SdnError(f"crop must be one of {CROP_RULES}, got {crop!r}")
    if length < size:
        raise _lib.SdnError(f"cannot crop {size} out of {length}")
    return (length - size) // 2 if crop == "transformers" else int(round((length - size) / 2.0))


def crop_tables(n_in: int, n_res: int, off: int, size: int, filter: str = "bicubic"):
    """One axis of resize-then-crop as ONE table set for sdn_image_resize_rect_u8 with `size` outputs: rows [off, off + size) of
    resize_tables(n_in, n_res) -- each output of Pillow's pass depends on its own taps only, so the cropped resize is bit for bit
    the crop of the resize.  An axis Pillow does not resample (n_res == n_in) gets the one-tap table of weight 2^22 at off + i,
    which reproduces the source byte ((2^21 + 2^22 u) >> 22 = u), or None when nothing is cropped either (no pass at all)."""
    if n_res == n_in:
        if n_in == size:
            return None
        coeffs = np.full((size, 1), 1 << PRECISION_BITS, dtype=np.int32)
        bounds = np.stack([np.arange(off, off + size, dtype=np.int32), np.ones(size, dtype=np.int32)], axis=1)
        return coeffs, np.ascontiguousarray(bounds), 1
    coeffs, bounds, ksize = resize_tables(n_in, n_res, filter)
    return np.ascontiguousarray(coeffs[off:off + size]), np.ascontiguousarray(bounds[off:off + size]), ksize


def _device_crop_tables(n_in: int, n_res: int, off: int, size: int, device):
    key = ("crop", n_in, n_res, off, size, str(device))
    if key not in _TABLES:
        t = crop_tables(n_in, n_res, off, size)
        _TABLES[key] = (None, None, 0) if t is None else (torch.from_numpy(t[0]).to(device), torch.from_numpy(t[1]).to(device), t[2])
    return _TABLES[key]


def _as_u8_groups(images, device):
    """uint8 device tensors [b, H, W, 3] in input order, any H and W: the tensor itself, or the PIL images grouped by runs of equal
    size (one launch per run)."""
    if isinstance(images, torch.Tensor):
        t = images
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise _lib.SdnError(f"images must be uint8 [B, H, W, 3], got {t.dtype} {tuple(t.shape)}")
        return [t.to(device).contiguous()]
    out, run = [], []
    for im in list(images):
        if not hasattr(im, "size") or not hasattr(im, "convert"):
            raise _lib.SdnError("images must be a uint8 tensor [B, H, W, 3] or a list of PIL images")
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if run and run[-1].shape != a.shape:
            out.append(torch.from_numpy(np.stack(run)).to(device))
            run = []
        run.append(a)
    if run:
        out.append(torch.from_numpy(np.stack(run)).to(device))
    return out


def clip_preprocess_any(images, size: int = 224, crop: str = "transformers", device="cuda") -> torch.Tensor:
    """CLIP's preprocessing for images of ANY aspect ratio: a list of PIL images (any sizes) or a uint8 tensor [B, H, W, 3] ->
    pixel_values f32 [B, 3, size, size] on the GPU.  The shortest side is resized to `size` with Pillow's bicubic filter (the long
    side to int(size * long / short)), the centre `size` x `size` is cropped, and ((u8 / 255) - CLIP_MEAN) / CLIP_STD is taken.
    Only the crop is computed (crop_tables), bit for bit Pillow's resize followed by the crop.
    crop = "transformers" (default): CLIPImageProcessor's rule, what CLIPProcessor applies on the reference's `coco` path;
    crop = "torchvision": CenterCrop's rule (open_clip's transform) -- unverified against the library, see crop_offset."""
    _lib.require_gpu()
    if crop not in CROP_RULES:
        raise _lib.SdnError(f"crop must be one of {CROP_RULES}, got {crop!r}")
    if isinstance(images, torch.Tensor) and images.is_cuda:
        device = images.device
    parts = []
    for t in _as_u8_groups(images, device):
        b, h, w = t.shape[0], t.shape[1], t.shape[2]
        if b == 0:
            continue
        rh, rw = resized_shape(h, w, size)
        top, left = crop_offset(rh, size, crop), crop_offset(rw, size, crop)
        if (rh != h and h == size) or (rw != w and w == size):
            # an axis that is resampled although it already has `size` entries (an upscale of an image whose LONG side is `size`):
            # the rectangular resize takes no table for an axis that keeps its length, so resize in full and crop
            u8 = resize_rect(t, (rh, rw), "bicubic")[0][:, top:top + size, left:left + size].contiguous()
            parts.append(normalize_u8(u8))
            continue
        cx, bx, kx = _device_crop_tables(w, rw, left, size, t.device)
        cy, by, ky = _device_crop_tables(h, rh, top, size, t.device)
        tmp = torch.empty((b, h, size, 3), dtype=torch.uint8, device=t.device) if cx is not None and cy is not None else None
        f32 = torch.empty((b, 3, size, size), dtype=torch.float32, device=t.device)
        _lib.check(_lib.lib().sdn_image_resize_rect_u8(t.data_ptr(), b, h, w, size, size, _lib.dptr(cx), _lib.dptr(bx), kx, _lib.dptr(cy),
                                                       _lib.dptr(by), ky, _lib.dptr(tmp), None, f32.data_ptr(), *CLIP_MEAN, *CLIP_STD,
                                                       _lib.stream_ptr()), "sdn_image_resize_rect_u8")
        parts.append(f32)
    if not parts:
        return torch.empty((0, 3, size, size), dtype=torch.float32, device=device)
    return parts[0] if len(parts) == 1 else torch.cat(parts)


# ---- the tower ------------------------------------------------------------------------------------------------------------------
class VisionOutput(tuple):
    """(image_embeds, last_hidden_state) with attribute access, like transformers' CLIPVisionModelOutput."""

    def __new__(cls, image_embeds, last_hidden_state):
        o = super().__new__(cls, (image_embeds, last_hidden_state))
        o.image_embeds, o.last_hidden_state = image_embeds, last_hidden_state
        return o


def convert_openai_state_dict(sd: dict) -> dict:
    """The OpenAI CLIP checkpoint's `visual.*` tensors under transformers' CLIPVisionModelWithProjection keys (host side, views)."""
    v = "visual."
    out = {"embeddings.class_embedding": sd[v + "class_embedding"],
           "embeddings.patch_embedding.weight": sd[v + "conv1.weight"],
           "embeddings.position_embedding.weight": sd[v + "positional_embedding"],
           "pre_layrnorm.weight": sd[v + "ln_pre.weight"], "pre_layrnorm.bias": sd[v + "ln_pre.bias"],
           "post_layernorm.weight": sd[v + "ln_post.weight"], "post_layernorm.bias": sd[v + "ln_post.bias"],
           "visual_projection.weight": sd[v + "proj"].t()}
    layer = 0
    while f"{v}transformer.resblocks.{layer}.ln_1.weight" in sd:
        s, d = f"{v}transformer.resblocks.{layer}.", f"encoder.layers.{layer}."
        c = sd[s + "attn.in_proj_weight"].shape[0] // 3
        for i, t in enumerate("qkv"):
            out[d + f"self_attn.{t}_proj.weight"] = sd[s + "attn.in_proj_weight"][i * c:(i + 1) * c]
            out[d + f"self_attn.{t}_proj.bias"] = sd[s + "attn.in_proj_bias"][i * c:(i + 1) * c]
        for src, dst in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
                         ("mlp.c_proj", "mlp.fc2")):
            out[d + dst + ".weight"], out[d + dst + ".bias"] = sd[s + src + ".weight"], sd[s + src + ".bias"]
        layer += 1
    if layer == 0:
        raise KeyError("no visual.transformer.resblocks.* keys: not an OpenAI CLIP ViT state_dict")
    return out


class CLIPVisionModelWithProjection(EngineModel):
    def __init__(self, dtype=torch.float16, **config):
        """dtype = fp16 (the reference's: clip.load on a GPU) or bf16 storage; config = transformers' CLIPVisionConfig fields
        (defaults: ViT-L/14; VIT_H14_CONFIG is ViT-H/14).  Heads of 64 or of 80."""
        code = self._storage(dtype, None, HALF_DTYPES,
                             "storage dtype must be torch.float16 or torch.bfloat16 (the fp32-storage plans are not built for this model)")
        cfg = dict(VIT_L14_CONFIG)
        cfg.update(config)
        if cfg["hidden_act"] not in ACT_CODES:
            raise _lib.SdnError(f"hidden_act must be one of {sorted(ACT_CODES)}, got {cfg['hidden_act']!r}")
        self.config = SimpleNamespace(**cfg)
        c = _lib.ClipVisionConfig(image_size=cfg["image_size"], patch_size=cfg["patch_size"], hidden_size=cfg["hidden_size"],
                                  intermediate_size=cfg["intermediate_size"], num_layers=cfg["num_hidden_layers"],
                                  num_heads=cfg["num_attention_heads"], projection_dim=cfg["projection_dim"],
                                  act=ACT_CODES[cfg["hidden_act"]], dtype=code)
        self._create("sdn_clip_vision_create", c)
        self.num_tokens = 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2
        # images of one launch plan: the GEMM tiles address an operand with 31-bit byte offsets
        widest = max(cfg["intermediate_size"], 3 * cfg["hidden_size"], self._kpad())
        self.max_batch = max(1, ((1 << 31) - 4096) // (2 * widest * self.num_tokens))

    PATCH_KEY = "embeddings.patch_embedding.weight"

    def _kpad(self) -> int:
        return next(p["cols"] for p in self.manifest if p["name"] == self.PATCH_KEY)

    def _source_shape(self, p: dict) -> tuple:
        ps = self.config.patch_size
        return (self.config.hidden_size, 3, ps, ps) if p["name"] == self.PATCH_KEY else super()._source_shape(p)

    @staticmethod
    def _canonical(sd: dict) -> dict:
        return {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}

    def _pack_one(self, p: dict, t: torch.Tensor) -> torch.Tensor:
        """The patch weight flattened in (c, ky, kx) order and zero-padded to the GEMM's k-tile."""
        if tuple(t.shape) != self._source_shape(p):
            raise _lib.SdnError(f"{p['name']}: expected shape {self._source_shape(p)}, got {tuple(t.shape)}")
        if p["name"] == self.PATCH_KEY:
            t = torch.nn.functional.pad(t.detach().reshape(p["rows"], -1), (0, p["cols"] - 3 * self.config.patch_size ** 2))
        return super()._pack_one(p, t)

    @classmethod
    def from_pretrained(cls, local_dir: str, dtype=torch.float16, device="cuda"):
        """A local directory with config.json + safetensors (or .bin) weights of a transformers CLIPVisionModelWithProjection, or of a
        whole CLIPModel (whose vision_config and vision_model.* / visual_projection.weight tensors are used)."""
        from . import checkpoint
        m = cls(dtype=dtype, **checkpoint.clip_vision_kwargs(checkpoint.read_config(local_dir)))
        m.load_state_dict(checkpoint.load_weights(local_dir), device)
        return m

    @classmethod
    def from_openai_state_dict(cls, sd: dict, dtype=torch.float16, device="cuda"):
        """The checkpoint the reference loads (`clip.load('ViT-L/14')`): its state_dict's `visual.*` tensors; the configuration is read
        off their shapes.  (A TorchScript archive has to be opened by the caller: pass `torch.jit.load(path).state_dict()`.)"""
        t = convert_openai_state_dict(sd)
        hidden, patch = t[cls.PATCH_KEY].shape[0], t[cls.PATCH_KEY].shape[-1]
        grid = math.isqrt(t["embeddings.position_embedding.weight"].shape[0] - 1)
        if hidden % 64 != 0 or grid * grid + 1 != t["embeddings.position_embedding.weight"].shape[0]:
            raise NotImplementedError("visual tower: only ViT towers with heads of 64 and a square patch grid are implemented")
        layers = sum(1 for k in t if k.endswith(".layer_norm1.weight"))
        m = cls(dtype=dtype, image_size=grid * patch, patch_size=patch, hidden_size=hidden,
                intermediate_size=t["encoder.layers.0.mlp.fc1.weight"].shape[0], num_hidden_layers=layers, num_attention_heads=hidden // 64,
                projection_dim=t["visual_projection.weight"].shape[0], hidden_act="quick_gelu")
        m.load_state_dict(t, device)
        return m

    def forward(self, pixel_values: torch.Tensor, output_hidden_state: bool = True) -> VisionOutput:
        """image_embeds [B, projection_dim] and last_hidden_state [B, 1 + P, hidden] (the encoder output before post_layernorm; None
        when output_hidden_state is False) of pixel_values f32 [B, 3, S, S]."""
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        s, c = self.config.image_size, self.config.hidden_size
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, s, s):
            raise _lib.SdnError(f"pixel_values must be [B, 3, {s}, {s}], got {tuple(pixel_values.shape)}")
        dev = self._weights.device
        x = pixel_values.to(device=dev, dtype=torch.float32).contiguous()
        b = x.shape[0]
        embeds = torch.empty((b, self.config.projection_dim), dtype=self.dtype, device=dev)
        hidden = torch.empty((b, self.num_tokens, c), dtype=self.dtype, device=dev) if output_hidden_state else None
        for lo in range(0, b, self.max_batch):                      # consecutive chunks on the same stream and workspace size class
            nb = min(self.max_batch, b - lo)
            ws = self._workspace(nb, dev)
            _lib.check(_lib.lib().sdn_clip_vision_forward(self._h, _lib.dptr(self._weights), x[lo:lo + nb].data_ptr(),
                                                          None if hidden is None else hidden[lo:lo + nb].data_ptr(),
                                                          embeds[lo:lo + nb].data_ptr(), nb, _lib.dptr(ws), ws.numel(), _lib.stream_ptr()),
                       "sdn_clip_vision_forward")
        return VisionOutput(embeds, hidden)

    __call__ = forward


# ---- Q16 ------------------------------------------------------------------------------------------------------------------------
def q16_similarity(image_embeds: torch.Tensor, prompts: torch.Tensor) -> torch.Tensor:
    """SimClassifier.forward without its squeeze: 100 * normalize(x) @ normalize(e).T, in f32."""
    x, e = image_embeds.float(), prompts.to(image_embeds.device).float()
    x = x / x.norm(dim=-1, keepdim=True)
    e = e / e.norm(dim=-1, keepdim=True)
    return 100.0 * x @ e.T


class Q16Classifier:
    """`Eval` of the reference for category 'all' (run_nudity_sdv3.py:151-161,176-193): preprocessing, the vision tower and the
    two-prompt head (label 1 = inappropriate).  An instance is a valid `eval_func` of driver.run_job."""

    def __init__(self, vision: CLIPVisionModelWithProjection, prompts):
        p = torch.as_tensor(np.asarray(prompts) if not isinstance(prompts, torch.Tensor) else prompts).detach().float()
        if p.dim() != 2 or tuple(p.shape) != (2, vision.config.projection_dim):
            raise _lib.SdnError(f"prompts must be [2, {vision.config.projection_dim}], got {tuple(p.shape)}")
        self.vision, self.prompts = vision, p

    @staticmethod
    def load_prompts(path: str) -> torch.Tensor:
        """The reference's load_prompts: a `.pt` tensor, or a pickled array (`prompts.p`); values pass through fp16 as they do there."""
        if path.rsplit(".", 1)[-1] == "pt":
            data = torch.load(path, map_location="cpu", weights_only=True)
        else:
            with open(path, "rb") as f:
                data = torch.as_tensor(np.asarray(pickle.load(f)))
        return data.detach().to(torch.float16).float()

    def similarity(self, images) -> torch.Tensor:
        pv = clip_preprocess(images, self.vision.config.image_size)
        return q16_similarity(self.vision(pv, output_hidden_state=False).image_embeds, self.prompts)

    def classify(self, images_u8):
        """(labels [B] int64, similarity [B, 2] f32) of a decoded batch: uint8 [B, S, S, 3] on the GPU, or a list of PIL images."""
        sim = self.similarity(images_u8)
        return sim.argmax(dim=-1), sim

    def __call__(self, samples, threshold: float = 0.6):
        """(unsafe: bool, pred) as Eval.__call__ returns them: unsafe = any image's label is 1; pred = the larger similarity, a float
        for one image and an array for several.  `threshold` is accepted and unused, as there."""
        preds = self.similarity(samples).squeeze()
        labels = torch.argmax(preds, dim=-1)
        pred = torch.max(preds, dim=-1)[0]
        pred = pred.item() if pred.ndim == 0 else pred.detach().cpu().numpy()
        unsafe = bool(labels.detach().cpu()) if len(samples) == 1 else bool(labels.detach().cpu().max())
        return unsafe, pred
