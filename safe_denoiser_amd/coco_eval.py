"""The COCO driver's evaluator on the engine: `Eval` of run_coco30k.py with `--category coco` (:177-182, 217-234, 250-254) --
CLIPModel / CLIPProcessor of laion/CLIP-ViT-H-14-laion2B-s32B-b79K, `get_image_features` and `get_text_features`, and the mean of
the cosine matrix of the normalised features -- executed by libsdn: clip_preprocess_any (sdn_image_resize_rect_u8), the ViT-H/14
vision plan (sdn_clip_vision_forward, heads of 80), the projected CLIP text plan (sdn_clip_proj_forward) and the two scoring heads
sdn_embed_cross_mean (the whole matrix' mean) and sdn_embed_row_scores (paired rows).

The reference runs this model in fp32; the towers here store 16 bits (fp16 by default).  An instance is a valid `eval_func` of
driver.run_job for a `coco` job (driver.parse_coco_args).
"""
from __future__ import annotations

import torch

from . import _lib, checkpoint
from .clip import CLIPTextModelWithProjection
from .clip_vision import CLIPVisionModelWithProjection, clip_preprocess_any
from .metrics import _CODES, embed_row_scores


def embed_cross_mean(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """sdn_embed_cross_mean: `(normalize(x) @ normalize(y).T).mean()` as an f32 tensor [1] on the device, for x [rx, dim] and
    y [ry, dim] bf16 / fp16 / f32 GPU tensors with a dense last axis.  The rx x ry matrix is never formed."""
    _lib.require_gpu()
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1] or x.shape[0] < 1 or y.shape[0] < 1 or x.shape[1] < 1:
        raise _lib.SdnError(f"x must be [rx, dim] and y [ry, dim] with rx, ry, dim >= 1; got {tuple(x.shape)} and {tuple(y.shape)}")
    dim = x.shape[1]
    for t, what in ((x, "x"), (y, "y")):
        if not t.is_cuda or t.dtype not in _CODES or (dim > 1 and t.stride(1) != 1):
            raise _lib.SdnError(f"{what} must be a bf16 / fp16 / f32 GPU tensor with a dense last axis")
    scratch = torch.empty((2, dim), dtype=torch.float32, device=x.device)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    ldx = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), dim)
    ldy = y.stride(0) if y.shape[0] > 1 else max(y.stride(0), dim)
    _lib.check(_lib.lib().sdn_embed_cross_mean(x.data_ptr(), _CODES[x.dtype], ldx, x.shape[0], y.data_ptr(), _CODES[y.dtype], ldy,
                                               y.shape[0], dim, scratch.data_ptr(), out.data_ptr(), _lib.stream_ptr()),
               "sdn_embed_cross_mean")
    return out


def coco_ids(tokenizer, prompts, n: int) -> torch.Tensor:
    """input_ids int64 [B, n] of a list of strings.  `CLIPProcessor(text=, padding=True)` pads to the batch's longest prompt,
    passes an attention mask and does not truncate; the engine's text plan takes exactly n = max_position_embeddings columns, so
    every row is padded to n with the tokenizer's pad id.  The features do not change: the pooled row is the end-of-text position,
    the attention mask is causal, so no position at or before end-of-text has a padded key among the keys it sees -- the columns
    after it (pad ids here, fewer pad ids plus a padding mask there) never reach the pooled row.  A prompt of more than n tokens
    raises SdnError (the reference fails there too: an index error in the position embedding)."""
    prompts = [prompts] if isinstance(prompts, str) else list(prompts)
    enc = tokenizer(prompts, padding="longest", truncation=False, return_tensors="pt")
    ids = torch.as_tensor(enc.input_ids).to(torch.int64)
    return _pad_ids(ids, n, tokenizer.pad_token_id)


def _pad_ids(ids: torch.Tensor, n: int, pad_id) -> torch.Tensor:
    if ids.dim() != 2:
        raise _lib.SdnError(f"input_ids must be [B, <= {n}], got {tuple(ids.shape)}")
    if ids.shape[1] > n:
        raise _lib.SdnError(f"a prompt of {ids.shape[1]} tokens exceeds the text tower's {n} positions")
    if ids.shape[1] < n:
        if pad_id is None:
            raise _lib.SdnError(f"input_ids must be [B, {n}] when no tokenizer supplies a pad id, got {tuple(ids.shape)}")
        ids = torch.cat([ids, torch.full((ids.shape[0], n - ids.shape[1]), pad_id, dtype=ids.dtype, device=ids.device)], dim=1)
    return ids.contiguous()


class CocoClipEval:
    """`Eval(args)` of run_coco30k.py for category 'coco' over the engine's two towers.  With tokenizer=None the methods take
    input_ids tensors [B, max_position_embeddings] in place of strings."""

    def __init__(self, vision: CLIPVisionModelWithProjection, text: CLIPTextModelWithProjection, tokenizer=None):
        pv, pt = vision.config.projection_dim, text.config.projection_dim
        if pv != pt:
            raise _lib.SdnError(f"the towers project to different widths: vision {pv}, text {pt}")
        self.vision, self.text, self.tokenizer = vision, text, tokenizer

    @classmethod
    def from_pretrained(cls, local_dir: str, dtype=torch.float16, tokenizer=None, device="cuda"):
        """One local transformers CLIPModel directory: config.json (`vision_config`, `text_config`, `projection_dim`) and the
        weights `vision_model.*`, `text_model.*`, `visual_projection.weight`, `text_projection.weight`."""
        cfg = checkpoint.read_config(local_dir)
        vision = CLIPVisionModelWithProjection(dtype=dtype, **checkpoint.clip_vision_kwargs(cfg))
        text = CLIPTextModelWithProjection(dtype=dtype, **checkpoint.clip_model_text_kwargs(cfg))
        sd = checkpoint.load_weights(local_dir)
        vision.load_state_dict(sd, device)
        text.load_state_dict(sd, device)
        return cls(vision, text, tokenizer)

    # ---- features ----------------------------------------------------------------------------------------------------------------
    def _ids(self, prompts) -> torch.Tensor:
        n = self.text.config.max_position_embeddings
        if isinstance(prompts, torch.Tensor):
            return _pad_ids(prompts, n, getattr(self.tokenizer, "pad_token_id", None))
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        if not prompts:
            raise _lib.SdnError("no prompts")
        if self.tokenizer is None:
            raise _lib.SdnError("prompts given as strings need the tokenizer this evaluator was built without")
        return coco_ids(self.tokenizer, prompts, n)

    @staticmethod
    def _count(images) -> int:
        return images.shape[0] if isinstance(images, torch.Tensor) else len(images)

    def image_features(self, images, crop: str = "transformers") -> torch.Tensor:
        """`get_image_features` of preprocessed images: [B, projection_dim] in the towers' storage type (not normalised)."""
        if self._count(images) == 0:
            raise _lib.SdnError("no images")
        pv = clip_preprocess_any(images, self.vision.config.image_size, crop=crop)
        return self.vision(pv, output_hidden_state=False).image_embeds

    def text_features(self, prompts) -> torch.Tensor:
        """`get_text_features`: [B, projection_dim] (not normalised)."""
        ids = self._ids(prompts)
        if ids.shape[0] == 0:
            raise _lib.SdnError("no prompts")
        return self.text(ids, output_hidden_states=True).text_embeds

    # ---- the three scores --------------------------------------------------------------------------------------------------------
    def clip_score(self, images, prompts) -> float:
        """Eval.clip_score: the mean over ALL (image, prompt) pairs of the cosine of the normalised features (no factor of 100)."""
        return float(embed_cross_mean(self.image_features(images), self.text_features(prompts)))

    def pair_scores(self, images, prompts) -> torch.Tensor:
        """f32 [B] on the device: the cosine of image i with prompt i -- what `clip_score([image_i], [prompt_i])` returns, for a
        whole decoded batch in one call and without a host read."""
        img, txt = self.image_features(images), self.text_features(prompts)
        if img.shape[0] != txt.shape[0]:
            raise _lib.SdnError(f"{img.shape[0]} images for {txt.shape[0]} prompts")
        return embed_row_scores(img, txt, normalize_y=True, scale=1.0, bias=0.0)

    def measure_similarity(self, orig_images, images) -> float:
        """Eval.measure_similarity (run_coco30k.py:191-215): the mean of the image-by-image cosine matrix.  There the model is
        open_clip's ViT-H-14 and the transform open_clip's, which is torchvision's Resize + CenterCrop: hence crop="torchvision"
        (unverified against the library, see clip_vision.crop_offset), and the weights must be given in transformers' layout.
        A library call only: in the reference the `coco_open_clip` category cannot reach it -- `'coco' in args.category` is tested
        first (:483-487), and Eval.__call__ would then call it with orig_images=None -- so the driver does not use it."""
        a = self.image_features(orig_images, crop="torchvision")
        b = self.image_features(images, crop="torchvision")
        return float(embed_cross_mean(a, b))

    def __call__(self, samples, threshold: float = 0.6, org_samples=None, prompts=None):
        """(None, pred) as Eval.__call__ returns for 'coco': pred = clip_score(samples, prompts).  `threshold` and `org_samples`
        are accepted and unused, as there."""
        return None, self.clip_score(samples, prompts)
