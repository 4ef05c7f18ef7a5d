"""The two image metrics of the reference's result tables, on the engine: the CLIP score (evaluate_coco30k_fid_clip.py and
evaluate_copro_aes_clip.py -> evaluations/fid.py:75-176 -> evaluations/base_image.py:145-157 -> torchmetrics' CLIPScore on
openai/clip-vit-base-patch32) and the aesthetic score (evaluate_copro_aes_clip.py -> evaluations/fid.py:178-221 ->
evaluations/base_image.py:190-203 -> evaluations/utils/aes.py; run_copro.py:170-223 carries the same head).

Everything heavy already runs in libsdn: the ViT tower (clip_vision.CLIPVisionModelWithProjection), the projected text tower
(clip.CLIPTextModelWithProjection) and Pillow's bicubic resize.  What this module adds is the scoring head on the GPU
(sdn_embed_row_scores: one scaled cosine per row), the two metric objects, the reference's three evaluators over a results tree, and
the objects `driver.run_job(metrics=...)` feeds with each decoded batch while it is still a uint8 device tensor.

Built:        CLIPScore, AestheticScore, evaluate_clip_score, evaluate_clip_score_CoPro, evaluate_aes_score_CoPro.
Unverified:   the token rule of the CLIP score for prompts longer than the text tower's position table (clip_score_ids): it is
              restated from torchmetrics' source from memory, torchmetrics is not installed where this was written.
Not built:    FID and KID (they need an Inception-v3 plan), NudeNet, and a precise-storage vision tower: the metric's vision tower
              stores 16 bits (fp16 or bf16) where torchmetrics runs the whole CLIP model in fp32, so a score carries the tower's
              16-bit error (at most 0.033 points on the test fixtures' four pairs: profiles/metrics_parity.json, synthetic weights).
An `ImageEvaluator`-shaped wrapper is deliberately absent: the three functions and the two classes are the surface.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .clip_vision import clip_preprocess
from .data import decode_workers

_CODES = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
AE_LINEARS = (0, 2, 4, 6, 7)                                       # the Linear slots of AE_MLP.layers (aes.py:54-69); the rest are Dropouts


# ---- the scoring head -----------------------------------------------------------------------------------------------------------
def embed_row_scores(x: torch.Tensor, y: torch.Tensor, normalize_y: bool, scale: float = 1.0, bias: float = 0.0) -> torch.Tensor:
    """sdn_embed_row_scores: out[i] = scale * <x_i / |x_i|, y'_j> + bias, f32 [rows].  x [rows, dim] and y [rows, dim] (paired, j = i)
    or [dim] / [1, dim] (one row for all, j = 0) are bf16 / fp16 / f32 GPU tensors, each with a dense last axis (row slices of wider
    buffers are welcome); y' = y_j / |y_j| when normalize_y, else y_j."""
    _lib.require_gpu()
    if y.dim() == 1:
        y = y.unsqueeze(0)
    if x.dim() != 2 or y.dim() != 2 or y.shape[1] != x.shape[1] or y.shape[0] not in (1, x.shape[0]):
        raise _lib.SdnError(f"x must be [rows, dim] and y [rows, dim], [1, dim] or [dim]; got {tuple(x.shape)} and {tuple(y.shape)}")
    rows, dim = x.shape
    for t, what in ((x, "x"), (y, "y")):
        if not t.is_cuda or t.dtype not in _CODES or (dim > 1 and t.stride(1) != 1):
            raise _lib.SdnError(f"{what} must be a bf16 / fp16 / f32 GPU tensor with a dense last axis")
    out = torch.empty((rows,), dtype=torch.float32, device=x.device)
    ldx = x.stride(0) if rows > 1 else max(x.stride(0), dim)
    ldy = y.stride(0) if y.shape[0] > 1 else max(y.stride(0), dim)
    _lib.check(_lib.lib().sdn_embed_row_scores(x.data_ptr(), _CODES[x.dtype], ldx, y.data_ptr(), _CODES[y.dtype], ldy, y.shape[0], rows,
                                               dim, 1 if normalize_y else 0, float(scale), float(bias), out.data_ptr(), _lib.stream_ptr()),
               "sdn_embed_row_scores")
    return out


class _ScoreState:
    """Per-sample f32 scores in update order, in a device buffer that grows by doubling.  Appending is stream-ordered device work:
    `update` never waits for the GPU; `scores`, `state` and `compute` are where the host reads."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._buf, self._n = None, 0

    def _append(self, s: torch.Tensor):
        k = s.numel()
        if k == 0:
            return
        if self._buf is None or self._n + k > self._buf.numel():
            grown = torch.empty((max(2 * (self._n + k), 1024),), dtype=torch.float32, device=s.device)
            if self._n:
                grown[:self._n].copy_(self._buf[:self._n])
            self._buf = grown
        self._buf[self._n:self._n + k].copy_(s)
        self._n += k

    @property
    def scores(self) -> torch.Tensor:
        """f32 [n]: the per-sample scores (unclamped), in update order, on the device they were computed on."""
        return torch.empty((0,), dtype=torch.float32) if self._buf is None else self._buf[:self._n].clone()

    def state(self):
        """(sum of the per-sample scores in float64, n): what ranks add up before dividing."""
        return (float(self.scores.double().sum()) if self._n else 0.0), self._n

    def _mean(self) -> float:
        s, n = self.state()
        if n == 0:
            raise _lib.SdnError("compute() before any update()")
        return s / n


# ---- CLIP score -----------------------------------------------------------------------------------------------------------------
def clip_score_ids(tokenizer, texts, n: int):
    """(input_ids int64 [B, n], number of prompts that were cut) of a list of strings, by the rule torchmetrics' CLIPScore applies:
    its processor tokenises with padding to the longest prompt of the batch and NO truncation, and the metric then keeps the first
    `max_position_embeddings` positions of a batch that came out longer.  A prompt longer than n tokens therefore loses its tail AND
    its end-of-text token.  Here every batch is brought to exactly n columns: padded with pad_token_id when shorter (what the
    engine's text plan takes; under causal attention the pad columns do not reach the pooled row), cut when longer.

    UNVERIFIED: torchmetrics is not installed where this was written; the rule is restated from its source from memory.

    A cut row holds no end-of-text id.  The text tower pools such a row where transformers does: under the legacy rule
    (eos_token_id == 2: the first position of the HIGHEST id) at the begin-of-text token, position 0, for any real CLIP vocabulary
    (begin-of-text is the second-highest id); under the first-match rule at position 0 too (sdn_clip_eos_rows: "0 when there is
    none", transformers' argmax of an all-zero vector).  Position 0 attends to itself only, so the score of an over-long prompt is
    the score of the begin-of-text embedding -- the same for every such prompt.  `CLIPScore.n_truncated` counts them."""
    texts = [texts] if isinstance(texts, str) else list(texts)
    enc = tokenizer(texts, padding="longest", truncation=False, return_tensors="pt")
    ids = torch.as_tensor(enc.input_ids).to(torch.int64)
    mask = getattr(enc, "attention_mask", None)
    lengths = (ids != tokenizer.pad_token_id).sum(-1) if mask is None else torch.as_tensor(mask).sum(-1)
    cut = int((lengths > n).sum())
    if ids.shape[1] < n:
        ids = torch.cat([ids, torch.full((ids.shape[0], n - ids.shape[1]), tokenizer.pad_token_id, dtype=torch.int64)], dim=1)
    return ids[:, :n].contiguous(), cut


class CLIPScore(_ScoreState):
    """torchmetrics' CLIPScore (multimodal/clip_score.py, third party) on the engine's two towers: per (image, caption) pair
    100 * cos(image_embeds, text_embeds); compute() = max(mean, 0).  The reference builds it on openai/clip-vit-base-patch32
    (base_image.py:146): vision hidden 768 / 12 heads / patch 32 / projection 512, text hidden 512 / 8 heads -- geometries both
    create calls accept.  The vision tower stores 16 bits where torchmetrics runs fp32 (see the module docstring)."""

    def __init__(self, vision, text, tokenizer=None):
        pv, pt = vision.config.projection_dim, text.config.projection_dim
        if pv != pt:
            raise _lib.SdnError(f"the towers project to different widths: vision {pv}, text {pt}")
        self.vision, self.text, self.tokenizer = vision, text, tokenizer
        self.n_truncated = 0
        super().__init__()

    def reset(self):
        super().reset()
        self.n_truncated = 0

    def _ids(self, text) -> torch.Tensor:
        n = self.text.config.max_position_embeddings
        if isinstance(text, torch.Tensor):
            if text.dim() != 2 or text.shape[1] != n:
                raise _lib.SdnError(f"input_ids must be [B, {n}], got {tuple(text.shape)}")
            return text
        if self.tokenizer is None:
            raise _lib.SdnError("text given as strings needs the tokenizer this CLIPScore was built without")
        ids, cut = clip_score_ids(self.tokenizer, text, n)
        self.n_truncated += cut
        return ids

    def score(self, images, text) -> torch.Tensor:
        """f32 [B]: the unclamped score of each (image, caption) pair.  images: uint8 [B, S, S, 3] (device or host) or a list of
        square PIL images; text: a list of strings or input_ids [B, max_position_embeddings]."""
        ids = self._ids(text)
        pv = clip_preprocess(images, self.vision.config.image_size)
        if pv.shape[0] != ids.shape[0]:
            raise _lib.SdnError(f"{pv.shape[0]} images for {ids.shape[0]} captions")
        img = self.vision(pv, output_hidden_state=False).image_embeds
        txt = self.text(ids.to(img.device), output_hidden_states=True).text_embeds
        return embed_row_scores(img, txt, normalize_y=True, scale=100.0)

    def update(self, images, text):
        self._append(self.score(images, text))

    def compute(self) -> float:
        """max(mean of the per-sample scores, 0), the mean taken in float64."""
        return max(self._mean(), 0.0)


# ---- aesthetic score ------------------------------------------------------------------------------------------------------------
def compose_affine(state_dict) -> tuple:
    """(w_eff f32 [input_size], b_eff float) with AE_MLP(x) = w_eff . x + b_eff: the reference's head (aes.py:48-72) is five Linears
    with no activation between them, and its Dropouts are the identity in eval mode, so it is one affine map.  Composed in float64
    on the host from the keys layers.{0,2,4,6,7}.{weight,bias}."""
    f64 = lambda t: (t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))).to(torch.float64)
    w, b = None, None
    for i in AE_LINEARS:
        wi, bi = f64(state_dict[f"layers.{i}.weight"]), f64(state_dict[f"layers.{i}.bias"])
        if wi.dim() != 2 or bi.shape != (wi.shape[0],) or (w is not None and wi.shape[1] != w.shape[0]):
            raise _lib.SdnError(f"layers.{i}: weight {tuple(wi.shape)} / bias {tuple(bi.shape)} do not chain")
        w, b = (wi, bi) if w is None else (wi @ w, wi @ b + bi)
    if w.shape[0] != 1:
        raise _lib.SdnError(f"the last Linear must have one output, got {w.shape[0]}")
    return w[0].float().contiguous(), float(b[0])


class AestheticScore(_ScoreState):
    """AE of the reference (aes.py:7-35): CLIP ViT-L/14 image embedding, L2-normalised, through AE_MLP; one f32 score per image.
    The embedding is the tower's own 16-bit `image_embeds` (the reference's `.float()` of an fp16 tower's output: the same values)."""

    def __init__(self, vision, state_dict):
        self.w_eff, self.b_eff = compose_affine(state_dict)
        if self.w_eff.numel() != vision.config.projection_dim:
            raise _lib.SdnError(f"the head takes {self.w_eff.numel()} inputs (layers.0.weight), the tower projects to "
                                f"{vision.config.projection_dim}")
        self.vision = vision
        self._w_dev = None
        super().__init__()

    @classmethod
    def load(cls, vision, path: str):
        """The reference's checkpoint file (`torch.load(path)` there; weights_only=True here: the file holds tensors only)."""
        return cls(vision, torch.load(path, map_location="cpu", weights_only=True))

    def score(self, images) -> torch.Tensor:
        """f32 [B] of a uint8 [B, S, S, 3] tensor (device or host) or a list of square PIL images."""
        emb = self.vision(clip_preprocess(images, self.vision.config.image_size), output_hidden_state=False).image_embeds
        if self._w_dev is None or self._w_dev.device != emb.device:
            self._w_dev = self.w_eff.to(emb.device)
        return embed_row_scores(emb, self._w_dev, normalize_y=False, scale=1.0, bias=self.b_eff)

    def update(self, images, text=None):
        """`text` is accepted and unused, so that run_job can feed every scorer alike."""
        self._append(self.score(images))

    def compute(self) -> float:
        """The mean of the per-image scores, in float64.  (The reference takes np.mean over a LIST of per-batch arrays,
        base_image.py:194-203: the same number while every batch has the same length, and an error -- a ragged array -- when the
        last batch is shorter.  That is not reproduced.)"""
        return self._mean()


# ---- the evaluators (evaluations/fid.py) ----------------------------------------------------------------------------------------
def _score_dir(sample_dir: str, batch_size, scorer, prompts=None):
    """Feeds every file of sample_dir to scorer.update in batches of batch_size (all at once for None), names sorted; the next
    batch is decoded by a thread pool (PIL releases the GIL) while the GPU scores this one.  The scorer is reset first: the value is
    this directory's."""
    from PIL import Image
    names = sorted(os.listdir(sample_dir))
    captions = None if prompts is None else prompts(names)
    step = len(names) if not batch_size else int(batch_size)
    decode = lambda name: Image.open(os.path.join(sample_dir, name)).convert("RGB")
    scorer.reset()
    with ThreadPoolExecutor(max_workers=decode_workers(), thread_name_prefix="sdn-metric-decode") as pool:
        spans = [(lo, min(lo + step, len(names))) for lo in range(0, len(names), max(step, 1))]
        pending = [pool.submit(decode, n) for n in names[slice(*spans[0])]] if spans else []
        for k, (lo, hi) in enumerate(spans):
            images = [f.result() for f in pending]
            pending = [pool.submit(decode, n) for n in names[slice(*spans[k + 1])]] if k + 1 < len(spans) else []
            if captions is None:
                scorer.update(images)
            else:
                scorer.update(images, captions[lo:hi])
    return scorer.compute()


def _write(sample_dir: str, kwargs: dict, key: str, value: float) -> dict:
    import yaml
    metrics = {key: float(value)}
    with open(os.path.join(os.path.dirname(sample_dir), f"{kwargs.get('filename', 'metrics')}.yaml"), "w") as f:
        yaml.dump(metrics, f)
    return metrics


def evaluate_clip_score(sample_dir="results", dataset="sample", prompts_csv=None, batch_size=None, device=None, *, scorer, **kwargs):
    """evaluations/fid.py:75-124 (COCO): every file `<image_id>.png` of sample_dir against the `caption` of its `image_id` row of the
    pandas frame prompts_csv; writes {dirname(sample_dir)}/{filename}.yaml = {clip_score: float} and returns that dict.
    `scorer`: a CLIPScore (the caller loads the towers from local directories); `dataset` and `device` are accepted and ignored."""
    match = lambda names: prompts_csv.set_index("image_id").loc[[int(n.replace(".png", "")) for n in names], "caption"].tolist()
    return _write(sample_dir, kwargs, "clip_score", _score_dir(sample_dir, batch_size, scorer, match))


def evaluate_clip_score_CoPro(sample_dir="results", dataset="sample", prompts_csv=None, batch_size=None, device=None, *, scorer, **kwargs):
    """evaluations/fid.py:126-176 (CoPro): files `<idx>_<...>.png` against the `unsafe_prompt` of their `idx` row."""
    match = lambda names: prompts_csv.set_index("idx").loc[[int(n.split("_")[0]) for n in names], "unsafe_prompt"].tolist()
    return _write(sample_dir, kwargs, "clip_score", _score_dir(sample_dir, batch_size, scorer, match))


def evaluate_aes_score_CoPro(sample_dir="results", dataset="sample", batch_size=None, device=None, checkpoint_path=None, *, scorer, **kwargs):
    """evaluations/fid.py:178-221: the mean aesthetic score of every file of sample_dir; writes {aes_score: float}.  `scorer`: an
    AestheticScore; `checkpoint_path` is accepted and ignored like `dataset` and `device` (AestheticScore.load reads the file)."""
    return _write(sample_dir, kwargs, "aes_score", _score_dir(sample_dir, batch_size, scorer))
