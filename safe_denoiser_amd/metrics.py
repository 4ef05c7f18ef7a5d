"""The image metrics of the reference's result tables, on the engine: the CLIP score (evaluate_coco30k_fid_clip.py and
evaluate_copro_aes_clip.py -> evaluations/fid.py:75-176 -> evaluations/base_image.py:145-157 -> torchmetrics' CLIPScore on
openai/clip-vit-base-patch32) and the aesthetic score (evaluate_copro_aes_clip.py -> evaluations/fid.py:178-221 ->
evaluations/base_image.py:190-203 -> evaluations/utils/aes.py; run_copro.py:170-223 carries the same head).

Everything heavy already runs in libsdn: the ViT tower (clip_vision.CLIPVisionModelWithProjection), the projected text tower
(clip.CLIPTextModelWithProjection) and Pillow's bicubic resize.  What this module adds is the scoring head on the GPU
(sdn_embed_row_scores: one scaled cosine per row), the two metric objects, the reference's three evaluators over a results tree, and
the objects `driver.run_job(metrics=...)` feeds with each decoded batch while it is still a uint8 device tensor.

FID and KID (evaluate_coco30k_fid_clip.py:29 -> evaluations/fid.py:18-69 -> ImageEvaluator._compute_fid / _compute_kid) rest on the
Inception-v3 pool3 tower of safe_denoiser_amd/inception.py (fp32 storage, libsdn); what this module adds to it is float64
bookkeeping: the Frechet distance through symmetric eigensolvers, per-set moment sums that ranks can add up, the polynomial-kernel
MMD of KID, and `evaluate_fid`.

Built:        CLIPScore, AestheticScore, evaluate_clip_score, evaluate_clip_score_CoPro, evaluate_aes_score_CoPro,
              frechet_distance, FrechetInceptionDistance, KernelInceptionDistance, evaluate_fid.
Unverified:   KID against torchmetrics: torchmetrics (and torch-fidelity, whose Inception it runs) is not installed where this was
              written.  Upstream KID feeds uint8 images to torch-fidelity's own extractor (its own resize and (x - 128) / 128 scaling)
              and draws its subsets from torch's GLOBAL generator; here KID uses the FID tower on Pillow-resized 299 x 299 images and
              takes a `generator=`.  The MMD formula is restated from torchmetrics' source from memory.
Unverified:   the token rule of the CLIP score for prompts longer than the text tower's position table (clip_score_ids): it is
              restated from torchmetrics' source from memory, torchmetrics is not installed where this was written.
Not built:    NudeNet, the Inception score, and a precise-storage vision tower: the metric's vision tower
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


# ---- FID and KID ----------------------------------------------------------------------------------------------------------------
def _f64(a) -> np.ndarray:
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), in float64 (calculate_frechet_distance, evaluations/utils/fid.py:132-168).
    S1 S2 is similar to the symmetric positive semi-definite S1^1/2 S2 S1^1/2, so tr sqrt(S1 S2) = sum sqrt(eig(S1^1/2 S2 S1^1/2)):
    two symmetric eigen-decompositions, real by construction -- no Schur square root of a non-symmetric product, no imaginary parts
    to discard and no `eps` retry for singular covariances (fewer samples than dimensions).  With S1 = R R^T, R = V_r diag(sqrt(w_r))
    over the eigenpairs of S1 above its rounding floor (w > d eps max w), the non-zero eigenvalues of S1^1/2 S2 S1^1/2 are those of
    the r x r matrix R^T S2 R: the null space of a rank-deficient S1 (zero eigenvalues that rounding turns into +-1e-16 max w, whose
    square roots would add up to 1e-8 max w each) never enters.  Eigenvalues of R^T S2 R that rounding left below zero count as zero."""
    mu1, mu2 = np.atleast_1d(_f64(mu1)), np.atleast_1d(_f64(mu2))
    s1, s2 = np.atleast_2d(_f64(sigma1)), np.atleast_2d(_f64(sigma2))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.shape[0], mu1.shape[0]):
        raise _lib.SdnError(f"shapes do not match: mu {mu1.shape} / {mu2.shape}, sigma {s1.shape} / {s2.shape}")
    w, v = np.linalg.eigh((s1 + s1.T) / 2)
    keep = w > w.max() * w.size * np.finfo(np.float64).eps
    r = v[:, keep] * np.sqrt(w[keep])
    m = r.T @ ((s2 + s2.T) / 2) @ r
    ev = np.linalg.eigvalsh((m + m.T) / 2) if m.size else np.zeros(0)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(ev, 0.0, None)).sum())


class _Moments:
    """n, sum x and sum x x^T of a feature set, float64, on the device the features arrive on."""

    def __init__(self):
        self.n, self.sx, self.sxx = 0, None, None

    def add(self, feats: torch.Tensor):
        x = feats.detach().to(torch.float64)
        if x.dim() != 2:
            raise _lib.SdnError(f"features must be [B, dim], got {tuple(x.shape)}")
        if x.shape[0] == 0:
            return
        sx, sxx = x.sum(0), x.T @ x
        self.n, self.sx, self.sxx = self.n + x.shape[0], (sx if self.sx is None else self.sx + sx), (sxx if self.sxx is None else self.sxx + sxx)

    def merge(self, n: int, sx, sxx):
        if n == 0:
            return
        dev = self.sx.device if self.sx is not None else (sx.device if isinstance(sx, torch.Tensor) else "cpu")
        sx, sxx = (torch.as_tensor(t, dtype=torch.float64).to(dev) for t in (sx, sxx))
        self.n, self.sx, self.sxx = self.n + int(n), (sx if self.sx is None else self.sx + sx), (sxx if self.sxx is None else self.sxx + sxx)

    def mean_cov(self):
        """np.mean(act, axis=0), np.cov(act, rowvar=False) of the accumulated rows (float64 numpy)."""
        if self.n < 2:
            raise _lib.SdnError(f"a covariance needs at least 2 samples, got {self.n}")
        sx, sxx = _f64(self.sx), _f64(self.sxx)
        mu = sx / self.n
        return mu, (sxx - self.n * np.outer(mu, mu)) / (self.n - 1)


class FrechetInceptionDistance:
    """FID between a reference set (`real=True`) and a generated set: calculate_fid of the reference (evaluations/utils/fid.py:203-215).
    Per set only n, sum x and sum x x^T are kept (float64, on the device): `update` is stream-ordered device work and never waits
    for the GPU; `compute`, `statistics` and `state` are where the host reads.  `tower`: an InceptionV3 (update feeds images through
    its get_activations: Resize((256, 256)), ToTensor, the tower); None for a metric fed with features only (update_features)."""

    def __init__(self, tower=None, batch_size: int = 50):
        self.tower, self.batch_size = tower, batch_size
        self._sets = {True: _Moments(), False: _Moments()}
        self._reference = None

    def reset(self, real: bool = False):
        """Forgets the generated set (and the reference set when real=True; a loaded reference stays)."""
        self._sets[False] = _Moments()
        if real:
            self._sets[True] = _Moments()

    def update_features(self, feats: torch.Tensor, real: bool = False):
        self._sets[bool(real)].add(feats)

    def update(self, images, text=None, real: bool = False):
        """images: uint8 [B, H, W, 3] (device or host) or a list of PIL images.  `text` is accepted and unused, so that run_job can
        feed every scorer alike."""
        if self.tower is None:
            raise _lib.SdnError("this metric was built without a tower: use update_features")
        self.update_features(self.tower.get_activations(images, self.batch_size), real)

    def load_reference(self, mu, sigma):
        """Precomputed statistics of the reference set (the `.npz` files FID is usually quoted against)."""
        self._reference = (_f64(mu), _f64(sigma))

    def statistics(self, real: bool = False) -> dict:
        """{n, sum [d], outer [d, d]} of one set as float64 numpy: what ranks exchange (merge)."""
        m = self._sets[bool(real)]
        return dict(n=m.n, sum=None if m.sx is None else _f64(m.sx), outer=None if m.sxx is None else _f64(m.sxx))

    def merge(self, other, real=None):
        """Adds another instance's sums (both sets), or one set's `statistics()` dict (real = which set)."""
        if isinstance(other, FrechetInceptionDistance):
            for r in (True, False):
                o = other._sets[r]
                self._sets[r].merge(o.n, o.sx, o.sxx)
            return self
        if real is None:
            raise _lib.SdnError("merging a statistics dict needs real=True or real=False")
        self._sets[bool(real)].merge(other["n"], other["sum"], other["outer"])
        return self

    def state(self):
        """(0.0, n of the generated set): FID is not a sum over samples, so run_job's report carries n only."""
        return 0.0, self._sets[False].n

    def compute(self) -> float:
        mu1, s1 = self._reference if self._reference is not None else self._sets[True].mean_cov()
        mu2, s2 = self._sets[False].mean_cov()
        return frechet_distance(mu1, s1, mu2, s2)


def poly_mmd2(x: torch.Tensor, y: torch.Tensor, degree: int = 3, gamma=None, coef: float = 1.0) -> torch.Tensor:
    """Unbiased MMD^2 estimate under k(a, b) = (gamma <a, b> + coef)^degree, gamma = 1 / dim by default, of two equally sized
    feature sets [m, dim] (torchmetrics' poly_mmd): (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m (m - 1))
    - 2 sum_{i, j} k(x_i, y_j) / m^2.  float64."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    m = x.shape[0]
    if y.shape != x.shape or m < 2:
        raise _lib.SdnError(f"two sets of the same size >= 2 are needed, got {tuple(x.shape)} and {tuple(y.shape)}")
    g = 1.0 / x.shape[1] if gamma is None else float(gamma)
    k = lambda a, b: (a @ b.T * g + coef) ** degree
    kxx, kyy, kxy = k(x, x), k(y, y), k(x, y)
    within = (kxx.sum() - kxx.diagonal().sum()) + (kyy.sum() - kyy.diagonal().sum())
    return within / (m * (m - 1)) - 2.0 * kxy.sum() / (m * m)


class KernelInceptionDistance:
    """torchmetrics' KernelInceptionDistance as the reference uses it (evaluations/base_image.py:96-114): the polynomial-kernel MMD^2
    between `subset_size` random rows of each feature set, averaged over `subsets` draws; compute() = (mean, std), the reference
    reads the mean.  The caller sets subset_size = min(len(images), 50) as base_image.py:97 does (evaluate_fid does).
    UNVERIFIED against torchmetrics, which is not installed where this was written: upstream extracts features with
    torch-fidelity's own Inception (its own resize, (x - 128) / 128 on uint8 input) and draws the subsets from torch's global
    generator; here the features are the FID tower's on Pillow-resized 299 x 299 images (Resize((299, 299)) + ToTensor,
    base_image.py:99-101) and the draws come from `generator` when one is given (the global generator otherwise)."""

    def __init__(self, tower=None, subsets: int = 100, subset_size: int = 50, degree: int = 3, gamma=None, coef: float = 1.0,
                 generator=None, batch_size: int = 50):
        if subsets < 1 or subset_size < 2 or degree < 1:
            raise _lib.SdnError("subsets >= 1, subset_size >= 2 and degree >= 1 are needed")
        self.tower, self.subsets, self.subset_size, self.degree, self.gamma, self.coef = tower, subsets, subset_size, degree, gamma, coef
        self.generator, self.batch_size = generator, batch_size
        self._feats = {True: [], False: []}

    def reset(self, real: bool = False):
        self._feats[False] = []
        if real:
            self._feats[True] = []

    def update_features(self, feats: torch.Tensor, real: bool = False):
        self._feats[bool(real)].append(feats.detach())

    def update(self, images, text=None, real: bool = False):
        if self.tower is None:
            raise _lib.SdnError("this metric was built without a tower: use update_features")
        self.update_features(self.tower.get_activations(images, self.batch_size, size=(299, 299)), real)

    def state(self):
        return 0.0, sum(f.shape[0] for f in self._feats[False])

    def subset_indices(self, n_real: int, n_fake: int):
        """The `subsets` pairs of row indices compute() uses, in draw order: a permutation of the real rows, then one of the generated
        rows, the first subset_size of each."""
        perm = lambda n: torch.randperm(n, generator=self.generator)[:self.subset_size]
        return [(perm(n_real), perm(n_fake)) for _ in range(self.subsets)]

    def compute(self):
        real, fake = (torch.cat(self._feats[r]) if self._feats[r] else None for r in (True, False))
        if real is None or fake is None or min(real.shape[0], fake.shape[0]) < self.subset_size:
            raise _lib.SdnError(f"subset_size {self.subset_size} exceeds the number of samples of a set")
        real, fake = real.to(torch.float64), fake.to(torch.float64)
        vals = torch.stack([poly_mmd2(real[i.to(real.device)], fake[j.to(fake.device)], self.degree, self.gamma, self.coef)
                            for i, j in self.subset_indices(real.shape[0], fake.shape[0])])
        return float(vals.mean()), float(vals.std(unbiased=False))


class _Feed:
    """_score_dir's scorer interface over several metrics fed alike (one decode of every file)."""

    def __init__(self, metrics, real: bool):
        self.metrics, self.real, self.n = metrics, real, 0

    def reset(self):
        self.n = 0

    def update(self, images):
        self.n += len(images)
        for m in self.metrics:
            m.update(images, real=self.real)

    def compute(self):
        return self.n


def evaluate_fid(sample_dir="results", dataset="sample", dataset_root=None, batch_size=None, device=None, *, tower, **kwargs):
    """evaluations/fid.py:18-69: FID and KID of every file of sample_dir against every file of dataset_root; writes
    {dirname(sample_dir)}/{filename}.yaml = {fid, kid, log_kid} and returns that dict.  `tower`: an InceptionV3 with its weights
    loaded (from a local file).  KID's subset_size is min(number of samples, 50) (base_image.py:97); kwargs `subsets` and
    `generator` reach KernelInceptionDistance.  `dataset` and `device` are accepted and ignored.  log_kid is NaN when the unbiased
    KID estimate is not positive, as np.log makes it in the reference."""
    n_samples = len(os.listdir(sample_dir))
    bs = int(batch_size) if batch_size else 50
    fid = FrechetInceptionDistance(tower, batch_size=bs)
    kid = KernelInceptionDistance(tower, subsets=kwargs.get("subsets", 100), subset_size=min(n_samples, 50),
                                  generator=kwargs.get("generator"), batch_size=bs)
    _score_dir(dataset_root, batch_size, _Feed((kid, fid), real=True))
    _score_dir(sample_dir, batch_size, _Feed((kid, fid), real=False))
    k = kid.compute()[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        metrics = {"fid": float(fid.compute()), "kid": float(k), "log_kid": float(np.log(k))}
    import yaml
    with open(os.path.join(os.path.dirname(sample_dir), f"{kwargs.get('filename', 'metrics')}.yaml"), "w") as f:
        yaml.dump(metrics, f)
    return metrics
