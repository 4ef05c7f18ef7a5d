"""CLIPTextModel front-end: `text_encoder(input_ids, attention_mask=None)[0]` as the reference's pipelines call it
(models/textuals_visual/modified_safree_diffusion_pipeline_threshold_time.py:197,225,287,333), executed by libsdn's launch
plan (sdn_clip_create / sdn_clip_forward).  SURVEY section 8f row 4.

Weights: a transformers CLIPTextModel state_dict (keys with or without the `text_model.` prefix), packed once into the
engine layout by EngineModel's packer (_model.py).  The tokenizer stays with the caller (its vocabulary files are not part of this engine): pass token ids.

CLIPTextModelWithProjection is the SD-v3 form of the same encoder (`text_encoder` = CLIP-L, `text_encoder_2` = OpenCLIP bigG;
models/sdv3/safe_denoiser_pipeline.py:379-386): an inner hidden state without the final norm, and the projected pooled vector
(sdn_clip_proj_create / sdn_clip_proj_forward).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import _lib
from ._model import ALL_DTYPES, EngineModel

SD14_CLIP_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                        num_attention_heads=12, max_position_embeddings=77)


class TextEncoderOutput(tuple):
    """(last_hidden_state, pooler_output) with attribute access, like transformers' BaseModelOutputWithPooling."""

    def __new__(cls, last_hidden_state, pooler_output):
        o = super().__new__(cls, (last_hidden_state, pooler_output))
        o.last_hidden_state, o.pooler_output = last_hidden_state, pooler_output
        return o


class CLIPTextModel(EngineModel):
    def __init__(self, dtype=torch.bfloat16, precision: str | None = None, **config):
        """dtype = bf16 / fp16 storage, or torch.float32 = the plan's fp32 storage mode on the f32-input matrix cores;
        precision = "bf16x3" = fp32 storage with split-operand GEMMs on the bf16 matrix cores (the UNet's tolerance-meeting
        mode).  The reference loads the text encoder in fp32 with the rest of the pipeline (run_nudity.py:277 -> load_sd(...,
        torch.float32)); its hidden states feed every cross-attention AND the SAFREE decisions (trigger-token mask, beta ->
        step count), so the fp32-storage modes are what a seed-for-seed comparison from token ids needs."""
        code = self._storage(dtype, precision, ALL_DTYPES, "storage dtype must be torch.bfloat16, torch.float16 or torch.float32")
        cfg = dict(SD14_CLIP_CONFIG)
        cfg.update(config)
        self.config = SimpleNamespace(**cfg)
        c = _lib.ClipConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"],
                            intermediate_size=cfg["intermediate_size"], num_layers=cfg["num_hidden_layers"],
                            num_heads=cfg["num_attention_heads"], max_position_embeddings=cfg["max_position_embeddings"],
                            dtype=code)
        self._create("sdn_clip_create", c)

    @staticmethod
    def _canonical(sd: dict) -> dict:
        return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor | None = None, **unused):
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        n = self.config.max_position_embeddings
        if input_ids.dim() != 2 or input_ids.shape[1] != n:
            raise _lib.SdnError(f"input_ids must be [B,{n}] (tokenizer padding='max_length'), got {tuple(input_ids.shape)}")
        ids = input_ids.to(torch.int32).contiguous()
        mask = None if attention_mask is None else attention_mask.to(device=ids.device, dtype=torch.int32).contiguous()
        if mask is not None and tuple(mask.shape) != tuple(ids.shape):
            raise _lib.SdnError("attention_mask must have the shape of input_ids")
        b = ids.shape[0]
        out = torch.empty((b, n, self.config.hidden_size), dtype=self.dtype, device=ids.device)
        ws = self._workspace(b, ids.device)
        _lib.check(_lib.lib().sdn_clip_forward(self._h, _lib.dptr(self._weights), _lib.dptr(ids, torch.int32),
                                               None if mask is None else _lib.dptr(mask, torch.int32), _lib.dptr(out, self.dtype),
                                               b, _lib.dptr(ws), ws.numel(), _lib.stream_ptr()), "sdn_clip_forward")
        # pooled = features at the EOT token = the highest id of each sequence (CLIPTextTransformer.forward)
        pooled = out[torch.arange(b, device=ids.device), ids.argmax(dim=-1)]
        return TextEncoderOutput(out, pooled)


SD3_CLIP_L_CONFIG = dict(SD14_CLIP_CONFIG)                        # text_encoder: quick_gelu, projection_dim 768
SD3_CLIP_G_CONFIG = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32,
                         num_attention_heads=20, max_position_embeddings=77)      # text_encoder_2: gelu, projection_dim 1280
ACT_CODES = {"quick_gelu": 4, "gelu": 7}                          # SDN_ACT_QUICK_GELU, SDN_ACT_GELU


class _TappedHiddenStates:
    """`hidden_states` of a plan that computes ONE of them: indexing with the built index returns it, any other index raises."""

    def __init__(self, tensor, tap, num_layers):
        self._t, self._tap, self._n = tensor, tap, num_layers + 1

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if not isinstance(i, int) or (i if i < 0 else i - self._n) != -self._tap:
            raise _lib.SdnError(f"hidden_states[{i!r}] was not computed: this encoder was built for hidden_states[{-self._tap}] "
                                f"(clip_skip = {None if self._tap == 2 else self._tap - 2})")
        return self._t


class TextEncoderProjOutput(tuple):
    """(text_embeds, last_hidden_state = None, hidden_states) with attribute access, like transformers' CLIPTextModelOutput: the
    reference reads `out[0]` (the projected pooled vector) and `out.hidden_states[-(clip_skip + 2)]`."""

    def __new__(cls, text_embeds, hidden_states):
        o = super().__new__(cls, (text_embeds, None, hidden_states))
        o.text_embeds, o.last_hidden_state, o.hidden_states = text_embeds, None, hidden_states
        return o


class CLIPTextModelWithProjection(CLIPTextModel):
    def __init__(self, dtype=torch.bfloat16, precision: str | None = None, hidden_act: str = "quick_gelu", projection_dim: int = 768,
                 eos_token_id: int = 2, clip_skip: int | None = None, **config):
        """hidden_act "quick_gelu" (CLIP-L) or "gelu" (exact erf: OpenCLIP bigG); eos_token_id 2 = transformers' legacy pooling rule
        (the highest id), else the first position holding that id; clip_skip as the reference's encode_prompt takes it: the plan
        returns hidden_states[-(clip_skip + 2)], hidden_states[-2] for None.  dtype / precision as CLIPTextModel."""
        code = self._storage(dtype, precision, ALL_DTYPES, "storage dtype must be torch.bfloat16, torch.float16 or torch.float32")
        if hidden_act not in ACT_CODES:
            raise _lib.SdnError(f"hidden_act must be one of {sorted(ACT_CODES)}, got {hidden_act!r}")
        if clip_skip is not None and (not isinstance(clip_skip, int) or clip_skip < 0):
            raise _lib.SdnError("clip_skip must be None or a non-negative integer")
        self.clip_skip = clip_skip
        self.hidden_tap = 2 if clip_skip is None else clip_skip + 2
        cfg = dict(SD14_CLIP_CONFIG)
        cfg.update(config)
        cfg.update(hidden_act=hidden_act, projection_dim=projection_dim, eos_token_id=eos_token_id)
        self.config = SimpleNamespace(**cfg)
        c = _lib.ClipProjConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"],
                                intermediate_size=cfg["intermediate_size"], num_layers=cfg["num_hidden_layers"],
                                num_heads=cfg["num_attention_heads"], max_position_embeddings=cfg["max_position_embeddings"],
                                dtype=code,
                                projection_dim=projection_dim, act=ACT_CODES[hidden_act], eos_token_id=eos_token_id,
                                hidden_tap=self.hidden_tap)
        self._create("sdn_clip_proj_create", c)

    def forward_into(self, input_ids: torch.Tensor, hidden: torch.Tensor, text_embeds: torch.Tensor):
        """Writes hidden_states[-hidden_tap] into `hidden` [B, 77, hidden_size] and text_embeds into `text_embeds` [B, projection_dim]:
        views (column slices) of larger buffers are welcome as long as the last axis is dense and the strides are multiples of 8
        elements; nothing outside the views is written."""
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        n, c, p = self.config.max_position_embeddings, self.config.hidden_size, self.config.projection_dim
        if input_ids.dim() != 2 or input_ids.shape[1] != n:
            raise _lib.SdnError(f"input_ids must be [B,{n}] (tokenizer padding='max_length'), got {tuple(input_ids.shape)}")
        b = input_ids.shape[0]
        for t, shape, what in ((hidden, (b, n, c), "hidden"), (text_embeds, (b, p), "text_embeds")):
            if tuple(t.shape) != shape or t.dtype != self.dtype or not t.is_cuda or t.stride(-1) != 1:
                raise _lib.SdnError(f"{what} must be a {self.dtype} GPU tensor of shape {shape} with a dense last axis")
        if b == 0:
            return
        ids = input_ids.to(device=hidden.device, dtype=torch.int32).contiguous()
        ws = self._workspace(b, hidden.device)
        hb = hidden.stride(0) if b > 1 else max(hidden.stride(0), n * hidden.stride(1))
        _lib.check(_lib.lib().sdn_clip_proj_forward(self._h, _lib.dptr(self._weights), _lib.dptr(ids, torch.int32), hidden.data_ptr(),
                                                    hb, hidden.stride(1), text_embeds.data_ptr(), text_embeds.stride(0), b,
                                                    _lib.dptr(ws), ws.numel(), _lib.stream_ptr()), "sdn_clip_proj_forward")

    def __call__(self, input_ids: torch.Tensor, output_hidden_states: bool = True, **unused):
        if not output_hidden_states:
            raise _lib.SdnError("this plan exists to return a hidden state: call it with output_hidden_states=True")
        _lib.require_gpu()
        dev = self._weights.device if self._weights is not None else "cuda"
        b = input_ids.shape[0]
        hidden = torch.empty((b, self.config.max_position_embeddings, self.config.hidden_size), dtype=self.dtype, device=dev)
        embeds = torch.empty((b, self.config.projection_dim), dtype=self.dtype, device=dev)
        self.forward_into(input_ids, hidden, embeds)
        return TextEncoderProjOutput(embeds, _TappedHiddenStates(hidden, self.hidden_tap, self.config.num_hidden_layers))
