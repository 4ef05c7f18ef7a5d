"""SD-v3 text front end on the engine: the three calls SD3SafeDenoiserPipeline makes on `text_front_end` (pipeline_sd3.py; the
reference's models/sdv3/safe_denoiser_pipeline.py:316-334, :722-771, :773-831), with all three text encoders running on libsdn:
T5-XXL (`text_encoder_3`, the only encoder the SD-v3 SAFREE decision uses) and the two projected CLIP encoders (`text_encoder` =
CLIP-L, `text_encoder_2` = OpenCLIP bigG; clip.CLIPTextModelWithProjection), so an SD-v3 run goes from prompt strings to latents
without leaving the engine.  `encode_prompt` tokenises each prompt for both CLIPs (:366-372), lets each encoder write its column
slice of ONE [P, 77 + 256, d_model] buffer (hidden_states[-2], CLIP-L first, :508-525; the columns past 2048 stay zero) and of
ONE [P, 2048] pooled buffer (:528), and puts the T5 rows behind the CLIP rows.  The three tokenizers stay with the caller.

A caller that computes the CLIP part elsewhere passes `clip_embeds(list_of_str) -> ([P, 77, c <= d_model], [P, pooled_dim])`
instead of the two encoders: the concatenated CLIP-L / CLIP-G hidden states and pooled outputs.
"""
from __future__ import annotations

import os
from typing import Callable, Optional

import torch

from . import _lib

MAX_SEQUENCE_LENGTH = 256
CLIP_SEQUENCE_LENGTH = 77


class SD3TextFrontEnd:
    def __init__(self, text_encoder_3, tokenizer_3, clip_embeds: Optional[Callable] = None, *, text_encoder=None, tokenizer=None,
                 text_encoder_2=None, tokenizer_2=None):
        clips = (text_encoder, tokenizer, text_encoder_2, tokenizer_2)
        if clip_embeds is not None and any(c is not None for c in clips):
            raise _lib.SdnError("pass either clip_embeds or text_encoder / tokenizer / text_encoder_2 / tokenizer_2, not both")
        if clip_embeds is None and any(c is None for c in clips):
            raise _lib.SdnError("without clip_embeds, all of text_encoder, tokenizer, text_encoder_2 and tokenizer_2 are needed")
        self.text_encoder_3, self.tokenizer_3, self.clip_embeds = text_encoder_3, tokenizer_3, clip_embeds
        self.text_encoder, self.tokenizer, self.text_encoder_2, self.tokenizer_2 = clips
        if clip_embeds is None:
            width = text_encoder.config.hidden_size + text_encoder_2.config.hidden_size
            if width > self.d_model:
                raise _lib.SdnError(f"the two CLIP widths add up to {width} > d_model {self.d_model}")
            if not (text_encoder.dtype == text_encoder_2.dtype == text_encoder_3.dtype):
                raise _lib.SdnError("the three text encoders must share one storage dtype")

    @classmethod
    def from_pretrained(cls, model_dir: str, *, tokenizer, tokenizer_2, tokenizer_3, dtype=torch.float16):
        """The three encoders of a diffusers-layout SD-v3 directory (text_encoder/, text_encoder_2/, text_encoder_3/: config.json +
        weights), on the engine.  The tokenizers are the caller's (their vocabulary files are not part of this engine)."""
        from . import checkpoint
        from .clip import CLIPTextModelWithProjection
        from .t5 import T5EncoderModel
        made = []
        for sub, ctor, kwargs in (("text_encoder", CLIPTextModelWithProjection, checkpoint.clip_projection_kwargs),
                                  ("text_encoder_2", CLIPTextModelWithProjection, checkpoint.clip_projection_kwargs),
                                  ("text_encoder_3", T5EncoderModel, checkpoint.t5_kwargs)):
            d = os.path.join(model_dir, sub)
            m = ctor(dtype=dtype, **kwargs(checkpoint.read_config(d)))
            m.load_state_dict(checkpoint.load_weights(d))
            made.append(m)
        return cls(made[2], tokenizer_3, text_encoder=made[0], tokenizer=tokenizer, text_encoder_2=made[1], tokenizer_2=tokenizer_2)

    @property
    def d_model(self) -> int:
        return self.text_encoder_3.config.d_model

    def masked_ids(self, prompt: str) -> torch.Tensor:
        """[n_real, n] ids: row i is the prompt with position i + 1 replaced by id 0 (:797-817).  n_real = n - 2 is the reference's
        count, kept as it is although the T5 tokenizer adds only an end token."""
        ids = self.tokenizer_3(prompt, padding="longest", max_length=MAX_SEQUENCE_LENGTH, truncation=True,
                               return_tensors="pt").input_ids
        if ids.shape[1] > MAX_SEQUENCE_LENGTH:
            ids = ids[:, :MAX_SEQUENCE_LENGTH]
        n_real = max(ids.shape[1] - 2, 0)
        masked = ids[:1].repeat(n_real, 1)
        for i in range(n_real):
            masked[i, i + 1] = 0
        return masked

    @torch.no_grad()
    def masked_encode_prompt(self, prompt: str) -> torch.Tensor:
        masked = self.masked_ids(prompt)
        if masked.shape[0] == 0:                                      # nothing to mask: no launch
            dev = "cuda" if torch.cuda.is_available() else "cpu"
            return torch.empty((0, self.d_model), dtype=self.text_encoder_3.dtype, device=dev)
        return self.text_encoder_3(masked, attention_mask=None).last_hidden_state[:, 0, :]

    @torch.no_grad()
    def encode_negative_prompt_space(self, phrases) -> torch.Tensor:
        tok = self.tokenizer_3(list(phrases), padding="max_length", max_length=MAX_SEQUENCE_LENGTH, truncation=True,
                               return_tensors="pt")
        return self.text_encoder_3(tok.input_ids, attention_mask=tok.attention_mask).last_hidden_state[:, 0, :]

    def _t5_embeds(self, prompts) -> torch.Tensor:
        ids = self.tokenizer_3(list(prompts), padding="max_length", max_length=MAX_SEQUENCE_LENGTH, truncation=True,
                               return_tensors="pt").input_ids
        return self.text_encoder_3(ids)[0]                            # no attention mask (:334)

    def clip_ids(self, prompts):
        """([P, 77], [P, 77]) token ids for text_encoder and text_encoder_2 (:366-372)."""
        return tuple(tok(list(prompts), padding="max_length", max_length=CLIP_SEQUENCE_LENGTH, truncation=True,
                         return_tensors="pt").input_ids for tok in (self.tokenizer, self.tokenizer_2))

    def _joint_on_engine(self, prompts):
        t5 = self._t5_embeds(prompts)
        p, n = len(prompts), CLIP_SEQUENCE_LENGTH
        e1, e2 = self.text_encoder, self.text_encoder_2
        c1, c2, p1, p2 = e1.config.hidden_size, e2.config.hidden_size, e1.config.projection_dim, e2.config.projection_dim
        pe = torch.zeros((p, n + t5.shape[1], t5.shape[2]), dtype=t5.dtype, device=t5.device)      # the zero padding: this one fill
        pooled = torch.empty((p, p1 + p2), dtype=t5.dtype, device=t5.device)
        ids1, ids2 = self.clip_ids(prompts)
        e1.forward_into(ids1, pe[:, :n, :c1], pooled[:, :p1])                                       # CLIP-L columns first (:508)
        e2.forward_into(ids2, pe[:, :n, c1:c1 + c2], pooled[:, p1:])
        pe[:, n:] = t5                                                                              # CLIP rows first (:525)
        return pe, pooled

    def _joint(self, prompts):
        if self.clip_embeds is None:
            return self._joint_on_engine(list(prompts))
        clip, pooled = self.clip_embeds(list(prompts))
        t5 = self._t5_embeds(prompts)
        if clip.shape[-1] > t5.shape[-1]:
            raise _lib.SdnError(f"clip_embeds returned width {clip.shape[-1]} > d_model {t5.shape[-1]}")
        clip = torch.nn.functional.pad(clip.to(device=t5.device, dtype=t5.dtype), (0, t5.shape[-1] - clip.shape[-1]))   # (:517-519)
        return torch.cat([clip, t5], dim=-2), pooled.to(device=t5.device, dtype=t5.dtype)                            # CLIP rows first (:525)

    @torch.no_grad()
    def encode_prompt(self, prompt=None, negative_prompt=None, **unused):
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        negative_prompt = negative_prompt if negative_prompt is not None else ""
        negs = [negative_prompt] * len(prompts) if isinstance(negative_prompt, str) else list(negative_prompt)
        if len(negs) != len(prompts):
            raise _lib.SdnError("prompt and negative_prompt must have the same length")
        pe, pooled = self._joint(prompts)
        npe, npooled = self._joint(negs)
        return pe, npe, pooled, npooled
