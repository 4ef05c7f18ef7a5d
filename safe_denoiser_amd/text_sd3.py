"""SD-v3 text front end on the engine's T5: the three calls SD3SafeDenoiserPipeline makes on `text_front_end`
(pipeline_sd3.py; the reference's models/sdv3/safe_denoiser_pipeline.py:316-334, :722-771, :773-831), with T5-XXL
(`text_encoder_3`, the only encoder the SD-v3 SAFREE decision uses) running on libsdn.  The two projected CLIP encoders are not
on the engine yet: the caller passes `clip_embeds(list_of_str) -> ([P, 77, c <= d_model], [P, pooled_dim])`, the concatenated
CLIP-L / CLIP-G hidden states and pooled outputs.  The T5 tokenizer stays with the caller as well.
"""
from __future__ import annotations

from typing import Callable

import torch

from . import _lib

MAX_SEQUENCE_LENGTH = 256


class SD3TextFrontEnd:
    def __init__(self, text_encoder_3, tokenizer_3, clip_embeds: Callable):
        self.text_encoder_3, self.tokenizer_3, self.clip_embeds = text_encoder_3, tokenizer_3, clip_embeds

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

    def _joint(self, prompts):
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
