"""T5EncoderModel front-end: `text_encoder_3(input_ids, attention_mask=None)[0]` as the reference's SD-v3 pipeline calls it
(models/sdv3/safe_denoiser_pipeline.py:316-334 prompt embeddings, :731-768 concept phrases, :797-827 one sequence per real
token), executed by libsdn's launch plan (sdn_t5_create / sdn_t5_forward).

Weights: a transformers T5EncoderModel state_dict (keys with or without the `encoder.` prefix; `shared.weight` stands in for
`embed_tokens.weight`), packed once into the engine layout by EngineModel's packer (_model.py).  The tokenizer stays with the caller: pass token ids.  The sequence
length is whatever the ids have (2 .. 512): the masked-token call pads to the prompt's own length.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib
from ._model import HALF_DTYPES, P_GLU_GATE, P_GLU_VALUE, EngineModel

# T5-v1.1-XXL as SD-v3 ships it (text_encoder_3/config.json)
T5_XXL_CONFIG = dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64,
                     relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
MIN_LEN, MAX_LEN = 2, 512


class T5EncoderOutput(tuple):
    """(last_hidden_state,) with attribute access, like transformers' BaseModelOutput."""

    def __new__(cls, last_hidden_state):
        o = super().__new__(cls, (last_hidden_state,))
        o.last_hidden_state = last_hidden_state
        return o


class T5EncoderModel(EngineModel):
    def __init__(self, dtype=torch.bfloat16, **config):
        code = self._storage(dtype, None, HALF_DTYPES,
                             "storage dtype must be torch.bfloat16 or torch.float16 (fp32-storage T5 modes are not built yet)")
        cfg = dict(T5_XXL_CONFIG)
        cfg.update(config)
        self.config = SimpleNamespace(**cfg)
        c = _lib.T5Config(vocab_size=cfg["vocab_size"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], d_ff=cfg["d_ff"],
                          num_layers=cfg["num_layers"], num_heads=cfg["num_heads"],
                          num_buckets=cfg["relative_attention_num_buckets"], max_distance=cfg["relative_attention_max_distance"],
                          eps=cfg["layer_norm_epsilon"], dtype=code)
        self._create("sdn_t5_create", c)
        # rows of one launch: the GEMM tiles address an operand with 31-bit byte offsets
        widest = max(cfg["d_ff"], 3 * cfg["num_heads"] * cfg["d_kv"], 2 * cfg["d_model"])
        self.max_rows = ((1 << 31) - 4096) // (2 * widest)

    @staticmethod
    def _is_norm_param(name: str) -> bool:
        return "layer_norm" in name

    @staticmethod
    def _canonical(sd: dict) -> dict:
        out = {(k[len("encoder."):] if k.startswith("encoder.") else k): v for k, v in sd.items()}
        if "embed_tokens.weight" not in out and "shared.weight" in out:
            out["embed_tokens.weight"] = out["shared.weight"]
        return out

    def _glu_view(self, buf: torch.Tensor, p: dict) -> torch.Tensor:
        """The [F / 16, 16, cols] rows of `buf` that one half (value or gate) of an interleaved gated weight occupies."""
        f, k, es = p["rows"], p["cols"], torch.empty((), dtype=self.dtype).element_size()
        base = p["offset"] - (16 * k * es if p["kind"] == P_GLU_GATE else 0)
        pair = buf[base:base + 2 * f * k * es].view(self.dtype).view(f // 16, 2, 16, k)
        return pair[:, 1 if p["kind"] == P_GLU_GATE else 0]

    def _store(self, buf: torch.Tensor, p: dict, t: torch.Tensor):
        if p["kind"] in (P_GLU_VALUE, P_GLU_GATE):
            self._glu_view(buf, p).copy_(t.view(p["rows"] // 16, 16, p["cols"]))
        else:
            super()._store(buf, p, t)

    def flops(self, batch: int, n: int = 256):
        a = C.c_double()
        total = _lib.lib().sdn_t5_flops(self._h, batch, n, C.byref(a))
        return total, a.value

    def _workspace(self, batch: int, n: int, device):
        ws = self._ws.get((batch, n))
        if ws is None:
            nbytes = _lib.lib().sdn_t5_workspace_bytes(self._h, batch, n)
            if len(self._ws) >= 8:
                self._ws.clear()
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._ws[(batch, n)] = ws
        return ws

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor | None = None, **unused):
        if input_ids.dim() != 2:
            raise _lib.SdnError(f"input_ids must be [B, n], got {tuple(input_ids.shape)}")
        b, n = input_ids.shape
        if not MIN_LEN <= n <= MAX_LEN:
            raise _lib.SdnError(f"sequence length {n} is outside [{MIN_LEN}, {MAX_LEN}]")
        if attention_mask is not None and tuple(attention_mask.shape) != (b, n):
            raise _lib.SdnError("attention_mask must have the shape of input_ids")
        if not input_ids.is_cuda and b > 0:               # (ids already on the device are clamped by the kernel: no read-back)
            lo, hi = int(input_ids.min()), int(input_ids.max())
            if lo < 0 or hi >= self.config.vocab_size:
                raise _lib.SdnError(f"input_ids outside the vocabulary [0, {self.config.vocab_size}): min {lo}, max {hi}")
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        dev = self._weights.device
        ids = input_ids.to(device=dev, dtype=torch.int32).contiguous()
        mask = None if attention_mask is None else attention_mask.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty((b, n, self.config.d_model), dtype=self.dtype, device=dev)
        step = max(1, self.max_rows // n)
        for lo in range(0, b, step):
            nb = min(step, b - lo)
            ws = self._workspace(nb, n, dev)
            _lib.check(_lib.lib().sdn_t5_forward(self._h, _lib.dptr(self._weights), _lib.dptr(ids[lo:lo + nb], torch.int32),
                                                 None if mask is None else _lib.dptr(mask[lo:lo + nb], torch.int32), n,
                                                 _lib.dptr(out[lo:lo + nb], self.dtype), nb, _lib.dptr(ws), ws.numel(),
                                                 _lib.stream_ptr()), "sdn_t5_forward")
        return T5EncoderOutput(out)
