"""EngineModel: an engine handle with packed weights, the base of every model front-end (unet, mmdit, vae, clip, t5, clip_vision).

A front-end resolves its storage mode (`_storage`), creates its handle (`_create`) and reads the manifest the C side publishes
(sdn_unet_param_info serves every handle kind): per state_dict tensor its name, kind, rows, cols and byte offset in the ONE weight
buffer.  A state_dict is packed by one path, `_pack`: canonical keys -> missing-keys check -> per manifest entry `_pack_one`
(vectors f32, matrices [rows, cols] in the storage type, 3x3 conv kernels [O,I,3,3] -> [O][ky][kx][I]) -> `_store` at the entry's
offset.  pack_state_dict is that into a host buffer, load_state_dict the same into a device buffer (tensor by tensor, each converted
where it lives: the engine-derived regions between the tensors never exist on the host) followed by `_prepare`.  What a model overrides:

  _canonical(sd)         key prefixes and aliases (`text_model.`, `shared.weight`, the VAE's deprecated attention names)
  _pack_one(p, t)        its own tensor layouts (GEGLU interleave, position-embedding crop, patch-weight pad)
  _store(buf, p, t)      where an entry's rows go when not at p["offset"] in one piece (T5's interleaved GLU halves)
  _source_shape(p)       the state_dict shape of an entry where it is not (rows,) / (rows, cols) / (rows, cols / 9, 3, 3)
  _is_norm_param(name)   which vectors are norm gains / biases (synthetic weights)
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

P_VEC_F32, P_MAT, P_CONV3X3, P_GEGLU_MAT, P_GEGLU_VEC, P_POS_CROP = 0, 1, 2, 3, 4, 5
P_DERIVED = 6      # regions the engine fills itself (sdn_unet_prepare): not state_dict tensors
P_GLU_VALUE, P_GLU_GATE = 7, 8

ALL_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
HALF_DTYPES = (torch.bfloat16, torch.float16)
DTYPE_CODES = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


class EngineModel:
    # ---- storage mode and handle ---------------------------------------------------------------------------
    def _storage(self, dtype, precision, allowed, refusal: str) -> int:
        """Sets self.dtype / self.precision and returns the C side's dtype code (sdn_*_config.dtype): 0 bf16, 1 fp16, 2 = fp32 storage
        on the f32-input matrix cores, 3 = fp32 storage with bf16x3 split-operand contractions."""
        if precision not in (None, "fp32", "bf16x3"):
            raise _lib.SdnError('precision must be None, "fp32" or "bf16x3"')
        if precision is not None:
            dtype = torch.float32                                   # both precision modes store f32
        if dtype not in allowed:
            raise _lib.SdnError(refusal)
        self.dtype = dtype
        self.precision = precision or ("fp32" if dtype == torch.float32 else None)
        return 3 if self.precision == "bf16x3" else DTYPE_CODES[dtype]

    def _create(self, create_fn: str, cstruct, *more):
        """`more`: further structs the creator takes between its config and the handle (sdn_mmdit_create_ex's sdn_mmdit_ext)."""
        h = C.c_void_p()
        _lib.check(getattr(_lib.lib(), create_fn)(C.byref(cstruct), *[C.byref(s) for s in more], C.byref(h)), create_fn)
        self._h = h
        self._weights = None
        self._ws = {}
        self._read_manifest()

    def _read_manifest(self):
        """state_dict-keyed tensors -> self.manifest; engine-derived regions (SDN_P_DERIVED) are left to _prepare()."""
        h = self._h
        self.manifest = []
        info = _lib.ParamInfo()
        for i in range(_lib.lib().sdn_unet_param_count(h)):
            _lib.check(_lib.lib().sdn_unet_param_info(h, i, C.byref(info)), "sdn_unet_param_info")
            if info.kind == P_DERIVED:
                continue
            self.manifest.append(dict(name=info.name.decode(), kind=info.kind, rows=info.rows, cols=info.cols,
                                      rows_padded=info.rows_padded, offset=info.offset))
        self.weight_bytes = _lib.lib().sdn_unet_weight_bytes(h)

    def _prepare(self):
        """Let the engine fill its derived weight regions (LayerNorm-folded projections) from the uploaded tensors."""
        _lib.check(_lib.lib().sdn_unet_prepare(self._h, _lib.dptr(self._weights), _lib.stream_ptr()), "sdn_unet_prepare")
        return self

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().sdn_unet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- packing ---------------------------------------------------------------------------------------------
    @staticmethod
    def _canonical(sd: dict) -> dict:
        return sd

    def _pack_one(self, p: dict, t: torch.Tensor) -> torch.Tensor:
        """One state_dict tensor in the engine layout, converted where it lives (device-resident state dicts stay on the device)."""
        t = t.detach()
        if p["cols"] == 0:
            return t.to(torch.float32).reshape(-1)
        if p["kind"] == P_CONV3X3:
            t = t.permute(0, 2, 3, 1)
        return t.to(self.dtype).reshape(p["rows"], p["cols"])

    def _store(self, buf: torch.Tensor, p: dict, t: torch.Tensor):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        buf[p["offset"]:p["offset"] + raw.numel()].copy_(raw)

    def _pack(self, sd: dict, device) -> torch.Tensor:
        sd = self._canonical(sd)
        missing = [p["name"] for p in self.manifest if p["name"] not in sd]
        if missing:
            raise KeyError(f"state_dict lacks {len(missing)} keys, e.g. {missing[:3]}")
        buf = torch.zeros(self.weight_bytes, dtype=torch.uint8, device=device)
        for p in self.manifest:
            self._store(buf, p, self._pack_one(p, sd[p["name"]]))
        return buf

    def pack_state_dict(self, sd: dict) -> torch.Tensor:
        """CPU uint8 buffer in the engine layout."""
        return self._pack(sd, "cpu")

    def load_state_dict(self, sd: dict, device="cuda"):
        _lib.require_gpu()
        self._weights = self._pack(sd, device)
        return self._prepare()

    # ---- synthetic weights -----------------------------------------------------------------------------------
    def _source_shape(self, p: dict) -> tuple:
        if p["cols"] == 0:
            return (p["rows"],)
        return (p["rows"], p["cols"] // 9, 3, 3) if p["kind"] == P_CONV3X3 else (p["rows"], p["cols"])

    def state_dict_shapes(self) -> dict:
        """state_dict key -> source tensor shape."""
        return {p["name"]: self._source_shape(p) for p in self.manifest}

    @staticmethod
    def _is_norm_param(name: str) -> bool:
        return "norm" in name.split(".")[-2]

    def synthetic_state_dict(self, seed: int = 1234) -> dict:
        """Random weights of this architecture (there are no checkpoints on the box): variance-preserving
        uniform U(-sqrt(3/fan_in), sqrt(3/fan_in)) for matrices, small uniform biases, norm gains near 1."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for name, shape in self.state_dict_shapes().items():
            if len(shape) == 1:
                if self._is_norm_param(name):
                    base = 1.0 if name.endswith("weight") else 0.0
                    sd[name] = base + 0.1 * (torch.rand(shape, generator=g) - 0.5)
                else:
                    sd[name] = 0.2 * (torch.rand(shape, generator=g) - 0.5)
            else:
                fan_in = 1
                for d in shape[1:]:
                    fan_in *= d
                bound = (3.0 / fan_in) ** 0.5
                sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        return sd

    def load_synthetic_on_device(self, seed: int = 1234, device="cuda"):
        """Random weights generated DIRECTLY in the packed engine layout on the GPU (benchmarks: no checkpoints exist
        on the box and the 0.86 G-parameter CPU generate+pack path takes tens of seconds per rank).  Same distributions
        as synthetic_state_dict(); the values are not the CPU generator's, so parity tests use the state_dict path."""
        _lib.require_gpu()
        g = torch.Generator(device=device).manual_seed(seed)
        buf = torch.zeros(self.weight_bytes, dtype=torch.uint8, device=device)
        for p in self.manifest:
            n = p["rows"] * max(p["cols"], 1)
            if p["cols"] == 0:
                is_gain = self._is_norm_param(p["name"]) and p["name"].endswith("weight")
                is_nb = self._is_norm_param(p["name"]) and p["name"].endswith("bias")
                amp = 0.1 if (is_gain or is_nb) else 0.2
                t = (torch.rand(n, generator=g, device=device) - 0.5) * amp + (1.0 if is_gain else 0.0)
            else:
                t = ((torch.rand(n, generator=g, device=device) * 2 - 1) * (3.0 / p["cols"]) ** 0.5).to(self.dtype).view(p["rows"], p["cols"])
            self._store(buf, p, t)
        self._weights = buf
        return self._prepare()

    # ---- queries and profiling ---------------------------------------------------------------------------------
    def flops(self, batch: int):
        a = C.c_double()
        total = _lib.lib().sdn_unet_flops(self._h, batch, C.byref(a))
        return total, a.value

    def _workspace(self, batch: int, device):
        ws = self._ws.get(batch)
        if ws is None:
            n = _lib.lib().sdn_unet_workspace_bytes(self._h, batch)
            ws = torch.empty(n, dtype=torch.uint8, device=device)
            self._ws[batch] = ws
        return ws

    def profile_next(self):
        """Arm HIP-event profiling of the next forward (diagnostics; see sdn_unet_profile_next)."""
        _lib.lib().sdn_unet_profile_next(self._h)

    def profile_read(self) -> list:
        rows = (_lib.ProfileRow * 32)()
        n = _lib.lib().sdn_unet_profile_read(self._h, rows, 32)
        if n < 0:
            raise _lib.SdnError("sdn_unet_profile_read failed (no profiled forward?)")
        return [dict(kernel=rows[i].kernel.decode(), launches=rows[i].launches, ms=rows[i].ms, flops=rows[i].flops,
                     bytes=rows[i].bytes) for i in range(n)]
