"""UNet2DConditionModel front-end: the call surface the reference's pipelines use
(`self.unet(latent_model_input, t, encoder_hidden_states=E).sample`, ...threshold_time.py:538,540;
`self.unet.config.sample_size`, `self.unet.in_channels`), executed by libsdn's static launch plan.

Weights: a diffusers-keyed state_dict (the names of `UNet2DConditionModel.state_dict()` for SD-v1.4) is packed
ONCE into a single device buffer in the engine's layouts, driven by the manifest the C side publishes
(sdn_unet_param_info): conv kernels [O,I,3,3] -> [O][ky][kx][I] bf16, linears / 1x1 convs -> [O][I] bf16,
GEGLU projection rows interleaved value/gate in blocks of 16, norms and biases f32.
The handle, the manifest and the packer are EngineModel's (_model.py), shared with every other front-end; this file adds the
GEGLU layout and what only a UNet has: latent_repeat, the text K / V cache, tail split and chunking, graph mode, split-K.
dtype=torch.float32 selects the plan's PRECISION mode (sdn_unet_config.dtype 2): weights, text and activations stay f32 and
the contractions run on the f32-input matrix cores -- 1/16 of the 16-bit rate, ~1e-6 per forward from the fp32 reference.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import torch

from . import _lib
from ._model import ALL_DTYPES, P_CONV3X3, P_DERIVED, P_GEGLU_MAT, P_GEGLU_VEC, P_MAT, P_VEC_F32, EngineModel  # noqa: F401

SD14_CONFIG = dict(in_channels=4, out_channels=4, sample_size=64, block_out_channels=(320, 640, 1280, 1280),
                   down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D",
                                     "DownBlock2D"),
                   layers_per_block=2, attention_head_dim=8, cross_attention_dim=768, norm_num_groups=32)

class UNetOutput:
    __slots__ = ("sample",)

    def __init__(self, sample):
        self.sample = sample


def _interleave16(t: torch.Tensor) -> torch.Tensor:
    """[2F, ...] (value rows then gate rows) -> blocks of 16 value rows followed by their 16 gate rows."""
    f = t.shape[0] // 2
    v, g = t[:f], t[f:]
    rest = t.shape[1:]
    return torch.stack([v.reshape(f // 16, 16, *rest), g.reshape(f // 16, 16, *rest)], dim=1).reshape(2 * f, *rest)


class UNet2DConditionModel(EngineModel):
    def __init__(self, text_len: int = 77, dtype=torch.bfloat16, latent_repeat: int = 1, precision: str | None = None, **config):
        """precision = "bf16x3" (with dtype=torch.float32, or alone): fp32 storage with split-operand contractions on the bf16
        matrix cores (sdn_unet_config.dtype 3, sdn_gemm_x3) -- the mode that meets the north star's 1e-3 at a multiple of the
        f32-MFMA plan's speed.
        latent_repeat = r > 1: the engine-side form of `torch.cat([latents] * r)` (classifier-free guidance): `sample`
        then holds B / r latents, `encoder_hidden_states` stays [B] branch-major, and everything up to the first
        cross-attention is computed once per latent (sdn_unet_config.latent_repeat).  Bit-identical results."""
        code = self._storage(dtype, precision, ALL_DTYPES,
                             "storage dtype must be torch.bfloat16, torch.float16 or torch.float32 (the precision mode)")
        self.latent_repeat = max(1, int(latent_repeat))
        cfg = dict(SD14_CONFIG)
        cfg.update(config)
        self.config = SimpleNamespace(**cfg)
        self.in_channels = cfg["in_channels"]
        self.text_len = text_len
        boc = list(cfg["block_out_channels"])
        n = len(boc)
        c = _lib.UnetConfig(in_channels=cfg["in_channels"], out_channels=cfg["out_channels"],
                            sample_size=cfg["sample_size"], n_levels=n,
                            block_out_channels=(C.c_int32 * 4)(*(boc + [0] * (4 - n))),
                            level_has_attn=(C.c_int32 * 4)(*([1 if "CrossAttn" in t else 0
                                                              for t in cfg["down_block_types"]] + [0] * (4 - n))),
                            layers_per_block=cfg["layers_per_block"], n_heads=cfg["attention_head_dim"],
                            cross_dim=cfg["cross_attention_dim"], text_len=text_len,
                            norm_groups=cfg["norm_num_groups"],
                            dtype=code, latent_repeat=self.latent_repeat)
        self.tail_split = False            # set_tail_split(): see _tail_split_of
        self.conv_up4 = True               # set_conv_up4(): mirrors the handle's switch (on by default)
        self._create("sdn_unet_create", c)

    # ---- parameters ---------------------------------------------------------------------------------
    def _source_shape(self, p: dict) -> tuple:
        if p["name"].endswith(("proj_in.weight", "proj_out.weight", "conv_shortcut.weight")):
            return (p["rows"], p["cols"], 1, 1)
        return super()._source_shape(p)

    @staticmethod
    def _is_norm_param(name: str) -> bool:
        return ".norm" in name or name.startswith("conv_norm_out")

    def _pack_one(self, p: dict, t: torch.Tensor) -> torch.Tensor:
        """GEGLU projections: value / gate rows interleaved in blocks of 16."""
        t = super()._pack_one(p, t)
        return _interleave16(t) if p["kind"] in (P_GEGLU_MAT, P_GEGLU_VEC) else t

    def sibling(self, latent_repeat: int | None = None):
        """A second handle over the SAME packed weights (its own launch plans, workspace and text K / V cache), with this one's
        latent_repeat or another.  The derived regions live in the weight buffer: nothing to prepare again."""
        net = UNet2DConditionModel(text_len=self.text_len, dtype=self.dtype, precision=self.precision,
                                   latent_repeat=self.latent_repeat if latent_repeat is None else latent_repeat, **vars(self.config))
        net._weights = self._weights
        if not self.conv_up4:
            net.set_conv_up4(False)
        return net

    # ---- forward --------------------------------------------------------------------------------------
    def set_graph_mode(self, on: bool = True):
        """Replay each forward as one hipGraph (sdn_unet_set_graph_mode): worth it when the batch is small enough for the
        ~850 launches of a forward to be the bound (a single prompt: 13 ms -> a few ms per step).  Identical results."""
        _lib.lib().sdn_unet_set_graph_mode(self._h, 1 if on else 0)
        return self

    def set_text_version(self, version: int = 0):
        """Declare the contents of the text operand of the next forwards (sdn_unet_set_text_version): while the version, the
        batch and the buffers stay the same, the cross-attention K / V projections of the text are not recomputed.  0 = undeclared."""
        _lib.lib().sdn_unet_set_text_version(self._h, int(version))
        self._text_version = int(version)
        return self

    def set_split_k(self, on: bool = True):
        """Small-batch option (sdn_unet_set_split_k): under-filled GEMMs run in split-K form.  Rebuilds the plans, so the
        cached workspaces are dropped.  Off by default (keeps outputs bit-identical across batch sizes)."""
        _lib.lib().sdn_unet_set_split_k(self._h, 1 if on else 0)
        self._ws = {}
        return self

    def set_conv_up4(self, on: bool = True):
        """Upsampler convs in phase form (sdn_unet_set_conv_up4; on by default): four 2x2 convs over the stored map with summed
        tap weights instead of nine taps over the upsampled one.  Off = the nine-tap op (A/B, tests).  Rebuilds the plans; the
        manifest and the packed weights do not change."""
        _lib.lib().sdn_unet_set_conv_up4(self._h, 1 if on else 0)
        self.conv_up4 = bool(on)
        self._ws = {}
        return self

    def prepare_text(self, encoder_hidden_states: torch.Tensor) -> torch.Tensor:
        e = encoder_hidden_states
        if e.shape[1] != self.text_len or e.shape[2] != self.config.cross_attention_dim:
            raise _lib.SdnError(f"encoder_hidden_states must be [B,{self.text_len},{self.config.cross_attention_dim}]")
        return e.to(self.dtype).contiguous()

    # ---- a few latents over whole waves of tiles: the tail runs beside the main forward ------------------------------------
    # Every level of the SD-v1.4 plan is a whole number of 256-CU waves of 256-row tiles when the batch is a multiple of 64
    # samples (64^2 level: 64 x 4096 / 256 = 1024 tiles = 4 waves; 16^2: 64 x 4 = 256 tiles = 1 wave).  A batch a few latents over
    # such a multiple (8 ranks x 515 prompts: 65 prompts x 3 branches = 195 samples on three of the ranks) starts one more wave in
    # every GEMM / conv launch for a handful of tiles: 162.6 ms against 152.7 ms for 192 samples, where the work grew 1.6 %
    # (tools/ab_tail_split.py).  With `tail_split` on, such a forward runs as the aligned part on the caller's stream and the
    # remaining latents as their own small forward (a second handle over the SAME packed weights) on a side stream, joined before
    # the outputs are put back in branch-major order: 156.8 ms, bit-identical outputs on the 16-bit plans (rows are independent;
    # bf16x3: 2e-6, its row chunks differ).  DESIGN 10.13.
    TAIL_MAX_SAMPLES = 12            # measured: 3 samples -3.6 %, 24 samples -1.4 % of the unsplit forward; above this it stays one batch

    def set_tail_split(self, on: bool = True):
        self.tail_split = bool(on)
        return self

    def _tail_split_of(self, b: int):
        """(latents in the aligned main forward, latents in the tail), or None when the batch runs as one forward."""
        rep = self.latent_repeat
        if not self.tail_split or rep <= 1:
            return None
        p = b // rep
        q = 64 // math.gcd(64, rep)                                  # latents per 64-sample quantum
        pm = p // q * q
        r = p - pm
        if pm == 0 or r == 0 or r * rep > self.TAIL_MAX_SAMPLES:
            return None
        return pm, r

    def max_samples(self) -> int:
        """Largest batch ONE launch plan addresses: the LDS-DMA tiles carry 31-bit byte offsets per operand, and the widest 16-bit
        operand of a forward is an up-path resnet's input (skip connection concatenated: 64^2 x 960 channels = 7.9 MB per sample
        for SD-v1.4 -> 273 samples).  Larger batches run as several forwards (`_chunks_of`)."""
        c = self.config
        boc = list(c.block_out_channels)
        n = len(boc)
        worst = max((c.sample_size >> i) ** 2 * (boc[min(i + 1, n - 1)] + boc[i]) * 2 for i in range(n))
        cap = ((1 << 31) - 1) // worst
        if self.precision in ("fp32", "bf16x3"):
            # fp32-storage plans: their GEMMs cut launches themselves (6-byte triples), the other kernels index 4-byte tensors of twice
            # the size; exercised up to 195 samples at full size (tests, tools/ab_tail_split.py) -- stay where that evidence is
            cap = min(cap, 3 * (cap // 4))
        return cap

    def _chunks_of(self, b: int):
        """How a forward of b samples runs: None = one launch plan; else [(first latent, latents, on the side stream)].  Two reasons to
        cut: the tail rule above, and a batch above `max_samples()` (it used to fail with SDN_E_INVALID): whole-wave chunks (multiples of
        64 samples) one after the other on the caller's stream, each on its own handle (its own workspace and text K / V cache), a
        small remainder beside them."""
        rep = self.latent_repeat
        p = b // rep
        cap = self.max_samples() // rep                                # latents one plan takes
        if p <= cap:
            ts = self._tail_split_of(b)
            return None if ts is None else [(0, ts[0], False), (ts[0], ts[1], True)]
        q = 64 // math.gcd(64, rep)
        per = cap // q * q if cap >= q else cap                        # whole waves of tiles where the cap allows it
        chunks = [(lo, min(per, p - lo), False) for lo in range(0, p, per)]
        lo, n, _ = chunks[-1]
        if n * rep <= self.TAIL_MAX_SAMPLES and self.tail_split and rep > 1:
            chunks[-1] = (lo, n, True)
        return chunks

    def _forward_chunks(self, sample, timestep, text, out, chunks):
        rep, dev = self.latent_repeat, sample.device
        p = sample.shape[0]
        st = getattr(self, "_split", None)
        if st is None or st["key"] != (p, tuple(chunks), dev):
            tshape, oshape = tuple(text.shape[1:]), tuple(out.shape[1:])
            parts = [dict(lo=lo, n=n, side=side, net=self if i == 0 else self.sibling(),
                          # rep = 1: a chunk's text / output rows are contiguous views of the caller's tensors, nothing is staged
                          text=None if rep == 1 else torch.empty((rep * n,) + tshape, dtype=self.dtype, device=dev),
                          out=None if rep == 1 else torch.empty((rep * n,) + oshape, dtype=torch.float32, device=dev))
                     for i, (lo, n, side) in enumerate(chunks)]
            st = self._split = dict(key=(p, tuple(chunks), dev), parts=parts, text_key=None,
                                    side=torch.cuda.Stream(device=dev) if any(c[2] for c in chunks) else None)
        ver = int(getattr(self, "_text_version", 0))
        tkey = (ver, text.data_ptr())
        if rep > 1 and (ver == 0 or st["text_key"] != tkey):         # branch-major text rows [rep][p] -> [rep][n] per chunk
            tv = text.view(rep, p, *text.shape[1:])
            for c in st["parts"]:
                c["text"].view(rep, c["n"], *text.shape[1:]).copy_(tv[:, c["lo"]:c["lo"] + c["n"]])
            st["text_key"] = tkey
        cur = torch.cuda.current_stream(dev)
        if st["side"] is not None:
            st["side"].wait_stream(cur)                              # latents and text are ready where the caller's stream stands

        def run(c):
            net, lo, n = c["net"], c["lo"], c["n"]
            if net is not self:
                net._weights = self._weights                         # the derived regions live in the buffer: nothing to prepare again
                net.set_text_version(ver)
            if rep == 1:
                net._forward_one(sample[lo:lo + n], timestep, text[lo:lo + n], out[lo:lo + n])
            else:
                net._forward_one(sample[lo:lo + n], timestep, c["text"], c["out"])

        for c in st["parts"]:
            if c["side"]:
                with torch.cuda.stream(st["side"]):
                    run(c)
        for c in st["parts"]:
            if not c["side"]:
                run(c)
        if st["side"] is not None:
            cur.wait_stream(st["side"])
        if rep > 1:
            ov = out.view(rep, p, -1)
            for c in st["parts"]:
                ov[:, c["lo"]:c["lo"] + c["n"]].copy_(c["out"].view(rep, c["n"], -1))
        return out

    def forward_into(self, sample, timestep, text_bf16, out):
        """No-allocation form used by the engine loop (text already bf16, `out` preallocated fp32).  With latent_repeat = r
        the sample has B / r rows, text and out have B."""
        b = text_bf16.shape[0]
        if sample.shape[0] * self.latent_repeat != b or out.shape[0] != b:
            raise _lib.SdnError(f"batch mismatch: {sample.shape[0]} latents x latent_repeat {self.latent_repeat} vs {b} text rows")
        chunks = self._chunks_of(b)
        if chunks is not None:
            _lib.dptr(sample, torch.float32), _lib.dptr(text_bf16, self.dtype), _lib.dptr(out, torch.float32)     # the loud checks
            return self._forward_chunks(sample, timestep, text_bf16, out, chunks)
        return self._forward_one(sample, timestep, text_bf16, out)

    def _forward_one(self, sample, timestep, text_bf16, out):
        b = text_bf16.shape[0]
        if b > self.max_samples():
            raise _lib.SdnError(f"{b} samples exceed what one launch plan addresses ({self.max_samples()}): forward_into cuts such batches")
        ws = self._workspace(b, sample.device)
        _lib.check(_lib.lib().sdn_unet_forward(self._h, _lib.dptr(self._weights), _lib.dptr(sample, torch.float32),
                                               float(timestep), _lib.dptr(text_bf16, self.dtype),
                                               _lib.dptr(out, torch.float32), b, _lib.dptr(ws), ws.numel(),
                                               _lib.stream_ptr()), "sdn_unet_forward")
        return out

    def __call__(self, sample, timestep, encoder_hidden_states=None, return_dict=True, **unused):
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        x = sample.float().contiguous()
        s = self.config.sample_size
        if tuple(x.shape[1:]) != (self.config.in_channels, s, s):
            raise _lib.SdnError(f"sample must be [B,{self.config.in_channels},{s},{s}], got {tuple(x.shape)}")
        e = self.prepare_text(encoder_hidden_states)
        if e.shape[0] != x.shape[0] * self.latent_repeat:
            raise _lib.SdnError("batch mismatch between sample and encoder_hidden_states")
        out = torch.empty((e.shape[0], self.config.out_channels, s, s), dtype=torch.float32, device=x.device)
        self.forward_into(x, float(timestep), e, out)
        return UNetOutput(out) if return_dict else (out,)
