"""SD3Transformer2DModel (MMDiT) front-end: the call surface the reference's SD-v3 pipelines use
(`self.transformer(hidden_states=, timestep=, encoder_hidden_states=, pooled_projections=, return_dict=False)[0]`,
models/sdv3/safe_denoiser_pipeline.py:1120-1127), executed by libsdn's static launch plan (sdn_mmdit_forward).
Weights are addressed by their diffusers state_dict keys and packed once into the engine layout by EngineModel's packer (_model.py).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import _lib
from ._model import ALL_DTYPES, P_POS_CROP, EngineModel  # noqa: F401

SD3_MEDIUM = dict(in_channels=16, out_channels=16, sample_size=64, patch_size=2, num_layers=24, num_attention_heads=24,
                  attention_head_dim=64, joint_attention_dim=4096, pooled_projection_dim=2048, pos_embed_max_size=192)
# SD-3.5-medium (diffusers >= 0.31): per-head RMS norm of q and k in every attention, a second image-only attention in blocks 0 ... 12
SD35_MEDIUM = dict(SD3_MEDIUM, pos_embed_max_size=384, qk_norm="rms_norm", dual_attention_layers=tuple(range(13)))
# SD-3.5-large: 38 blocks, 38 heads of 64 (2432 wide), q/k RMS norm, no dual-attention blocks
SD35_LARGE = dict(SD3_MEDIUM, num_layers=38, num_attention_heads=38, qk_norm="rms_norm")
# widest block the plan runs (sdn_mmdit_create_ex; above 2048 a multiple of 128: the NQ = 5 LayerNorm forms)
MAX_WIDTH = 2560
QK_NORM_GAINS = (".norm_q.weight", ".norm_k.weight", ".norm_added_q.weight", ".norm_added_k.weight")


class SD3Transformer2DModel(EngineModel):
    """`sample_size` is the LATENT side this plan is built for (64 -> 512x512 images, the reference driver's default,
    run_nudity_sdv3.py:357-358,500; 128 -> 1024x1024).
    dtype=torch.float32 selects the fp32 precision plan (sdn_mmdit_config.dtype 2): weights, text, pooled projections and
    activations stay f32 and the contractions run on the f32-input matrix cores.  precision = "bf16x3" (with dtype=torch.float32,
    or alone) keeps the f32 storage and forms every contraction as three bf16 products (dtype 3, sdn_gemm_x3); "fp32" = dtype 2.
    Same meaning as UNet2DConditionModel's arguments.
    qk_norm = "rms_norm" and dual_attention_layers = (i, ...) are the SD-3.5 additions (sdn_mmdit_ext, include/sdn.h); with neither
    the handle is sdn_mmdit_create's."""

    def __init__(self, text_len: int = 333, dtype=torch.float16, precision: str | None = None, qk_norm: str | None = None,
                 dual_attention_layers=(), **config):
        code = self._storage(dtype, precision, ALL_DTYPES,
                             "storage dtype must be torch.bfloat16, torch.float16 or torch.float32 (the precision mode)")
        cfg = dict(SD3_MEDIUM)
        cfg.update(config)
        if qk_norm not in (None, "rms_norm"):
            raise NotImplementedError(f'qk_norm = {qk_norm!r} is not implemented by the engine\'s plan (needs None or "rms_norm")')
        dual = tuple(sorted(set(int(i) for i in (dual_attention_layers or ()))))
        if dual and not (0 <= dual[0] and dual[-1] < min(cfg["num_layers"], 64)):
            raise _lib.SdnError(f"dual_attention_layers {dual} must name blocks below num_layers = {cfg['num_layers']} (and below 64)")
        cfg.update(qk_norm=qk_norm, dual_attention_layers=dual)
        self.config = SimpleNamespace(**cfg)
        self.in_channels = cfg["in_channels"]
        self.text_len = text_len
        c = _lib.MmditConfig(in_channels=cfg["in_channels"], out_channels=cfg["out_channels"],
                             sample_size=cfg["sample_size"], patch_size=cfg["patch_size"], num_layers=cfg["num_layers"],
                             num_heads=cfg["num_attention_heads"], head_dim=cfg["attention_head_dim"],
                             joint_dim=cfg["joint_attention_dim"], pooled_dim=cfg["pooled_projection_dim"],
                             text_len=text_len, time_dim=256, dtype=code)
        if qk_norm or dual:
            ext = _lib.MmditExt(qk_norm=1 if qk_norm else 0, qk_norm_eps=1e-6, dual_attention_mask=sum(1 << i for i in dual))
            self._create("sdn_mmdit_create_ex", c, ext)
        else:
            self._create("sdn_mmdit_create", c)

    # ---- parameters -------------------------------------------------------------------------------------
    def _source_shape(self, p: dict) -> tuple:
        cfg = self.config
        if p["kind"] == P_POS_CROP:
            return (1, cfg.pos_embed_max_size ** 2, p["cols"])
        if p["name"] == "pos_embed.proj.weight":
            return (p["rows"], cfg.in_channels, cfg.patch_size, cfg.patch_size)
        return super()._source_shape(p)

    @staticmethod
    def _is_norm_param(name: str) -> bool:
        return ".norm" in name                    # (the blocks' adaLN biases: their amplitude in load_synthetic_on_device)

    def synthetic_state_dict(self, seed: int = 1234) -> dict:
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for name, shape in self.state_dict_shapes().items():
            if name == "pos_embed.pos_embed":
                sd[name] = 0.5 * torch.randn(shape, generator=g)
            elif name.endswith(QK_NORM_GAINS):
                # U(1, 3): the 1-D rule below would make gains of about 0 (attention that ignores q and k), and with gains near 1
                # dropping the norms moves a small network's output less than the bf16 bound -- a test would not see it
                sd[name] = 1.0 + 2.0 * torch.rand(shape, generator=g)
            elif len(shape) == 1:
                sd[name] = 0.2 * (torch.rand(shape, generator=g) - 0.5)
            else:
                fan_in = 1
                for d in shape[1:]:
                    fan_in *= d
                scale = 0.3 if ("norm1" in name or "norm_out" in name) else 1.0      # keep adaLN modulation moderate
                sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * (3.0 / fan_in) ** 0.5 * scale
        return sd

    def crop_pos_embed(self, pe: torch.Tensor) -> torch.Tensor:
        """PatchEmbed.cropped_pos_embed: centre crop of the [max,max] grid to this plan's token grid."""
        cfg = self.config
        m, hp = cfg.pos_embed_max_size, cfg.sample_size // cfg.patch_size
        top = (m - hp) // 2
        grid = pe.reshape(m, m, -1)
        return grid[top:top + hp, top:top + hp].reshape(hp * hp, -1)

    def _pack_one(self, p: dict, t: torch.Tensor) -> torch.Tensor:
        return super()._pack_one(p, self.crop_pos_embed(t) if p["kind"] == P_POS_CROP else t)

    # ---- forward ------------------------------------------------------------------------------------------
    def prepare_text(self, encoder_hidden_states: torch.Tensor) -> torch.Tensor:
        e = encoder_hidden_states
        if e.shape[1] != self.text_len or e.shape[2] != self.config.joint_attention_dim:
            raise _lib.SdnError(f"encoder_hidden_states must be [B,{self.text_len},{self.config.joint_attention_dim}]")
        return e.to(self.dtype).contiguous()

    def max_samples(self) -> int:
        """Largest batch ONE launch plan addresses (31-bit LDS-DMA offsets per operand): the widest 16-bit operand is the feed-forward
        hidden state, tokens x 4 x width x 2 B per sample -- 170 samples at 512^2, 42 at 1024^2 for SD3-medium (1536 wide); 107 and 26 for
        SD-3.5-large (2432 wide; 53 and 13 in the fp32-storage plans).  `forward_into` runs
        larger batches as consecutive row blocks (samples do not interact; one handle: this plan keeps no per-text cache).
        fp32-storage plans (precision "fp32" / "bf16x3"): the same rule at 4 B per element -- 85 samples at 512^2, 21 at 1024^2.  Their
        kernels (sdn_gemm_f32 / sdn_gemm_x3, the f32 attention, LayerNorm, patchify and unpatchify) address every operand with 64-bit
        element offsets, so the cap keeps each operand under 2 GiB as a margin, not because a kernel would wrap."""
        c = self.config
        tokens = (c.sample_size // c.patch_size) ** 2
        esz = 4 if self.precision in ("fp32", "bf16x3") else 2
        return ((1 << 31) - 1) // (tokens * 4 * c.num_attention_heads * c.attention_head_dim * esz)

    def forward_into(self, sample, timestep, text16, pooled16, out):
        b = sample.shape[0]
        cap = self.max_samples()
        if b > cap:
            if text16.shape[0] != b or pooled16.shape[0] != b or out.shape[0] != b:
                raise _lib.SdnError("batch mismatch between sample, text, pooled projections and out")
            per = max(cap // 2 * 2, 1)                          # (even: a classifier-free-guidance pair's halves stay whole blocks apart)
            for lo in range(0, b, per):
                hi = min(b, lo + per)
                self.forward_into(sample[lo:hi], timestep, text16[lo:hi], pooled16[lo:hi], out[lo:hi])
            return out
        ws = self._workspace(b, sample.device)
        _lib.check(_lib.lib().sdn_mmdit_forward(self._h, _lib.dptr(self._weights), _lib.dptr(sample, torch.float32),
                                                float(timestep), _lib.dptr(text16, self.dtype),
                                                _lib.dptr(pooled16, self.dtype), _lib.dptr(out, torch.float32), b,
                                                _lib.dptr(ws), ws.numel(), _lib.stream_ptr()), "sdn_mmdit_forward")
        return out

    def __call__(self, hidden_states, timestep=None, encoder_hidden_states=None, pooled_projections=None,
                 joint_attention_kwargs=None, return_dict=False, **unused):
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        in_dtype = hidden_states.dtype
        x = hidden_states.float().contiguous()
        s = self.config.sample_size
        if tuple(x.shape[1:]) != (self.config.in_channels, s, s):
            raise _lib.SdnError(f"hidden_states must be [B,{self.config.in_channels},{s},{s}], got {tuple(x.shape)}")
        t = timestep
        if torch.is_tensor(t):
            t = float(t.reshape(-1)[0])                         # the reference broadcasts one t to the batch (:1114)
        e = self.prepare_text(encoder_hidden_states)
        pl = pooled_projections.to(self.dtype).contiguous()
        out = torch.empty((x.shape[0], self.config.out_channels, s, s), dtype=torch.float32, device=x.device)
        self.forward_into(x, t, e, pl, out)
        out = out.to(in_dtype)
        return (out,) if not return_dict else SimpleNamespace(sample=out)
