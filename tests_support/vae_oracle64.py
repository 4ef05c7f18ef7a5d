"""Float64 reference of the AutoencoderKL decoder / encoder: oracle/vae.py's arithmetic on double tensors.

The oracle's blocks (`resnet`, `attention`) are dtype-agnostic once `act_dtype` is None: they only call torch.nn.functional on
whatever they are given.  Its constructor and its two entry functions are not (`v.float()`, `z.float()`, `x.float()`), so this
module keeps the weights in double and restates those two functions, line for line, without the casts; above Q_BLOCK attention
tokens the attention is restated too, with the softmax taken over blocks of query rows.  tests/test_vae_precise_host.py pins the
restatement against the oracle itself (fp32 evaluation vs this one: rel L2 <= 1e-5, blocked = unblocked)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.vae import SD14_VAE, OracleVAEEncoder


class OracleVAE64(OracleVAEEncoder):
    """decode(z, latent_scale) and encode(x) in float64; inputs of any float type, outputs double."""

    def __init__(self, state_dict: dict, config: dict | None = None):
        self.cfg = dict(SD14_VAE)
        if config:
            self.cfg.update(config)
        self.q_dtype = None
        self.sd = {k: v.detach().double() for k, v in state_dict.items()}

    Q_BLOCK = 4096       # queries per softmax block: rows are independent, so the block size changes memory (a 16384-token score
                         # matrix is 2 GiB in double), not the result

    def attention(self, pfx, x):
        b, c, hh, ww = x.shape
        if hh * ww <= self.Q_BLOCK:
            return super().attention(pfx, x)
        h = F.group_norm(x, self.cfg["norm_groups"], self.P(pfx + ".group_norm.weight"), self.P(pfx + ".group_norm.bias"), eps=1e-6)
        t = h.reshape(b, c, hh * ww).transpose(1, 2)
        qq, kk, vv = (F.linear(t, self.P(f"{pfx}.{n}.weight"), self.P(f"{pfx}.{n}.bias")) for n in ("to_q", "to_k", "to_v"))
        a = torch.cat([torch.softmax(qq[:, r0:r0 + self.Q_BLOCK] @ kk.transpose(1, 2) * (c ** -0.5), dim=-1) @ vv
                       for r0 in range(0, hh * ww, self.Q_BLOCK)], dim=1)
        o = F.linear(a, self.P(pfx + ".to_out.0.weight"), self.P(pfx + ".to_out.0.bias"))
        return o.transpose(1, 2).reshape(b, c, hh, ww) + x

    def decode(self, z: torch.Tensor, latent_scale: float = 1.0) -> torch.Tensor:
        c = self.cfg
        x = F.conv2d(z.double() * latent_scale, self.P("post_quant_conv.weight"), self.P("post_quant_conv.bias"))
        x = F.conv2d(x, self.P("decoder.conv_in.weight"), self.P("decoder.conv_in.bias"), padding=1)
        x = self.resnet("decoder.mid_block.resnets.0", x)
        x = self.attention("decoder.mid_block.attentions.0", x)
        x = self.resnet("decoder.mid_block.resnets.1", x)
        n = len(c["block_out_channels"])
        for i in range(n):
            for j in range(c["layers_per_block"] + 1):
                x = self.resnet(f"decoder.up_blocks.{i}.resnets.{j}", x)
            if i + 1 < n:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
                x = F.conv2d(x, self.P(f"decoder.up_blocks.{i}.upsamplers.0.conv.weight"),
                             self.P(f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"), padding=1)
        x = F.silu(F.group_norm(x, c["norm_groups"], self.P("decoder.conv_norm_out.weight"), self.P("decoder.conv_norm_out.bias"),
                                eps=1e-6))
        return F.conv2d(x, self.P("decoder.conv_out.weight"), self.P("decoder.conv_out.bias"), padding=1)

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        c = self.cfg
        h = F.conv2d(x.double(), self.P("encoder.conv_in.weight"), self.P("encoder.conv_in.bias"), padding=1)
        n = len(c["block_out_channels"])
        for i in range(n):
            for j in range(c["layers_per_block"]):
                h = self.resnet(f"encoder.down_blocks.{i}.resnets.{j}", h)
            if i + 1 < n:
                h = F.pad(h, (0, 1, 0, 1))
                h = F.conv2d(h, self.P(f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"),
                             self.P(f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"), stride=2)
        h = self.resnet("encoder.mid_block.resnets.0", h)
        h = self.attention("encoder.mid_block.attentions.0", h)
        h = self.resnet("encoder.mid_block.resnets.1", h)
        h = F.silu(F.group_norm(h, c["norm_groups"], self.P("encoder.conv_norm_out.weight"), self.P("encoder.conv_norm_out.bias"),
                                eps=1e-6))
        m = F.conv2d(h, self.P("encoder.conv_out.weight"), self.P("encoder.conv_out.bias"), padding=1)
        return F.conv2d(m, self.P("quant_conv.weight"), self.P("quant_conv.bias"))

    def image_uint8(self, latents: torch.Tensor, shift: float = 0.0) -> torch.Tensor:
        """decode_latents + numpy_to_pil in double: round_half_even(255 * clamp(x / 2 + 0.5, 0, 1)), NHWC uint8."""
        x = self.decode(latents.double() / self.cfg["scaling_factor"] + shift)
        return (255.0 * (x / 2 + 0.5).clamp(0, 1)).round().permute(0, 2, 3, 1).to(torch.uint8)


def rel_l2(a: torch.Tensor, ref64: torch.Tensor) -> float:
    a, ref64 = a.detach().double().cpu(), ref64.double().cpu()
    return float((a - ref64).norm() / ref64.norm())
