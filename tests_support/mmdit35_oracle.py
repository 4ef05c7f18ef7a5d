"""CPU oracle: the SD-3.5 MMDiT forward -- oracle.mmdit.OracleMMDiT with the two SD-3.5 additions, plain torch ops.

PARITY UNPINNED at the reference level, as for oracle/mmdit.py: diffusers >= 0.31 is not installed here and the reference holds no
tests for its transformer.  This restates the published diffusers definitions of the additions:
  qk_norm = "rms_norm": every Attention has norm_q / norm_k = RMSNorm(head_dim, eps = 1e-6) (and, with added_kv_proj_dim,
      norm_added_q / norm_added_k); JointAttnProcessor2_0 applies them per head after the projections and the split into heads,
      before the concatenation (image tokens first); v is untouched.
  dual_attention_layers: in those blocks norm1 is SD35AdaLayerNormZeroX (linear -> 9 C, chunk order shift_msa, scale_msa, gate_msa,
      shift_mlp, scale_mlp, gate_mlp, shift_msa2, scale_msa2, gate_msa2; both modulated inputs from the same LayerNorm(x)) and the
      block has attn2, self-attention over the image tokens alone (to_q / to_k / to_v / to_out.0 with biases, norm_q / norm_k):
      x = x + gate_msa attn.to_out(a_img);  x = x + gate_msa2 attn2.to_out.0(attn2(xn2));  then norm2 / feed-forward as before.
One structural fact pins the wiring: the SD-3.5-medium configuration yields 2,243,171,520 transformer parameters
(tests/test_mmdit35_host.py).

`act_dtype` emulates the engine's 16-bit storage points as the parent class does: one rounding after each tensor the engine writes,
the q / k thirds normalised in place included.  `skip_qk_norm` / `skip_attn2` build deliberately WRONG networks: the tests require
them to be far from the right one, so that a missing piece cannot pass.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle.mmdit import OracleMMDiT


class OracleMMDiT35(OracleMMDiT):
    def __init__(self, state_dict: dict, config: dict | None = None, act_dtype=None, device=None, *, qk_norm=None,
                 dual_attention_layers=(), skip_qk_norm: bool = False, skip_attn2: bool = False):
        super().__init__(state_dict, config, act_dtype, device)
        self.qk_norm = qk_norm == "rms_norm" and not skip_qk_norm
        self.dual = () if skip_attn2 else tuple(dual_attention_layers)
        self.dual9 = tuple(dual_attention_layers)          # blocks whose norm1.linear has 9 chunks, attn2 evaluated or not

    def rms(self, t, gain):
        """t [b, n, C] -> per head x * rsqrt(mean(x^2 over the 64) + 1e-6) * gain, rounded like the tensor the engine overwrites."""
        if not self.qk_norm:
            return t
        b, n, _ = t.shape
        h = t.reshape(b, n, self.cfg["num_heads"], self.cfg["head_dim"])
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-6) * self.P(gain)
        return self.q(h.reshape(b, n, -1))

    @torch.no_grad()
    def __call__(self, hidden_states, timestep: float, encoder_hidden_states, pooled_projections):
        c = self.cfg
        C_ = c["num_heads"] * c["head_dim"]
        b = hidden_states.shape[0]
        ps, m = c["patch_size"], c["pos_embed_max_size"]
        hp = c["sample_size"] // ps
        x = F.conv2d(self.q(hidden_states.float()), self.P("pos_embed.proj.weight"), self.P("pos_embed.proj.bias"), stride=ps)
        x = x.flatten(2).transpose(1, 2)
        top = (m - hp) // 2
        pos = self.P("pos_embed.pos_embed").reshape(m, m, -1)[top:top + hp, top:top + hp].reshape(1, hp * hp, -1)
        x = self.q(x + pos)
        half = c["time_dim"] // 2
        fr = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half).to(hidden_states.device)
        ang = torch.full((b, 1), float(timestep), device=hidden_states.device) * fr[None]
        tsin = self.q(torch.cat([torch.cos(ang), torch.sin(ang)], -1))
        te = self.q(F.silu(self.lin(tsin, "time_text_embed.timestep_embedder.linear_1")))
        te = self.lin(te, "time_text_embed.timestep_embedder.linear_2")
        pe = self.q(F.silu(self.lin(self.q(pooled_projections.float()), "time_text_embed.text_embedder.linear_1")))
        pe = self.lin(pe, "time_text_embed.text_embedder.linear_2")
        scond = self.q(F.silu(te + pe))
        ctx = self.q(self.lin(self.q(encoder_hidden_states.float()), "context_embedder"))
        L = c["num_layers"]
        sp = lambda t: t.reshape(b, -1, c["num_heads"], c["head_dim"]).transpose(1, 2)
        for i in range(L):
            pfx = f"transformer_blocks.{i}"
            last = i == L - 1
            mod = self.lin(scond, pfx + ".norm1.linear")
            if i in self.dual9:
                sh_a, sc_a, g_a, sh_m, sc_m, g_m, sh_a2, sc_a2, g_a2 = mod.chunk(9, dim=1)
            else:
                sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
            lnx = self.ln(x)
            xn = self.q(lnx * (1 + sc_a[:, None]) + sh_a[:, None])
            if last:
                c_sc, c_sh = self.lin(scond, pfx + ".norm1_context.linear").chunk(2, dim=1)
                cn = self.q(self.ln(ctx) * (1 + c_sc[:, None]) + c_sh[:, None])
            else:
                c_sh_a, c_sc_a, c_g_a, c_sh_m, c_sc_m, c_g_m = self.lin(scond, pfx + ".norm1_context.linear").chunk(6, dim=1)
                cn = self.q(self.ln(ctx) * (1 + c_sc_a[:, None]) + c_sh_a[:, None])
            qx, kx, vx = (self.q(self.lin(xn, f"{pfx}.attn.to_{n}")) for n in "qkv")
            qc, kc, vc = (self.q(self.lin(cn, f"{pfx}.attn.add_{n}_proj")) for n in "qkv")
            qx, kx = self.rms(qx, pfx + ".attn.norm_q.weight"), self.rms(kx, pfx + ".attn.norm_k.weight")
            qc, kc = self.rms(qc, pfx + ".attn.norm_added_q.weight"), self.rms(kc, pfx + ".attn.norm_added_k.weight")
            N = x.shape[1]
            a = F.scaled_dot_product_attention(sp(torch.cat([qx, qc], 1)), sp(torch.cat([kx, kc], 1)), sp(torch.cat([vx, vc], 1)))
            a = self.q(a.transpose(1, 2).reshape(b, -1, C_))
            ax, ac = a[:, :N], a[:, N:]
            x = self.q(x + g_a[:, None] * self.lin(ax, pfx + ".attn.to_out.0"))
            if i in self.dual:
                xn2 = self.q(lnx * (1 + sc_a2[:, None]) + sh_a2[:, None])
                q2, k2, v2 = (self.q(self.lin(xn2, f"{pfx}.attn2.to_{n}")) for n in "qkv")
                q2, k2 = self.rms(q2, pfx + ".attn2.norm_q.weight"), self.rms(k2, pfx + ".attn2.norm_k.weight")
                a2 = F.scaled_dot_product_attention(sp(q2), sp(k2), sp(v2))
                a2 = self.q(a2.transpose(1, 2).reshape(b, -1, C_))
                x = self.q(x + g_a2[:, None] * self.lin(a2, pfx + ".attn2.to_out.0"))
            xm = self.q(self.ln(x) * (1 + sc_m[:, None]) + sh_m[:, None])
            h = self.q(F.gelu(self.lin(xm, pfx + ".ff.net.0.proj"), approximate="tanh"))
            x = self.q(x + g_m[:, None] * self.lin(h, pfx + ".ff.net.2"))
            if not last:
                ctx = self.q(ctx + c_g_a[:, None] * self.lin(ac, pfx + ".attn.to_add_out"))
                cm = self.q(self.ln(ctx) * (1 + c_sc_m[:, None]) + c_sh_m[:, None])
                hc = self.q(F.gelu(self.lin(cm, pfx + ".ff_context.net.0.proj"), approximate="tanh"))
                ctx = self.q(ctx + c_g_m[:, None] * self.lin(hc, pfx + ".ff_context.net.2"))
        sc, sh = self.lin(scond, "norm_out.linear").chunk(2, dim=1)
        x = self.q(self.ln(x) * (1 + sc[:, None]) + sh[:, None])
        tok = self.lin(x, "proj_out")
        co = c["out_channels"]
        tok = tok.reshape(b, hp, hp, ps, ps, co)
        return torch.einsum("nhwpqc->nchpwq", tok).reshape(b, co, hp * ps, hp * ps)
