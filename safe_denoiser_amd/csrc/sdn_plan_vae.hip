// Launch planner, AutoencoderKL: the VAE's resnet and single-head attention blocks, build_vae() (decoder) and
// build_vae_encoder().
#include <math.h>

#include "sdn_plan.h"

namespace sdn_plan {

// =================================================================================================
// AutoencoderKL decoder: vae.decode(latents / scaling_factor) of
// StableDiffusionPipeline.decode_latents (...threshold_time.py:589).  diffusers-0.29.0 definitions (third party,
// restated): Decoder = conv_in -> UNetMidBlock2D(resnet, 1-head attention, resnet) -> UpDecoderBlock2D x n
// (layers_per_block + 1 resnets, nearest-2x + conv except the last) -> GroupNorm -> SiLU -> conv_out; resnets have no
// time embedding, every norm uses eps 1e-6.
// =================================================================================================
Act Builder::vae_resnet(const std::string& pfx, Act& x, int cout) {
  const int cin = x.C;
  Ref n1g = param(pfx + ".norm1.weight", SDN_P_VEC_F32, cin, 0), n1b = param(pfx + ".norm1.bias", SDN_P_VEC_F32, cin, 0);
  Ref c1w = param(pfx + ".conv1.weight", SDN_P_CONV3X3, cout, 9 * cin), c1b = param(pfx + ".conv1.bias", SDN_P_VEC_F32, cout, 0);
  Ref n2g = param(pfx + ".norm2.weight", SDN_P_VEC_F32, cout, 0), n2b = param(pfx + ".norm2.bias", SDN_P_VEC_F32, cout, 0);
  Ref c2w = param(pfx + ".conv2.weight", SDN_P_CONV3X3, cout, 9 * cout), c2b = param(pfx + ".conv2.bias", SDN_P_VEC_F32, cout, 0);
  const int64_t rows = (int64_t)B * x.hw;
  Act g1 = act(rows, cin, x.hw, x.side);
  groupnorm(x, nullptr, 1e-6f, 1, n1g, n1b, g1);
  Act h = act_gn(rows, cout, x.hw, x.side);
  conv3x3(ConvSpec(g1, cout, c1w, c1b, R(h)).with_cols(stats_of(h)));
  drop(g1);
  Act g2 = act(rows, cout, x.hw, x.side);
  groupnorm(h, nullptr, 1e-6f, 1, n2g, n2b, g2);
  drop(h);
  Act out = act_gn(rows, cout, x.hw, x.side);
  Act sc;                                                    // the shortcut: x itself, or its 1x1 conv
  if (cin != cout) {
    Ref scw = param(pfx + ".conv_shortcut.weight", SDN_P_MAT, cout, cin), scb = param(pfx + ".conv_shortcut.bias", SDN_P_VEC_F32, cout, 0);
    sc = act(rows, cout, x.hw, x.side);
    gemm(GemmSpec(rows, cout, cin, R(x), scw, scb, R(sc)));
  }
  conv3x3(ConvSpec(g2, cout, c2w, c2b, R(out)).with_residual(cin != cout ? R(sc) : R(x)).with_cols(stats_of(out)));
  drop(sc); drop(g2);
  return out;
}

// Attention(C, heads = 1, dim_head = C) with GroupNorm, biased q/k/v/out linears and a residual connection.
// d = C = 512 does not fit the flash kernel: per image  S = Q K^T (fp32) -> row softmax -> P V.
Act Builder::vae_attention(const std::string& pfx, Act& x) {
  const int C = x.C, hw = x.hw;
  const int64_t rows = (int64_t)B * hw;
  Ref gg = param(pfx + ".group_norm.weight", SDN_P_VEC_F32, C, 0), gb = param(pfx + ".group_norm.bias", SDN_P_VEC_F32, C, 0);
  Ref qw = param(pfx + ".to_q.weight", SDN_P_MAT, C, C), qb = param(pfx + ".to_q.bias", SDN_P_VEC_F32, C, 0);
  Ref kw = param(pfx + ".to_k.weight", SDN_P_MAT, C, C), kb = param(pfx + ".to_k.bias", SDN_P_VEC_F32, C, 0);
  Ref vw = param(pfx + ".to_v.weight", SDN_P_MAT, C, C), vb = param(pfx + ".to_v.bias", SDN_P_VEC_F32, C, 0);
  Ref ow = param(pfx + ".to_out.0.weight", SDN_P_MAT, C, C), ob = param(pfx + ".to_out.0.bias", SDN_P_VEC_F32, C, 0);
  Act gn = act(rows, C, hw, x.side);
  groupnorm(x, nullptr, 1e-6f, 0, gg, gb, gn);
  // three dense projections (not one stacked GEMM): the per-image Q K^T / P V GEMMs below take dense operands
  Act q = act(rows, C, hw, x.side), k = act(rows, C, hw, x.side), v = act(rows, C, hw, x.side);
  gemm(GemmSpec(rows, C, C, R(gn), qw, qb, R(q)));
  gemm(GemmSpec(rows, C, C, R(gn), kw, kb, R(k)));
  gemm(GemmSpec(rows, C, C, R(gn), vw, vb, R(v)));
  drop(gn);
  Act at = act(rows, C, hw, x.side);
  // fp32 scores of ONE image -- of one block of at most 4096 queries when the image has more tokens (1024 x 1024:
  // 16384) -- reused block after block (stream order)
  const int qrows = hw > 4096 ? 4096 : hw;
  Act sc = act(qrows, hw, 0, 0, 4);
  Act pr = act(qrows, hw);                                         // probabilities and V^T in the storage type (f32 in the fp32-storage plans)
  Act vt = act(C, hw);
  const float scale = 1.0f / sqrtf((float)C);
  for (int b = 0; b < B; ++b) {
    const int64_t img = (int64_t)b * hw * C * es;
    { Op o; o.kind = OP_TRANSPOSE; o.a = Ref{SP_WS, v.off + img}; o.out = R(vt); o.rows = hw; o.c1 = C; o.ldq = C;
      o.ldo = hw; o.bytes = 4.0 * hw * C; snprintf(o.label, sizeof(o.label), "k_transpose16"); emit(o); }
    for (int r0 = 0; r0 < hw; r0 += qrows) {
      const int64_t rowoff = (int64_t)r0 * C * es;
      { // S = Q K^T : A = this block's Q rows, "weight" operand = the image's K rows
        Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
        o.gd.M = qrows; o.gd.N = hw; o.gd.K = C; o.gd.a_mode = SDN_A_PLAIN; o.gd.out_kind = SDN_OUT_F32;
        o.a = Ref{SP_WS, q.off + img + rowoff}; o.w = Ref{SP_WS, k.off + img}; o.out = R(sc);
        o.flops = 2.0 * qrows * (double)hw * C; o.bytes = 2.0 * (qrows + (double)hw) * C + 4.0 * qrows * (double)hw;
        snprintf(o.label, sizeof(o.label), "k_gemm<%d>", sdn_gemm_pick_tile(qrows, hw, C, SDN_ACT_NONE));
        emit(o, /*attn=*/true);
      }
      { Op o; o.kind = OP_SOFTMAX; o.a = R(sc); o.out = R(pr); o.rows = qrows; o.c1 = hw; o.scale = scale;
        o.bytes = 6.0 * qrows * (double)hw; snprintf(o.label, sizeof(o.label), "k_softmax_rows"); emit(o); }
      { // O = P V : A = P [qrows, hw], "weight" = V^T [C, hw]
        Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
        o.gd.M = qrows; o.gd.N = C; o.gd.K = hw; o.gd.a_mode = SDN_A_PLAIN; o.gd.out_kind = SDN_OUT_BF16;
        o.a = R(pr); o.w = R(vt); o.out = Ref{SP_WS, at.off + img + rowoff};
        o.flops = 2.0 * qrows * (double)hw * C; o.bytes = 2.0 * (qrows * (double)hw + (qrows + (double)hw) * C);
        snprintf(o.label, sizeof(o.label), "k_gemm<%d>", sdn_gemm_pick_tile(qrows, C, hw, SDN_ACT_NONE));
        emit(o, /*attn=*/true);
      }
    }
  }
  drop(sc); drop(pr); drop(vt); drop(q); drop(k); drop(v);
  Act out = act_gn(rows, C, hw, x.side);
  gemm(GemmSpec(rows, C, C, R(at), ow, ob, R(out)).with_residual(R(x)).with_cols(stats_of(out)));
  drop(at);
  return out;
}

// fp32-storage plans (dtype 2 / 3): the shared emitters above label and size their ops for the 16-bit kernels.  The op list is the
// same; what launch_op_f32 runs for each kind, and the algorithmic bytes at 4 B per element, are filled in here (FLOPs are
// algorithmic and do not change with the storage type).
void Builder::vae_f32_rows() {
  const bool x3 = u->vcfg.dtype == 3;
  for (Op& o : plan->ops) {
    const char* label = nullptr;
    switch (o.kind) {
      case OP_GEMM: {
        const sdn_gemm_desc& d = o.gd;
        const double a_el = d.a_mode == SDN_A_CONV3X3 ? (double)(d.M / (d.Ho * d.Wo)) * d.Hs * d.Ws * d.Cin : (double)d.M * d.K;
        const double out_el = (double)d.M * (d.n_valid > 0 ? d.n_valid : d.N);
        o.bytes = 4.0 * (a_el + (double)d.N * d.K + out_el + (o.residual.space != SP_NONE ? out_el : 0.0));
        label = (x3 && d.M >= 64) ? "k_gemm_x3" : "k_gemm_f32";            // (sdn_gemm_x3 hands fewer than 64 rows to the f32 tile)
        break;
      }
      case OP_GN: o.bytes = 12.0 * (double)o.batch * o.hw * (o.c1 + o.c2); label = "k_gn_rows_f32"; break;   // two reads, one write
      case OP_CONV_IN: o.bytes = 4.0 * (double)o.batch * o.hw * o.hw * (o.c1 + o.c2); label = "k_conv_in_f32"; break;
      case OP_SOFTMAX: o.bytes = 8.0 * (double)o.rows * o.c1; label = "k_softmax_rows_f32"; break;
      case OP_TRANSPOSE: o.bytes = 8.0 * (double)o.rows * o.c1; label = "k_transpose32"; break;
      default: break;                                                       // k_latent_mix: fp32 NCHW on both sides in every mode
    }
    if (label) snprintf(o.label, sizeof(o.label), "%s", label);
  }
}

void Builder::build_vae() {
  const sdn_vae_config& c = u->vcfg;
  const int S = c.sample_size, L = c.latent_channels, n = c.n_levels;
  const int ctop = c.block_out_channels[n - 1];
  char buf[96];
  gn_stats = Ref{SP_WS, arena.alloc((int64_t)B * 129 * 64 * 2 * 4)};
  Ref pqw = param("post_quant_conv.weight", SDN_P_VEC_F32, L * L, 0), pqb = param("post_quant_conv.bias", SDN_P_VEC_F32, L, 0);
  Act z = act((int64_t)B * L, S * S, 0, 0, 4);                    // fp32 NCHW
  { Op o; o.kind = OP_LATENT_MIX; o.batch = B; o.c1 = L; o.hw = S * S; o.a = Ref{SP_IN, 0}; o.w = pqw; o.bias = pqb; o.out = R(z);
    o.flops = 2.0 * B * S * S * (double)L * L; o.bytes = 8.0 * B * S * S * L; snprintf(o.label, sizeof(o.label), "k_latent_mix"); emit(o); }
  Ref ciw = param("decoder.conv_in.weight", SDN_P_CONV3X3, ctop, 9 * L), cib = param("decoder.conv_in.bias", SDN_P_VEC_F32, ctop, 0);
  Act cur = act((int64_t)B * S * S, ctop, S * S, S);
  { Op o; o.kind = OP_CONV_IN; o.batch = B; o.c1 = L; o.c2 = ctop; o.hw = S; o.a = R(z); o.w = ciw; o.bias = cib; o.out = R(cur);
    o.flops = 2.0 * B * S * S * (double)ctop * 9 * L; o.bytes = (double)B * S * S * (4.0 * L + 2.0 * ctop);
    snprintf(o.label, sizeof(o.label), "k_conv_in"); emit(o); }
  drop(z);
  { Act r = vae_resnet("decoder.mid_block.resnets.0", cur, ctop); drop(cur); cur = r; }
  { Act r = vae_attention("decoder.mid_block.attentions.0", cur); drop(cur); cur = r; }
  { Act r = vae_resnet("decoder.mid_block.resnets.1", cur, ctop); drop(cur); cur = r; }
  for (int i = 0; i < n; ++i) {
    const int cout = c.block_out_channels[n - 1 - i];
    for (int j = 0; j <= c.layers_per_block; ++j) {
      snprintf(buf, sizeof(buf), "decoder.up_blocks.%d.resnets.%d", i, j);
      Act r = vae_resnet(buf, cur, cout);
      drop(cur); cur = r;
    }
    if (i + 1 < n) {
      snprintf(buf, sizeof(buf), "decoder.up_blocks.%d.upsamplers.0.conv", i);
      Ref w = param(std::string(buf) + ".weight", SDN_P_CONV3X3, cout, 9 * cout), bb = param(std::string(buf) + ".bias", SDN_P_VEC_F32, cout, 0);
      const int s2 = cur.side * 2;
      Act up = act_gn((int64_t)B * s2 * s2, cout, s2 * s2, s2);
      conv3x3(ConvSpec(cur, cout, w, bb, R(up)).with_upsample().with_cols(stats_of(up)));
      drop(cur); cur = up;
    }
  }
  const int c0 = c.block_out_channels[0];
  Ref og = param("decoder.conv_norm_out.weight", SDN_P_VEC_F32, c0, 0), ob = param("decoder.conv_norm_out.bias", SDN_P_VEC_F32, c0, 0);
  const int npad = 32;
  Ref cow = param("decoder.conv_out.weight", SDN_P_CONV3X3, c.out_channels, 9 * c0, npad);
  Ref cob = param("decoder.conv_out.bias", SDN_P_VEC_F32, c.out_channels, 0, npad);
  Act g = act((int64_t)B * cur.hw, c0, cur.hw, cur.side);
  groupnorm(cur, nullptr, 1e-6f, 1, og, ob, g);
  drop(cur);
  conv3x3(ConvSpec(g, c.out_channels, cow, cob, Ref{SP_OUT, 0}).with_nchw_out(npad));
  drop(g);
  if (es == 4) vae_f32_rows();
  plan->ws_bytes = arena.peak;
}
// AutoencoderKL encoder (the proj_ref builder's embed_fn, run_nudity.py:308): conv_in -> DownEncoderBlock2D x n
// (layers_per_block resnets; Downsample2D(padding=0) = F.pad (0,1,0,1) + conv3x3 stride 2 on all but the last) ->
// UNetMidBlock2D -> GroupNorm -> SiLU -> conv_out (2L moments) -> quant_conv 1x1.  Output: fp32 NCHW moments
// [B, 2L, S, S] (mean | logvar); sampling is sdn_gaussian_sample.
void Builder::build_vae_encoder() {
  const sdn_vae_config& c = u->vcfg;
  const int n = c.n_levels, L = c.latent_channels;
  const int S0 = c.sample_size << (n - 1);                         // image side
  char buf[96];
  gn_stats = Ref{SP_WS, arena.alloc((int64_t)B * 129 * 64 * 2 * 4)};
  const int c0 = c.block_out_channels[0];
  Ref ciw = param("encoder.conv_in.weight", SDN_P_CONV3X3, c0, 9 * c.out_channels), cib = param("encoder.conv_in.bias", SDN_P_VEC_F32, c0, 0);
  Act cur = act((int64_t)B * S0 * S0, c0, S0 * S0, S0);
  { Op o; o.kind = OP_CONV_IN; o.batch = B; o.c1 = c.out_channels; o.c2 = c0; o.hw = S0; o.a = Ref{SP_IN, 0}; o.w = ciw; o.bias = cib; o.out = R(cur);
    o.flops = 2.0 * B * S0 * S0 * (double)c0 * 9 * c.out_channels; o.bytes = (double)B * S0 * S0 * (4.0 * c.out_channels + 2.0 * c0);
    snprintf(o.label, sizeof(o.label), "k_conv_in"); emit(o); }
  for (int i = 0; i < n; ++i) {
    const int cout = c.block_out_channels[i];
    for (int j = 0; j < c.layers_per_block; ++j) {
      snprintf(buf, sizeof(buf), "encoder.down_blocks.%d.resnets.%d", i, j);
      Act r = vae_resnet(buf, cur, cout);
      drop(cur); cur = r;
    }
    if (i + 1 < n) {
      snprintf(buf, sizeof(buf), "encoder.down_blocks.%d.downsamplers.0.conv", i);
      Ref w = param(std::string(buf) + ".weight", SDN_P_CONV3X3, cout, 9 * cout), bb = param(std::string(buf) + ".bias", SDN_P_VEC_F32, cout, 0);
      const int s2 = cur.side / 2;
      Act d = act_gn((int64_t)B * s2 * s2, cout, s2 * s2, s2);
      conv3x3(ConvSpec(cur, cout, w, bb, R(d)).with_stride(2, /*asym_pad=*/1).with_cols(stats_of(d)));
      drop(cur); cur = d;
    }
  }
  const int ctop = c.block_out_channels[n - 1];
  { Act r = vae_resnet("encoder.mid_block.resnets.0", cur, ctop); drop(cur); cur = r; }
  { Act r = vae_attention("encoder.mid_block.attentions.0", cur); drop(cur); cur = r; }
  { Act r = vae_resnet("encoder.mid_block.resnets.1", cur, ctop); drop(cur); cur = r; }
  Ref og = param("encoder.conv_norm_out.weight", SDN_P_VEC_F32, ctop, 0), ob = param("encoder.conv_norm_out.bias", SDN_P_VEC_F32, ctop, 0);
  const int npad = 32, M2 = 2 * L;
  Ref cow = param("encoder.conv_out.weight", SDN_P_CONV3X3, M2, 9 * ctop, npad);
  Ref cob = param("encoder.conv_out.bias", SDN_P_VEC_F32, M2, 0, npad);
  Ref qw = param("quant_conv.weight", SDN_P_VEC_F32, M2 * M2, 0), qb = param("quant_conv.bias", SDN_P_VEC_F32, M2, 0);
  Act g = act((int64_t)B * cur.hw, ctop, cur.hw, cur.side);
  groupnorm(cur, nullptr, 1e-6f, 1, og, ob, g);
  const int hw = cur.hw;
  drop(cur);
  Act mom = act((int64_t)B * M2, hw, 0, 0, 4);                     // fp32 NCHW moments before quant_conv
  conv3x3(ConvSpec(g, M2, cow, cob, R(mom)).with_nchw_out(npad));
  drop(g);
  { Op o; o.kind = OP_LATENT_MIX; o.batch = B; o.c1 = M2; o.hw = hw; o.a = R(mom); o.w = qw; o.bias = qb; o.out = Ref{SP_OUT, 0};
    o.mod = 1; o.scale = 1.0f;
    o.flops = 2.0 * B * hw * (double)M2 * M2; o.bytes = 8.0 * B * hw * M2; snprintf(o.label, sizeof(o.label), "k_latent_mix"); emit(o); }
  drop(mom);
  if (es == 4) vae_f32_rows();
  plan->ws_bytes = arena.peak;
}

}  // namespace sdn_plan
