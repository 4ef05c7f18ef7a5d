// Launch planner, execution: the interpreter that launches a plan's ops (one function per storage class) on the operands of one Call (what
// differs between two forwards of a handle is read from it, never from the handle), the chunked GEMM launch of the bf16x3 plan,
// run_plan() with hipGraph capture / replay and text K / V reuse, and the readers of a profiled forward.
#include "sdn_plan.h"

namespace sdn_plan {

// A GEMM of the bf16x3 plan on sdn_gemm_bf16 (triple operands, expanded weights).  The LDS-DMA tiles address each operand with
// 31-bit byte offsets, and a triple is 1.5 x its f32 tensor: the launch is cut into row chunks (whole samples for a conv) that
// stay below 2 GiB per operand.  Rows are independent, so the chunks are the same arithmetic.
static long g_x3_chunk_limit = (1L << 31) - 4096;      // bytes of A operand per launch (tests lower it: sdn_debug_set_x3_chunk_bytes)
extern "C" void sdn_debug_set_x3_chunk_bytes(long long bytes) { g_x3_chunk_limit = bytes > 0 ? (long)bytes : (1L << 31) - 4096; }

static int launch_x3t_gemm(const Op& o, const char* a, const char* w, const float* bias, const float* rowbias, const char* residual,
                           void* out, void* stream) {
  const sdn_gemm_desc& d = o.gd;
  const bool conv = d.a_mode == SDN_A_CONV3X3;
  const long rows_out_unit = conv ? (long)d.Ho * d.Wo : 256;                 // chunk granularity in output rows
  const long a_bytes_unit = conv ? (long)d.Hs * d.Ws * d.Cin * 2 : 256L * d.K * 2;
  const long units = conv ? d.M / rows_out_unit : (d.M + 255) / 256;
  long per = g_x3_chunk_limit / a_bytes_unit;                                 // units per launch
  if (per < 1) return SDN_E_INVALID;
  if (per > units) per = units;
  if (per < units) {
    // More than one launch: EQUAL chunks that are whole waves of tiles where the operand allows it.  "As many units as fit, then the
    // rest" gave 192 samples of a 960-channel 64^2 conv as 91 + 91 + 10 (6 + 6 + 1 waves of 256-row tiles on 256 CUs against 12 for
    // the rows themselves) and the 3072 row blocks of FF2 at 64^2 as 1092 + 1092 + 888 (5 + 5 + 4); 64 + 64 + 64 and 3 x 1024 are 12.
    const long n = (units + per - 1) / per;
    long even = (units + n - 1) / n;
    const int nrep = sdn_gemm_pick_tile((int)(even * rows_out_unit < d.M ? even * rows_out_unit : d.M), d.N, d.K, d.act, 0);
    const long tile_rows = nrep >= 8 ? 256 : 128, tile_cols = 32L * (nrep > 0 ? nrep : 2);
    const long tiles_per_unit = ((rows_out_unit + tile_rows - 1) / tile_rows) * ((d.N + tile_cols - 1) / tile_cols);
    long a_ = 256, b_ = tiles_per_unit % 256;                                 // q = units per whole wave of 256 tiles = 256 / gcd(256, tiles_per_unit)
    while (b_) { const long t_ = a_ % b_; a_ = b_; b_ = t_; }
    const long q = 256 / a_;
    const long aligned = (even + q - 1) / q * q;
    if (aligned <= per) even = aligned;
    per = even;
  }
  const int n_cols = d.x3_out == 2 ? d.N / 2 : d.N;                           // logical output width
  const long out_row_bytes = d.x3_out == 0 ? 0 : ((d.x3_out == 1 || d.x3_out == 4) ? 4L * n_cols : 6L * n_cols);
  if (d.x3_out == 0 && per < units) return SDN_E_INVALID;                     // (the NCHW output of conv_out is not chunked: 4 channels)
  for (long u0 = 0; u0 < units; u0 += per) {
    const long nu = units - u0 < per ? units - u0 : per;
    sdn_gemm_desc c = d;
    const long r0 = u0 * rows_out_unit;
    long rn = nu * rows_out_unit;
    if (r0 + rn > d.M) rn = d.M - r0;
    c.M = (int)rn;
    const float* rb = rowbias;
    if (rowbias && d.rows_per_batch > 0) rb = rowbias + (r0 / d.rows_per_batch) * d.ld_rowbias;   // chunks start on sample boundaries when it matters (conv)
    const int rc = sdn_gemm_bf16(&c, a + u0 * a_bytes_unit, nullptr, w, bias, rb, nullptr,
                                 residual ? residual + r0 * 4L * n_cols : nullptr, (char*)out + r0 * out_row_bytes, stream);
    if (rc != SDN_OK) return rc;
  }
  return SDN_OK;
}

// One op of a plan in the fp32-storage modes: same plan, fp32 operators (sdn_f32.hip); x3 = bf16x3 contractions (sdn_gemm_x3 /
// sdn_attention_x3).  t_dev != nullptr: the timestep is read from device memory (graph mode).
static int launch_op_f32(const sdn_unet* u, const Op& o, const Call& P, bool x3, const float* t_dev, void* stream) {
  int rc = SDN_OK;
  switch (o.kind) {
    case OP_TEMB:
      rc = sdn_temb_f32(P.scalar, t_dev, o.batch, o.c1, (void*)P(o.out), stream);
      break;
    case OP_CONV_IN:
      rc = sdn_conv_in_f32((const float*)P(o.a), P(o.w), (const float*)P(o.bias), o.batch, o.c1, o.hw, o.hw, o.c2, (void*)P(o.out), stream);
      break;
    case OP_GEMM:
      if (o.x3t) { rc = launch_x3t_gemm(o, P(o.a), P(o.w), (const float*)P(o.bias), (const float*)P(o.rowbias), P(o.residual), (void*)P(o.out), stream); break; }
      if (o.dyn_ldc) {
        sdn_gemm_desc gd = o.gd; gd.ldc = (int)P.out2_rs;
        rc = (x3 ? sdn_gemm_x3 : sdn_gemm_f32)(&gd, P(o.a), nullptr, P(o.w), nullptr, nullptr, nullptr, nullptr, (void*)P(o.out), stream);
        break;
      }
      rc = (o.ln || o.gd.split_k > 1) ? SDN_E_INVALID
           : (x3 ? sdn_gemm_x3 : sdn_gemm_f32)(&o.gd, P(o.a), P(o.a2), P(o.w), (const float*)P(o.bias), (const float*)P(o.rowbias),
                                               (const float*)P(o.rowgate), P(o.residual), (void*)P(o.out), stream);
      break;
    case OP_QK_RMSNORM:                          // dtype 2 and 3 both store f32
      rc = sdn_qk_rmsnorm(2, (void*)P(o.a), o.rows, o.heads, o.ldq, (const float*)P(o.w), (const float*)P(o.bias), o.eps, stream);
      break;
    case OP_SPLIT3:
      rc = sdn_split3((const float*)P(o.a), (const float*)P(o.a2), o.rows, o.c1, o.c2, (void*)P(o.out), stream);
      break;
    case OP_GN:
      rc = (o.tri_out ? sdn_groupnorm_f32_triple : sdn_groupnorm_f32)(P(o.a), P(o.a2), o.batch, o.hw, o.c1, o.c2, o.groups, o.eps, o.silu,
                                                                     (const float*)P(o.w), (const float*)P(o.bias), (void*)P(o.out),
                                                                     (float*)P(o.aux), stream);
      break;
    case OP_LN:
      if (o.mod) {                                 // MMDiT adaLN: w = scale, bias = shift (per-sample rows)
        rc = o.tri_out ? SDN_E_INVALID
                       : sdn_layernorm_mod_f32(P(o.a), o.rows, o.c1, o.eps, (const float*)P(o.w), (const float*)P(o.bias), o.ld_mod,
                                               o.hw, (void*)P(o.out), stream);
        break;
      }
      rc = (o.tri_out ? sdn_layernorm_f32_triple : sdn_layernorm_f32)(P(o.a), o.rows, o.c1, o.eps, (const float*)P(o.w),
                                                                      (const float*)P(o.bias), (void*)P(o.out), stream);
      break;
    case OP_PATCHIFY:
      rc = sdn_patchify_f32((const float*)P(o.a), o.batch, o.c1, o.hw, o.hw, o.patch, (void*)P(o.out), stream);
      break;
    case OP_UNPATCHIFY:
      rc = sdn_unpatchify_f32((const float*)P(o.a), o.batch, o.c1, o.hw, o.hw, o.patch, (float*)P(o.out), stream);
      break;
    case OP_ATTN:
      if (o.pair_in == 1) {                        // ld = 2 x (qkv width) bf16 elements, lo plane = one width on
        rc = sdn_attention_x3_pairs(P(o.a), P(o.a) + (size_t)o.ldo * 2, P(o.a) + (size_t)o.ldo * 4, o.ldq, o.ldq, (void*)P(o.out), o.batch, o.heads,
                                    o.nq, o.nk, o.hd, 2 * o.ldq, 2 * o.ldk, 2 * o.ldv, o.ldo, o.scale, o.tri_out, stream);
        break;
      }
      if (o.pair_in == 2) {                        // q rows [hi(C) | lo(C)]; k / v = column blocks 0 / C of the rows [hi(2C) | lo(2C)]
        rc = sdn_attention_x3_pairs(P(o.a), P(o.k), P(o.k) + (size_t)o.ldo * 2, o.ldq, o.ldk, (void*)P(o.out), o.batch, o.heads,
                                    o.nq, o.nk, o.hd, 2 * o.ldq, 2 * o.ldk, 2 * o.ldv, o.ldo, o.scale, o.tri_out, stream);
        break;
      }
      if (o.n1 > 0) {                              // MMDiT joint attention over the image and text streams
        sdn_attn_segment2 s2{P(o.q2), P(o.k2), P(o.v2), (void*)P(o.out2), o.n1, o.ldq, o.ldk, o.ldv, o.ldo};
        rc = o.tri_out ? SDN_E_INVALID
                       : sdn_joint_attention_f32(x3 ? 1 : 0, P(o.a), P(o.k), P(o.v), (void*)P(o.out), &s2, o.batch, o.heads, o.nq, o.hd,
                                                 o.ldq, o.ldk, o.ldv, o.ldo, o.scale, stream);
        break;
      }
      rc = (o.tri_out ? sdn_attention_x3_triple : (x3 ? sdn_attention_x3 : sdn_attention_f32))(
          P(o.a), P(o.k), P(o.v), (void*)P(o.out), o.batch, o.heads, o.nq, o.nk, o.hd, o.ldq, o.ldk, o.ldv, o.ldo, o.scale, stream);
      break;
    case OP_REPEAT:
      rc = sdn_repeat(P(o.a), (size_t)o.rows, o.c1, (void*)P(o.out), stream);
      break;
    case OP_CLIP_EMBED:
      rc = sdn_clip_embed_f32((const int32_t*)P(o.a), P(o.w), P(o.bias), o.rows, o.hw, o.c1, o.c2, (void*)P(o.out), stream);
      break;
    case OP_EOS_ROWS:
      rc = sdn_clip_eos_rows(2, (const int32_t*)P(o.a), P(o.k), (const float*)P(o.w), (const float*)P(o.bias), o.batch, o.hw, o.c1, o.c2,
                             u->pcfg.eos_token_id, o.eps, (void*)P(o.out), nullptr, stream);
      break;
    case OP_COPY_ROWS:
      rc = sdn_copy_rows_strided(P(o.a), o.batch, o.hw, o.c1, 4, (void*)P(o.out), P.out_bs, P.out_rs, stream);
      break;
    case OP_CONV_ROWS:
      rc = sdn_patch_rows_f32((const float*)P(o.a), o.batch, o.hw, o.hw, o.c1, o.kh, o.kw, o.sh, o.sw, o.ph, o.pw, o.c2, (float*)P(o.out), stream);
      break;
    case OP_POOL3:
      rc = sdn_pool3_f32(o.mod, (const float*)P(o.a), o.batch, o.hw, o.hw, o.c1, o.sh, o.ph, (float*)P(o.out), o.ldo, o.c2, stream);
      break;
    case OP_RESIZE:                              // source size: the call's; target: the plan's map (the same size = layout change only)
      rc = sdn_resize_bilinear_f32((const float*)P(o.a), o.batch, P.in_h, P.in_w, o.hw, o.hw, o.scale, o.eps, (float*)P(o.out), stream);
      break;
    case OP_SPATIAL_MEAN:
      rc = sdn_spatial_mean_f32((const float*)P(o.a), o.batch, o.hw, o.c1, (float*)P(o.out), stream);
      break;
    case OP_LATENT_MIX:                          // VAE plans: fp32 NCHW on both sides in every storage mode
      rc = sdn_latent_mix((const float*)P(o.a), (const float*)P(o.w), (const float*)P(o.bias), o.batch, o.c1, o.hw,
                          o.mod ? o.scale : P.scalar /* decoder: the caller's latent_scale */, (float*)P(o.out), stream);
      break;
    case OP_SOFTMAX:                             // ... their d = C mid-block attention: f32 scores -> f32 probabilities
      rc = sdn_softmax_rows(2, (const float*)P(o.a), o.c1, o.rows, o.c1, o.scale, (void*)P(o.out), o.c1, stream);
      break;
    case OP_TRANSPOSE:                           // ... and V^T as the "weight" operand of P V
      rc = sdn_transpose32(P(o.a), (int)o.rows, o.c1, o.ldq, (void*)P(o.out), o.ldo, stream);
      break;
    case OP_MATTN:                               // 1.7 % of the encoder's FLOPs: exact f32 products in both fp32-storage modes
      rc = sdn_masked_attention_f32(P(o.a), P(o.k), P(o.v), (void*)P(o.out), P.mask, 1, o.batch, o.heads,
                                    o.nq, o.hd, o.ldq, o.ldk, o.ldv, o.ldo, o.scale, stream);
      break;
    default:
      rc = SDN_E_INVALID;
  }
  return rc;
}

// One op of a plan in the 16-bit storage modes (bf16, or f16 when `f16`).
static int launch_op_16(const sdn_unet* u, const Op& o, const Call& P, bool f16, const float* t_dev, void* stream) {
  int rc = SDN_OK;
  switch (o.kind) {
    case OP_TEMB:
      if (t_dev) rc = sdn_temb_from_device(f16 ? 1 : 0, t_dev, o.batch, o.c1, (void*)P(o.out), stream);
      else rc = (f16 ? sdn_timestep_embed_f16 : sdn_timestep_embed_bf16)(P.scalar, o.batch, o.c1, (void*)P(o.out), stream);
      break;
    case OP_CONV_IN:
      rc = (f16 ? sdn_conv_in_f16 : sdn_conv_in_bf16)((const float*)P(o.a), P(o.w), (const float*)P(o.bias), o.batch, o.c1, o.hw, o.hw, o.c2,
                            (void*)P(o.out), stream);
      break;
    case OP_ROWSTATS:
      rc = (f16 ? sdn_row_stats_f16 : sdn_row_stats_bf16)(P(o.a), o.rows, o.c1, o.eps, (float*)P(o.out), stream);
      break;
    case OP_FFN:
      rc = sdn_ffn_geglu_fused(f16 ? 1 : 0, o.rows, o.c1, P(o.a), (const float*)P(o.ln_stats), P(o.w), (const float*)P(o.ln_c),
                               (const float*)P(o.ln_d), P(o.a2), (const float*)P(o.bias), P(o.residual), (void*)P(o.out),
                               o.col.space != SP_NONE ? (float*)P(o.col) : nullptr, stream);
      break;
    case OP_EOS_ROWS:
      rc = sdn_clip_eos_rows(f16 ? 1 : 0, (const int32_t*)P(o.a), P(o.k), (const float*)P(o.w), (const float*)P(o.bias), o.batch, o.hw,
                             o.c1, o.c2, u->pcfg.eos_token_id, o.eps, (void*)P(o.out), nullptr, stream);
      break;
    case OP_COPY_ROWS:
      rc = sdn_copy_rows_strided(P(o.a), o.batch, o.hw, o.c1, 2, (void*)P(o.out), P.out_bs, P.out_rs, stream);
      break;
    case OP_PATCH_ROWS:
      rc = sdn_clip_patch_rows(f16 ? 1 : 0, (const float*)P(o.a), o.batch, o.hw, o.patch, o.c1, (void*)P(o.out), stream);
      break;
    case OP_VISION_EMBED:
      rc = sdn_clip_vision_embed(f16 ? 1 : 0, P(o.a), (const float*)P(o.a2), P(o.aux), (const float*)P(o.w), (const float*)P(o.bias), o.batch,
                                 o.hw, o.c1, o.eps, (void*)P(o.out), stream);
      break;
    case OP_CLASS_ROWS:
      rc = sdn_clip_class_rows(f16 ? 1 : 0, P(o.a), (const float*)P(o.w), (const float*)P(o.bias), o.batch, o.hw, o.c1, o.eps,
                               (void*)P(o.out), stream);
      break;
    case OP_GEMM:
      if (o.k320) {
        rc = sdn_gemm_k320(f16 ? 1 : 0, &o.gd, P(o.a), P(o.w), o.ln ? nullptr : (const float*)P(o.bias), o.ln ? (const float*)P(o.ln_c) : nullptr,
                           o.ln ? (const float*)P(o.ln_d) : nullptr, o.eps, o.ln ? nullptr : P(o.residual), (void*)P(o.out), stream);
        break;
      }
      if (o.dyn_ldc) {
        sdn_gemm_desc gd = o.gd; gd.ldc = (int)P.out2_rs;
        rc = (f16 ? sdn_gemm_f16 : sdn_gemm_bf16)(&gd, P(o.a), nullptr, P(o.w), nullptr, nullptr, nullptr, nullptr, (void*)P(o.out), stream);
        break;
      }
      if (o.ln) {
        rc = (f16 ? sdn_gemm_ln_f16 : sdn_gemm_ln_bf16)(&o.gd, P(o.a), P(o.w), (const float*)P(o.ln_c), (const float*)P(o.ln_d), o.eps,
                                                        (const float*)P(o.ln_stats), (void*)P(o.out), stream);
        break;
      }
      if (o.col.space != SP_NONE && o.gd.split_k <= 1) {
        rc = (f16 ? sdn_gemm_stats_f16 : sdn_gemm_stats_bf16)(&o.gd, P(o.a), P(o.a2), P(o.w), (const float*)P(o.bias),
                                                              (const float*)P(o.rowbias), P(o.residual), (void*)P(o.out),
                                                              (float*)P(o.col), stream);
        break;
      }
      if (o.gd.split_k > 1) {
        rc = (f16 ? sdn_gemm_splitk_f16 : sdn_gemm_splitk_bf16)(&o.gd, P(o.a), P(o.a2), P(o.w), (const float*)P(o.bias),
                                                                (const float*)P(o.rowbias), (const float*)P(o.rowgate), P(o.residual),
                                                                (void*)P(o.out), (void*)P(o.aux), (size_t)o.rows, stream);
        break;
      }
      rc = (f16 ? sdn_gemm_f16 : sdn_gemm_bf16)(&o.gd, P(o.a), P(o.a2), P(o.w), (const float*)P(o.bias), (const float*)P(o.rowbias),
                         (const float*)P(o.rowgate), P(o.residual), (void*)P(o.out), stream);
      break;
    case OP_GN:
      if (o.cols1.space != SP_NONE) {
        rc = (f16 ? sdn_groupnorm_cols_f16 : sdn_groupnorm_cols_bf16)(P(o.a), P(o.a2), o.batch, o.hw, o.c1, o.c2, o.groups, o.eps,
                                                                      o.silu, (const float*)P(o.w), (const float*)P(o.bias),
                                                                      (void*)P(o.out), (float*)P(o.aux), (const float*)P(o.cols1),
                                                                      (const float*)P(o.cols2), stream);
        break;
      }
      rc = (f16 ? sdn_groupnorm_f16 : sdn_groupnorm_bf16)(P(o.a), P(o.a2), o.batch, o.hw, o.c1, o.c2, o.groups, o.eps, o.silu,
                              (const float*)P(o.w), (const float*)P(o.bias), (void*)P(o.out), (float*)P(o.aux), stream);
      break;
    case OP_CLIP_EMBED:
      rc = sdn_clip_embed(f16 ? 1 : 0, (const int32_t*)P(o.a), P(o.w), P(o.bias), o.rows, o.hw, o.c1, o.c2, (void*)P(o.out), stream);
      break;
    case OP_MATTN:
      rc = sdn_masked_attention(f16 ? 1 : 0, P(o.a), P(o.k), P(o.v), (void*)P(o.out), P.mask, 1, o.batch,
                                o.heads, o.nq, o.hd, o.ldq, o.ldk, o.ldv, o.ldo, o.scale, stream);
      break;
    case OP_RMSNORM:
      rc = sdn_rmsnorm(f16 ? 1 : 0, P(o.a), o.mod, o.rows, o.c1, o.eps, (const float*)P(o.w), (void*)P(o.out), stream);
      break;
    case OP_QK_RMSNORM:
      rc = sdn_qk_rmsnorm(f16 ? 1 : 0, (void*)P(o.a), o.rows, o.heads, o.ldq, (const float*)P(o.w), (const float*)P(o.bias), o.eps, stream);
      break;
    case OP_EMBED:
      rc = sdn_embed_tokens(f16 ? 1 : 0, (const int32_t*)P(o.a), P(o.w), o.rows, o.c1, o.c2, (float*)P(o.out), stream);
      break;
    case OP_T5_BIAS:
      rc = sdn_t5_relative_bias(f16 ? 1 : 0, P(o.w), u->tcfg.num_buckets, u->tcfg.max_distance, o.heads, o.nq, (float*)P(o.out), stream);
      break;
    case OP_BATTN:
      rc = sdn_bias_attention(f16 ? 1 : 0, P(o.a), P(o.k), P(o.v), (void*)P(o.out), (const float*)P(o.aux), P.mask,
                              o.batch, o.heads, o.nq, o.hd, o.ldq, o.ldk, o.ldv, o.ldo, o.scale, stream);
      break;
    case OP_REPEAT:
      rc = sdn_repeat(P(o.a), (size_t)o.rows, o.c1, (void*)P(o.out), stream);
      break;
    case OP_LATENT_MIX:
      rc = sdn_latent_mix((const float*)P(o.a), (const float*)P(o.w), (const float*)P(o.bias), o.batch, o.c1, o.hw,
                          o.mod ? o.scale : P.scalar /* decoder: the caller's latent_scale */,
                          (float*)P(o.out), stream);
      break;
    case OP_SOFTMAX:
      rc = sdn_softmax_rows(f16 ? 1 : 0, (const float*)P(o.a), o.c1, o.rows, o.c1, o.scale, (void*)P(o.out), o.c1, stream);
      break;
    case OP_TRANSPOSE:
      rc = sdn_transpose16(P(o.a), (int)o.rows, o.c1, o.ldq, (void*)P(o.out), o.ldo, stream);
      break;
    case OP_PATCHIFY:
      rc = (f16 ? sdn_patchify_f16 : sdn_patchify_bf16)((const float*)P(o.a), o.batch, o.c1, o.hw, o.hw, o.patch,
                                                        (void*)P(o.out), stream);
      break;
    case OP_UNPATCHIFY:
      rc = sdn_unpatchify_f32((const float*)P(o.a), o.batch, o.c1, o.hw, o.hw, o.patch, (float*)P(o.out), stream);
      break;
    case OP_LN:
      if (o.mod) {
        rc = (f16 ? sdn_layernorm_mod_f16 : sdn_layernorm_mod_bf16)(P(o.a), o.rows, o.c1, o.eps, (const float*)P(o.w),
                                                                    (const float*)P(o.bias), o.ld_mod, o.hw,
                                                                    (void*)P(o.out), stream);
        break;
      }
      rc = (f16 ? sdn_layernorm_f16 : sdn_layernorm_bf16)(P(o.a), o.rows, o.c1, o.eps, (const float*)P(o.w), (const float*)P(o.bias),
                              (void*)P(o.out), stream);
      break;
    case OP_ATTN:
      if (o.n1 > 0) {
        sdn_attn_segment2 s2{P(o.q2), P(o.k2), P(o.v2), (void*)P(o.out2), o.n1, o.ldq, o.ldk, o.ldv, o.ldo};
        rc = sdn_joint_attention(f16 ? 1 : 0, P(o.a), P(o.k), P(o.v), (void*)P(o.out), &s2, o.batch, o.heads, o.nq, o.hd,
                                 o.ldq, o.ldk, o.ldv, o.ldo, o.scale, stream);
        break;
      }
      rc = (f16 ? sdn_attention_f16 : sdn_attention_bf16)(P(o.a), P(o.k), P(o.v), (void*)P(o.out), o.batch, o.heads, o.nq, o.nk, o.hd, o.ldq,
                              o.ldk, o.ldv, o.ldo, o.scale, stream);
      break;
    default:
      rc = SDN_E_INVALID;
  }
  return rc;
}

// Launches every op of the plan on `stream`.  t_dev != nullptr: the timestep is read from device memory (graph mode).
static int launch_ops(sdn_unet* u, const Plan* p, const Call& c, const float* t_dev, bool prof, void* stream, bool skip_text_kv = false) {
  const int sdt = u->dtype();
  const bool f32 = sdt >= 2;                                                 // fp32-storage modes (SD-v1.4 UNet, CLIP, MMDiT and VAE plans)
  for (size_t opi = 0; opi < p->ops.size(); ++opi) {
    const Op& o = p->ops[opi];
    if ((skip_text_kv && o.text_kv) || (o.kind == OP_COPY_ROWS && !c.out)) continue;   // K / V of an unchanged text stand; no last_hidden_state buffer was given
    if (prof) (void)hipEventRecord(u->ev[2 * opi], (hipStream_t)stream);
    const int rc = f32 ? launch_op_f32(u, o, c, sdt == 3, t_dev, stream) : launch_op_16(u, o, c, sdt == 1, t_dev, stream);
    if (prof) (void)hipEventRecord(u->ev[2 * opi + 1], (hipStream_t)stream);
    if (rc != SDN_OK) return rc;
  }
  return SDN_OK;
}

int run_plan(sdn_unet* u, const Call& given) {
  if (!u || !given.weights || !given.workspace || given.batch <= 0) return SDN_E_INVALID;
  Plan* p = get_plan(u, given.batch, given.n);
  if (p->ws_bytes < 0) return SDN_E_INVALID;                      // e.g. batch not a multiple of latent_repeat
  if (given.workspace_bytes < (size_t)p->ws_bytes) return SDN_E_WORKSPACE;
  Call c = given; c.kv_base = p->kv_base;
  const bool prof = u->profile_next;
  if (prof) {                                    // opt-in diagnostics: HIP events around every launch of this forward
    u->profile_next = false;
    while (u->ev.size() < 2 * p->ops.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return SDN_E_LAUNCH; u->ev.push_back(e); }
    u->profiled_batch = c.batch; u->profiled_n = c.n;
  }
  hipStream_t hs = (hipStream_t)c.stream;
  if (u->use_graph && !prof && (u->kind == UNET || u->kind == MMDIT) && p->tscalar_off >= 0) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(hs, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
      // Graph mode: small batches are launch-bound (~850 launches per forward); the forward is captured once per
      // (batch, operand addresses) and replayed.  The timestep is the only per-step scalar: it is stored to the
      // workspace by one ordinary launch and k_temb reads it from there.
      float* t_dev = (float*)((char*)c.workspace + p->tscalar_off);
      int rc = sdn_set_scalar(t_dev, c.scalar, c.stream);
      if (rc != SDN_OK) return rc;
      const sdn_unet::GraphKey key{c.batch, c.weights, c.in, c.text, c.pooled, c.out, c.workspace};
      auto it = u->graphs.find(key);
      if (it == u->graphs.end()) {
        if (u->graphs.size() >= 16) {                          // operands keep moving: graphs do not pay, stop hoarding
          (void)hipStreamSynchronize(hs);                      // a replay may still be executing on the launch stream
          for (auto& kv : u->graphs) (void)hipGraphExecDestroy(kv.second);
          u->graphs.clear();
        }
        hipGraph_t graph = nullptr;
        if (!u->cap_stream && hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking) != hipSuccess) return SDN_E_LAUNCH;
        if (hipStreamBeginCapture(u->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return SDN_E_LAUNCH;
        rc = launch_ops(u, p, c, t_dev, false, (void*)u->cap_stream);   // records, does not run
        const hipError_t ec = hipStreamEndCapture(u->cap_stream, &graph);
        if (rc != SDN_OK || ec != hipSuccess || !graph) { if (graph) (void)hipGraphDestroy(graph); return rc != SDN_OK ? rc : SDN_E_LAUNCH; }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess || !exec) return SDN_E_LAUNCH;
        it = u->graphs.emplace(key, exec).first;
      }
      u->kv_version = 0;                                       // the replay rewrites every K / V slot: nothing to reuse afterwards
      return hipGraphLaunch(it->second, hs) == hipSuccess ? SDN_OK : SDN_E_LAUNCH;
    }
  }
  // text K / V reuse (ordinary launches only: a captured graph holds a fixed op list; only UNet plans emit text_kv ops)
  const bool declared = u->kind == UNET && u->text_version != 0 && u->subbatch_bytes == 0;
  const bool skip = declared && !prof && u->kv_version == u->text_version && u->kv_batch == c.batch && u->kv_w == c.weights &&
                    u->kv_text == c.text && u->kv_ws == c.workspace;
  const int rc_l = launch_ops(u, p, c, nullptr, prof, c.stream, skip);
  if (rc_l == SDN_OK && declared) { u->kv_version = u->text_version; u->kv_batch = c.batch; u->kv_w = c.weights; u->kv_text = c.text; u->kv_ws = c.workspace; }
  else if (!declared) u->kv_version = 0;
  return rc_l;
}

// Configuration calls (not on the hot path) drop the cached graphs; a replay may still be in flight on whatever stream the
// caller launched it, so the device is drained first.
void drop_graphs(sdn_unet* u) {
  if (u->graphs.empty()) return;
  (void)hipDeviceSynchronize();
  for (auto& kv : u->graphs) (void)hipGraphExecDestroy(kv.second);
  u->graphs.clear();
}

}  // namespace sdn_plan

using namespace sdn_plan;

// Milliseconds op i of the profiled forward took (between its two events); false when they cannot be read.
static bool op_ms(const sdn_unet* u, size_t i, float* ms) {
  return hipEventSynchronize(u->ev[2 * i + 1]) == hipSuccess && hipEventElapsedTime(ms, u->ev[2 * i], u->ev[2 * i + 1]) == hipSuccess;
}

// Undeclared debug hook (tools/profile_ops.py): per-launch rows of the profiled forward, in plan order.
// out[i*6 + {0..5}] = {ms, flops, bytes, M, N, K}; labels[i*24..] = kernel label.  Returns the op count.
extern "C" int sdn_debug_profile_ops(sdn_unet* u, double* out, char* labels, int max_ops) {
  if (!u || !out || !labels || u->profiled_batch <= 0) return -1;
  Plan* p = get_plan(u, u->profiled_batch, u->profiled_n);
  int n = 0;
  for (size_t i = 0; i < p->ops.size() && n < max_ops; ++i, ++n) {
    float ms = 0.f;
    if (!op_ms(u, i, &ms)) return -2;
    const Op& o = p->ops[i];
    out[n * 6 + 0] = ms; out[n * 6 + 1] = o.flops; out[n * 6 + 2] = o.bytes;
    out[n * 6 + 3] = o.kind == OP_GEMM ? o.gd.M : (o.kind == OP_ATTN ? o.nq : o.rows);
    out[n * 6 + 4] = o.kind == OP_GEMM ? o.gd.N : (o.kind == OP_ATTN ? o.nk : o.c1);
    out[n * 6 + 5] = o.kind == OP_GEMM ? o.gd.K : (o.kind == OP_ATTN ? o.hd : o.c2);
    memcpy(labels + n * 24, o.label, 24);
  }
  return n;
}

// Undeclared debug hook (tools/plan_fingerprint.py, tests/test_plan_digests.py): 64-bit FNV-1a over everything the planner decided for
// (batch, n) -- the plan header, every op field by field in declaration order (never a whole Op: padding), then the handle's fold
// jobs.  gd is hashed for OP_GEMM only: no other emitter initialises it.  Host only.
namespace {
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } }
  template <class T> void operator()(const T& v) { bytes(&v, sizeof(T)); }     // scalars only
  void operator()(const Ref& r) { (*this)(r.space); (*this)(r.off); }
};
}  // namespace
extern "C" int sdn_debug_plan_digest(sdn_unet* u, int32_t batch, int32_t n, uint64_t* out) {
  if (!u || !out || batch <= 0) return SDN_E_INVALID;
  const Plan* p = get_plan(u, batch, n);
  Fnv f;
  f(p->batch); f(p->tscalar_off); f(p->ws_bytes); f(p->kv_base); f(p->flops); f(p->attn_flops); f((uint64_t)p->ops.size());
  static_assert(sizeof(sdn_gemm_desc) == 25 * sizeof(int32_t), "sdn_gemm_desc: 25 int32 fields");
  for (const Op& o : p->ops) {
    f(o.kind);
    if (o.kind == OP_GEMM) for (int i = 0; i < 25; ++i) f(((const int32_t*)&o.gd)[i]);
    f(o.a); f(o.a2); f(o.w); f(o.bias); f(o.rowbias); f(o.rowgate); f(o.residual); f(o.out); f(o.aux);
    f(o.q2); f(o.k2); f(o.v2); f(o.out2);
    f(o.col); f(o.cols1); f(o.cols2);
    f(o.ln_c); f(o.ln_d); f(o.ln_stats);
    f(o.ln); f(o.text_kv); f(o.x3t); f(o.pair_in); f(o.tri_out); f(o.dyn_ldc); f(o.k320);
    f(o.n1); f(o.mod); f(o.ld_mod); f(o.patch);
    f(o.batch); f(o.hw); f(o.c1); f(o.c2); f(o.groups); f(o.silu);
    f(o.eps); f(o.rows);
    f(o.heads); f(o.nq); f(o.nk); f(o.hd); f(o.ldq); f(o.ldk); f(o.ldv); f(o.ldo);
    f(o.scale); f(o.k); f(o.v);
    f(o.kh); f(o.kw); f(o.sh); f(o.sw); f(o.ph); f(o.pw);
    f.bytes(o.label, sizeof(o.label)); f(o.flops); f(o.bytes);
  }
  for (const sdn_unet::FoldJob& j : u->fold_jobs) {
    f(j.w); f(j.gamma); f(j.beta); f(j.bias); f(j.wf); f(j.c); f(j.d); f(j.rows); f(j.cols); f(j.kind); f(j.group);
  }
  *out = f.h;
  return SDN_OK;
}

extern "C" int sdn_unet_profile_read(sdn_unet* u, sdn_profile_row* rows, int32_t max_rows) {
  if (!u || !rows || max_rows <= 0 || u->profiled_batch <= 0) return SDN_E_INVALID;
  Plan* p = get_plan(u, u->profiled_batch, u->profiled_n);
  if (u->ev.size() < 2 * p->ops.size()) return SDN_E_INVALID;
  int n = 0;
  for (size_t i = 0; i < p->ops.size(); ++i) {
    float ms = 0.f;
    if (!op_ms(u, i, &ms)) return SDN_E_LAUNCH;
    const Op& o = p->ops[i];
    int r = 0;
    for (; r < n; ++r) if (strcmp(rows[r].kernel, o.label) == 0) break;
    if (r == n) {
      if (n == max_rows) return SDN_E_INVALID;
      memset(&rows[r], 0, sizeof(rows[r]));
      snprintf(rows[r].kernel, sizeof(rows[r].kernel), "%s", o.label);
      ++n;
    }
    rows[r].launches += 1; rows[r].ms += ms; rows[r].flops += o.flops; rows[r].bytes += o.bytes;
  }
  return n;
}
