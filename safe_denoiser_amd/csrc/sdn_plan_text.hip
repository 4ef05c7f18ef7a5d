// Launch planner, text encoders: build_clip() (CLIPTextModel, and CLIPTextModelWithProjection's tapped hidden state and pooled
// projection tail), and the T5 encoder's emitters (gated weight pair, f32-stream GEMM, RMS norm) with build_t5().
#include <math.h>

#include "sdn_plan.h"

namespace sdn_plan {

// =================================================================================================
// CLIP text encoder: `self.text_encoder(input_ids, attention_mask)[0]`
// (...threshold_time.py:197,225,287,333).  transformers' CLIPTextModel (third party): token + position embeddings,
// pre-LN transformer layers with CAUSAL self-attention and a quick-GELU MLP, final LayerNorm.
// =================================================================================================
void Builder::build_clip() {
  const sdn_clip_config& c = u->ccfg;
  const int C = c.hidden_size, I = c.intermediate_size, n = c.max_position_embeddings, H = c.num_heads;
  const int64_t rows = (int64_t)B * n;
  Ref tok = param("embeddings.token_embedding.weight", SDN_P_MAT, c.vocab_size, C);
  Ref pos = param("embeddings.position_embedding.weight", SDN_P_MAT, n, C);
  Act x = act(rows, C, n, 0);
  { Op o; o.kind = OP_CLIP_EMBED; o.a = Ref{SP_IN, 0}; o.w = tok; o.bias = pos; o.out = R(x); o.rows = rows; o.hw = n; o.c1 = C;
    o.c2 = c.vocab_size; o.bytes = 6.0 * rows * C; snprintf(o.label, sizeof(o.label), "k_clip_embed"); emit(o); }
  const bool proj = u->kind == CLIP_PROJ;
  const int mlp_act = proj ? u->pcfg.act : SDN_ACT_QUICK_GELU;
  char buf[96];
  for (int l = 0; l < c.num_layers; ++l) {
    snprintf(buf, sizeof(buf), "encoder.layers.%d", l);
    const std::string p = buf;
    Ref l1g = param(p + ".layer_norm1.weight", SDN_P_VEC_F32, C, 0), l1b = param(p + ".layer_norm1.bias", SDN_P_VEC_F32, C, 0);
    Ref qkvw = stacked({p + ".self_attn.q_proj.weight", p + ".self_attn.k_proj.weight", p + ".self_attn.v_proj.weight"}, C, C);
    Ref qkvb = stacked({p + ".self_attn.q_proj.bias", p + ".self_attn.k_proj.bias", p + ".self_attn.v_proj.bias"}, C, 0);
    Ref ow = param(p + ".self_attn.out_proj.weight", SDN_P_MAT, C, C), ob = param(p + ".self_attn.out_proj.bias", SDN_P_VEC_F32, C, 0);
    Ref l2g = param(p + ".layer_norm2.weight", SDN_P_VEC_F32, C, 0), l2b = param(p + ".layer_norm2.bias", SDN_P_VEC_F32, C, 0);
    Ref f1w = param(p + ".mlp.fc1.weight", SDN_P_MAT, I, C), f1b = param(p + ".mlp.fc1.bias", SDN_P_VEC_F32, I, 0);
    Ref f2w = param(p + ".mlp.fc2.weight", SDN_P_MAT, C, I), f2b = param(p + ".mlp.fc2.bias", SDN_P_VEC_F32, C, 0);
    Act ln = act(rows, C, n, 0);
    layernorm(x, l1g, l1b, ln);
    Act qkv = act(rows, 3 * C, n, 0);
    gemm(GemmSpec(rows, 3 * C, C, R(ln), qkvw, qkvb, R(qkv)));
    Act at = act(rows, C, n, 0);
    { Op o; o.kind = OP_MATTN; o.a = R(qkv); o.k = Ref{SP_WS, qkv.off + (int64_t)C * es}; o.v = Ref{SP_WS, qkv.off + (int64_t)2 * C * es};
      o.out = R(at); o.batch = B; o.heads = H; o.nq = n; o.nk = n; o.hd = C / H; o.ldq = o.ldk = o.ldv = 3 * C; o.ldo = C;
      o.scale = 1.0f / sqrtf((float)o.hd);
      o.flops = 4.0 * B * H * (double)n * n * o.hd; o.bytes = 2.0 * 4.0 * rows * C;
      snprintf(o.label, sizeof(o.label), "k_attn<%d>", o.hd); emit(o); }
    drop(qkv);
    Act x2 = act(rows, C, n, 0);
    gemm(GemmSpec(rows, C, C, R(at), ow, ob, R(x2)).with_residual(R(x)));
    drop(at); drop(x);
    layernorm(x2, l2g, l2b, ln);
    Act h = act(rows, I, n, 0);
    gemm(GemmSpec(rows, I, C, R(ln), f1w, f1b, R(h)).with_act(mlp_act));
    drop(ln);
    x = act(rows, C, n, 0);
    gemm(GemmSpec(rows, C, I, R(h), f2w, f2b, R(x)).with_residual(R(x2)));
    drop(h); drop(x2);
    if (proj && l == c.num_layers - u->pcfg.hidden_tap) {
      // hidden_states[-hidden_tap]: this layer's output as it is (no final norm), into the caller's strided slice
      Op o; o.kind = OP_COPY_ROWS; o.a = R(x); o.out = Ref{SP_OUT, 0}; o.batch = B; o.hw = n; o.c1 = C;
      o.bytes = 2.0 * es * rows * C; snprintf(o.label, sizeof(o.label), "k_copy_rows"); emit(o);
    }
  }
  Ref fg = param("final_layer_norm.weight", SDN_P_VEC_F32, C, 0), fb = param("final_layer_norm.bias", SDN_P_VEC_F32, C, 0);
  if (proj) {
    // text_embeds = text_projection(final_layer_norm(last)[pooling position]): the norm runs on B rows, not B x 77
    const int P = u->pcfg.projection_dim;
    Ref tpw = param("text_projection.weight", SDN_P_MAT, P, C);
    Act pooled = act(B, C, 1, 0);
    { Op o; o.kind = OP_EOS_ROWS; o.a = Ref{SP_IN, 0}; o.k = R(x); o.w = fg; o.bias = fb; o.out = R(pooled); o.batch = B; o.hw = n;
      o.c1 = C; o.c2 = c.vocab_size; o.eps = 1e-5f; o.bytes = 2.0 * es * B * C + 4.0 * rows;
      snprintf(o.label, sizeof(o.label), "k_clip_eos_rows"); emit(o); }
    drop(x);
    gemm(GemmSpec(B, P, C, R(pooled), tpw, Ref(), Ref{SP_OUT2, 0}).with_dyn_ldc());
    drop(pooled);
    plan->ws_bytes = arena.peak;
    return;
  }
  { Op o; o.kind = OP_LN; o.a = R(x); o.rows = rows; o.c1 = C; o.eps = 1e-5f; o.w = fg; o.bias = fb; o.out = Ref{SP_OUT, 0};
    o.bytes = 4.0 * rows * C; snprintf(o.label, sizeof(o.label), "k_layernorm"); emit(o); }
  drop(x);
  plan->ws_bytes = arena.peak;
}
// =================================================================================================
// T5 encoder (SD-v3 text_encoder_3): `self.text_encoder_3(input_ids, attention_mask)[0]` (models/sdv3/safe_denoiser_pipeline.py
// :316-334, :731-768, :797-827).  transformers' T5EncoderModel (third party): token embedding (no position table), pre-RMS-norm
// layers of bidirectional self-attention with a shared relative-position bias and NO 1/sqrt(d) scale, gated tanh-GELU
// feed-forward, final RMS norm; no biases.  The residual stream x stays F32: both output projections add into it in place.
// =================================================================================================
// one SDN_ACT_GEGLU* weight from two state_dict tensors: value / gate row blocks of 16 interleaved in ONE [2F, K] region
Ref Builder::glu_pair(const std::string& value_name, const std::string& gate_name, int F, int K) {
  auto it = u->param_index.find(value_name);
  if (it != u->param_index.end()) return Ref{SP_W, u->params[it->second].offset};
  const int64_t base = u->weight_bytes;
  const std::string* names[2] = {&value_name, &gate_name};
  for (int i = 0; i < 2; ++i) {
    sdn_param_info pi; memset(&pi, 0, sizeof(pi));
    snprintf(pi.name, sizeof(pi.name), "%s", names[i]->c_str());
    pi.kind = i == 0 ? SDN_P_GLU_VALUE : SDN_P_GLU_GATE; pi.rows = F; pi.cols = K; pi.rows_padded = F;
    pi.offset = base + (int64_t)i * 16 * K * es;
    u->param_index[*names[i]] = (int)u->params.size();
    u->params.push_back(pi);
  }
  u->weight_bytes += ((int64_t)2 * F * K * es + 255) & ~(int64_t)255;
  return Ref{SP_W, base};
}
// T5's GEMM: no bias; a 16-bit output, or (f32_stream) out += A W^T on the F32 residual stream, charged as a read and a write of it
void Builder::t5_gemm(const GemmSpec& s) {
  if (s.bias.space != SP_NONE || s.a2.space != SP_NONE || s.rowbias.space != SP_NONE || s.rowgate.space != SP_NONE || s.residual.space != SP_NONE ||
      s.out_kind != SDN_OUT_BF16 || s.n_valid || s.res_pre || s.k320 || s.triple_out || s.pair_out || s.force_x3t || s.text_kv || s.dyn_ldc)
    plan_bad = true;                                           // forms of gemm() / gemm_ex()
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.gd.M = (int)s.M; o.gd.N = s.N; o.gd.K = s.K; o.gd.a_mode = SDN_A_PLAIN; o.gd.act = s.act; o.gd.out_kind = SDN_OUT_BF16;
  o.a = s.a; o.w = s.w; o.out = s.out;
  if (s.f32_stream) { o.gd.f32_stream = 1; o.gd.out_kind = SDN_OUT_F32; o.residual = s.out; }   // F32 residual and output, the same tensor
  o.flops = 2.0 * (double)s.M * (double)s.N * (double)s.K;
  o.bytes = 2.0 * ((double)s.M * s.K + (double)s.N * s.K) + (s.f32_stream ? 8.0 : (s.act == SDN_ACT_GEGLU_TANH ? 1.0 : 2.0)) * (double)s.M * s.N;
  snprintf(o.label, sizeof(o.label), "k_gemm<%d>%s", sdn_gemm_pick_tile((int)s.M, s.N, s.K, s.act), s.f32_stream ? "/f32" : "");
  push_gemm(o, s.cols);
}
void Builder::t5_rmsnorm(Ref x, bool x_f32, int64_t rows, int C, Ref w, Ref out) {
  Op o; o.kind = OP_RMSNORM; o.a = x; o.mod = x_f32 ? 1 : 0; o.rows = rows; o.c1 = C; o.eps = u->tcfg.eps; o.w = w; o.out = out;
  o.bytes = (x_f32 ? 6.0 : 4.0) * (double)rows * C; snprintf(o.label, sizeof(o.label), "k_rmsnorm"); emit(o);
}
void Builder::build_t5() {
  const sdn_t5_config& c = u->tcfg;
  const int D = c.d_model, F = c.d_ff, H = c.num_heads, I = H * c.d_kv, n = seq;
  const int64_t rows = (int64_t)B * n;
  Ref tok = param("embed_tokens.weight", SDN_P_MAT, c.vocab_size, D);
  Act x = act(rows, D, n, 0, 4);
  { Op o; o.kind = OP_EMBED; o.a = Ref{SP_IN, 0}; o.w = tok; o.out = R(x); o.rows = rows; o.c1 = D; o.c2 = c.vocab_size;
    o.bytes = 6.0 * rows * D; snprintf(o.label, sizeof(o.label), "k_embed_tokens"); emit(o); }
  Act bias = act(H, 2 * n - 1, 0, 0, 4);               // computed once per forward, shared by every layer
  char buf[96];
  for (int l = 0; l < c.num_layers; ++l) {
    snprintf(buf, sizeof(buf), "block.%d.layer", l);
    const std::string p = buf;
    Ref n1 = param(p + ".0.layer_norm.weight", SDN_P_VEC_F32, D, 0);
    Ref qkvw = stacked({p + ".0.SelfAttention.q.weight", p + ".0.SelfAttention.k.weight", p + ".0.SelfAttention.v.weight"}, I, D);
    Ref ow = param(p + ".0.SelfAttention.o.weight", SDN_P_MAT, D, I);
    if (l == 0) {
      Ref tab = param(p + ".0.SelfAttention.relative_attention_bias.weight", SDN_P_MAT, c.num_buckets, H);
      Op o; o.kind = OP_T5_BIAS; o.w = tab; o.out = R(bias); o.heads = H; o.nq = n; o.bytes = 4.0 * H * (2 * n - 1);
      snprintf(o.label, sizeof(o.label), "k_t5_bias"); emit(o);
    }
    Ref n2 = param(p + ".1.layer_norm.weight", SDN_P_VEC_F32, D, 0);
    Ref wi = glu_pair(p + ".1.DenseReluDense.wi_1.weight", p + ".1.DenseReluDense.wi_0.weight", F, D);
    Ref wo = param(p + ".1.DenseReluDense.wo.weight", SDN_P_MAT, D, F);
    Act ln = act(rows, D, n, 0);
    t5_rmsnorm(R(x), true, rows, D, n1, R(ln));
    Act qkv = act(rows, 3 * I, n, 0);
    t5_gemm(GemmSpec(rows, 3 * I, D, R(ln), qkvw, Ref(), R(qkv)));
    Act at = act(rows, I, n, 0);
    { Op o; o.kind = OP_BATTN; o.a = R(qkv); o.k = Ref{SP_WS, qkv.off + (int64_t)I * es}; o.v = Ref{SP_WS, qkv.off + (int64_t)2 * I * es};
      o.aux = R(bias); o.out = R(at); o.batch = B; o.heads = H; o.nq = n; o.nk = n; o.hd = c.d_kv; o.ldq = o.ldk = o.ldv = 3 * I; o.ldo = I;
      o.scale = 1.0f;                                  // T5 folds the scale into its initialisation
      o.flops = 4.0 * B * H * (double)n * n * o.hd; o.bytes = 2.0 * 4.0 * rows * I;
      snprintf(o.label, sizeof(o.label), "k_attn<%d>/bias", o.hd); emit(o); }
    drop(qkv);
    t5_gemm(GemmSpec(rows, D, I, R(at), ow, Ref(), R(x)).with_f32_stream(true));
    drop(at);
    t5_rmsnorm(R(x), true, rows, D, n2, R(ln));
    Act h = act(rows, F, n, 0);
    t5_gemm(GemmSpec(rows, 2 * F, D, R(ln), wi, Ref(), R(h)).with_act(SDN_ACT_GEGLU_TANH));
    drop(ln);
    t5_gemm(GemmSpec(rows, D, F, R(h), wo, Ref(), R(x)).with_f32_stream(true));
    drop(h);
  }
  Ref fn = param("final_layer_norm.weight", SDN_P_VEC_F32, D, 0);
  t5_rmsnorm(R(x), true, rows, D, fn, Ref{SP_OUT, 0});
  drop(x); drop(bias);
  plan->ws_bytes = arena.peak;
}

}  // namespace sdn_plan
