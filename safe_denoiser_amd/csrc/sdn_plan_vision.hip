// Launch planner, CLIP ViT vision tower with projection: build_clip_vision() and its two C entry points.
#include <math.h>

#include "sdn_plan.h"

namespace sdn_plan {

// =================================================================================================
// CLIP vision tower: `clip_model.encode_image(x)` (run_nudity_sdv3.py:101-102,158-161).  transformers'
// CLIPVisionModelWithProjection (third party): bias-free patch convolution (patch rows + a GEMM on the [hidden, Kpad] weight),
// class token + position embedding and pre_layrnorm in one row kernel, pre-LN layers with BIDIRECTIONAL self-attention and a
// quick-GELU / erf-GELU MLP (the CLIP text plan's layer without the causal mask), post_layernorm on the class rows, bias-free
// visual_projection.  last_hidden_state is the last layer's output as it is (no post_layernorm).
// =================================================================================================
void Builder::build_clip_vision() {
  const sdn_clip_vision_config& c = u->vis;
  const int C = c.hidden_size, I = c.intermediate_size, H = c.num_heads, g = c.image_size / c.patch_size, P = g * g, n = 1 + P;
  const int Kpad = (3 * c.patch_size * c.patch_size + 63) / 64 * 64;
  const int64_t rows = (int64_t)B * n, prows = (int64_t)B * P;
  Ref cls = param("embeddings.class_embedding", SDN_P_VEC_F32, C, 0);
  Ref pw = param("embeddings.patch_embedding.weight", SDN_P_MAT, C, Kpad);
  Ref pos = param("embeddings.position_embedding.weight", SDN_P_MAT, n, C);
  Ref pg = param("pre_layrnorm.weight", SDN_P_VEC_F32, C, 0), pb = param("pre_layrnorm.bias", SDN_P_VEC_F32, C, 0);
  Act pr = act(prows, Kpad, P, 0);
  { Op o; o.kind = OP_PATCH_ROWS; o.a = Ref{SP_IN, 0}; o.out = R(pr); o.batch = B; o.hw = c.image_size; o.patch = c.patch_size;
    o.c1 = Kpad; o.rows = prows; o.bytes = 12.0 * B * c.image_size * c.image_size + 2.0 * prows * Kpad;
    snprintf(o.label, sizeof(o.label), "k_clip_patch_rows"); emit(o); }
  Act pp = act(prows, C, P, 0);
  gemm(GemmSpec(prows, C, Kpad, R(pr), pw, Ref(), R(pp)));
  drop(pr);
  Act x = act(rows, C, n, 0);
  { Op o; o.kind = OP_VISION_EMBED; o.a = R(pp); o.a2 = cls; o.aux = pos; o.w = pg; o.bias = pb; o.out = R(x); o.batch = B; o.hw = n;
    o.c1 = C; o.eps = 1e-5f; o.rows = rows; o.bytes = 2.0 * (prows + rows) * C;
    snprintf(o.label, sizeof(o.label), "k_clip_vision_embed"); emit(o); }
  drop(pp);
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
    { Op o; o.kind = OP_ATTN; o.a = R(qkv); o.k = Ref{SP_WS, qkv.off + (int64_t)C * es}; o.v = Ref{SP_WS, qkv.off + (int64_t)2 * C * es};
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
    gemm(GemmSpec(rows, I, C, R(ln), f1w, f1b, R(h)).with_act(c.act));
    drop(ln);
    x = act(rows, C, n, 0);
    gemm(GemmSpec(rows, C, I, R(h), f2w, f2b, R(x)).with_residual(R(x2)));
    drop(h); drop(x2);
  }
  // last_hidden_state: skipped by the interpreter when the caller gave no buffer
  { Op o; o.kind = OP_COPY_ROWS; o.a = R(x); o.out = Ref{SP_OUT, 0}; o.batch = B; o.hw = n; o.c1 = C;
    o.bytes = 2.0 * es * rows * C; snprintf(o.label, sizeof(o.label), "k_copy_rows"); emit(o); }
  Ref qg = param("post_layernorm.weight", SDN_P_VEC_F32, C, 0), qb = param("post_layernorm.bias", SDN_P_VEC_F32, C, 0);
  Ref vpw = param("visual_projection.weight", SDN_P_MAT, c.projection_dim, C);
  Act pooled = act(B, C, 1, 0);
  { Op o; o.kind = OP_CLASS_ROWS; o.a = R(x); o.w = qg; o.bias = qb; o.out = R(pooled); o.batch = B; o.hw = n; o.c1 = C; o.eps = 1e-5f;
    o.rows = B; o.bytes = 2.0 * es * B * C; snprintf(o.label, sizeof(o.label), "k_clip_class_rows"); emit(o); }
  drop(x);
  gemm(GemmSpec(B, c.projection_dim, C, R(pooled), vpw, Ref(), Ref{SP_OUT2, 0}));
  drop(pooled);
  plan->ws_bytes = arena.peak;
}

}  // namespace sdn_plan

using namespace sdn_plan;

extern "C" int sdn_clip_vision_create(const sdn_clip_vision_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  // widths: the projected CLIP text plan's rules (its ceiling, bigG's 1280, covers ViT-L's 1024 and ViT-H's 1280); at most 4096
  // patches; heads of 64 (ViT-L) or 80 (ViT-H): the two head dimensions of the unmasked 16-bit attention kernel a ViT uses
  const bool head_ok = cfg->num_heads > 0 && (cfg->hidden_size == (int64_t)64 * cfg->num_heads || cfg->hidden_size == (int64_t)80 * cfg->num_heads);
  if (cfg->image_size <= 0 || cfg->patch_size <= 0 || cfg->patch_size > 64 || cfg->image_size % cfg->patch_size != 0 ||
      cfg->image_size / cfg->patch_size > 64 || cfg->hidden_size <= 0 || cfg->hidden_size % 128 != 0 || cfg->hidden_size > 1280 ||
      cfg->intermediate_size <= 0 || cfg->intermediate_size % 128 != 0 || cfg->num_layers <= 0 || cfg->num_heads <= 0 ||
      !head_ok || cfg->projection_dim <= 0 || cfg->projection_dim % 32 != 0 ||
      (cfg->act != SDN_ACT_QUICK_GELU && cfg->act != SDN_ACT_GELU) || cfg->dtype < 0 || cfg->dtype > 1)
    return SDN_E_INVALID;                                       // (dtype 2 / 3, the fp32-storage modes, are not built yet)
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  u->vis = *cfg;
  u->kind = CLIP_VISION;
  get_plan(u, 1);                                               // registers the parameter manifest (batch-independent)
  *out = u;
  return SDN_OK;
}

extern "C" int sdn_clip_vision_forward(sdn_unet* m, const void* weights, const float* pixel_values, void* last_hidden_state,
                                       void* image_embeds, int32_t batch, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || m->kind != CLIP_VISION || !pixel_values || !image_embeds) return SDN_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(pixel_values) & 15) || (reinterpret_cast<uintptr_t>(last_hidden_state) & 15) ||
      (reinterpret_cast<uintptr_t>(image_embeds) & 15))
    return SDN_E_INVALID;
  const sdn_clip_vision_config& c = m->vis;
  const int g = c.image_size / c.patch_size, n = 1 + g * g;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = pixel_values; call.out = last_hidden_state; call.out2 = image_embeds;   // out is nullable: the copy into it is skipped
  call.out_bs = (int64_t)n * c.hidden_size; call.out_rs = c.hidden_size;            // the copy's destination is contiguous
  return run_plan(m, call);
}
