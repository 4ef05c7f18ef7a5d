// Launch planner, C ABI: the sdn_*_create functions (the vision tower's is in sdn_plan_vision.hip) with their config validation, sdn_unet_prepare, the manifest / workspace /
// FLOP queries, the forward and encode / decode entry points (each states the handle kinds it accepts), sdn_unet_set_* and the
// undeclared debug hooks.
#include <algorithm>

#include "sdn_plan.h"

using namespace sdn_plan;

// Configuration calls that change what a plan contains: assign, then drop the cached graphs and plans (rebuilt on the next use).
template <class F, class V> static void set_plan_toggle(sdn_unet* u, F sdn_unet::*field, V value) {
  u->*field = value;
  drop_graphs(u);
  u->plans.clear();
}

// fp32-storage modes (dtype 2 / 3) run the plain operator chain (sdn_f32.hip): no statistics from the producers, no folded LayerNorm,
// no fused feed-forward.  A creator calls this before its first get_plan().
static void plain_chain_for_f32(sdn_unet* u, int dtype) { if (dtype >= 2) u->gn_fuse = u->ln_fold = u->ff_fuse = false; }

extern "C" {

int sdn_unet_create(const sdn_unet_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  if (cfg->n_levels < 1 || cfg->n_levels > 4 || cfg->layers_per_block < 1 || cfg->n_heads <= 0 ||
      cfg->in_channels <= 0 || cfg->in_channels > 16 || cfg->out_channels <= 0 || cfg->out_channels > 32 ||
      cfg->sample_size <= 0 || (cfg->sample_size % (1 << (cfg->n_levels - 1))) != 0 || cfg->cross_dim % 64 != 0 ||
      cfg->text_len <= 0 || cfg->norm_groups <= 0 || cfg->norm_groups > 64 || cfg->dtype < 0 || cfg->dtype > 3 ||
      cfg->latent_repeat < 0 || cfg->latent_repeat > 8)
    return SDN_E_INVALID;
  for (int i = 0; i < cfg->n_levels; ++i) {
    const int c = cfg->block_out_channels[i];
    if (c <= 0 || c % 64 != 0 || c % cfg->norm_groups != 0 || c % cfg->n_heads != 0) return SDN_E_INVALID;
    const int hd = c / cfg->n_heads;
    if (cfg->level_has_attn[i] && hd != 40 && hd != 64 && hd != 80 && hd != 160) return SDN_E_INVALID;
    if (sdn_gemm_pick_nrep(c, SDN_ACT_NONE) == 0 || sdn_gemm_pick_nrep(8 * c, SDN_ACT_GEGLU) == 0) return SDN_E_INVALID;
  }
  {
    const int hd_mid = cfg->block_out_channels[cfg->n_levels - 1] / cfg->n_heads;       // mid block always attends
    if (hd_mid != 40 && hd_mid != 64 && hd_mid != 80 && hd_mid != 160) return SDN_E_INVALID;
  }
  sdn_unet* u = new sdn_unet();
  u->cfg = *cfg;
  plain_chain_for_f32(u, cfg->dtype);
  get_plan(u, cfg->latent_repeat > 1 ? cfg->latent_repeat : 1);   // registers the parameter manifest (batch-independent)
  *out = u;
  return SDN_OK;
}

int sdn_mmdit_create(const sdn_mmdit_config* cfg, sdn_unet** out) { return sdn_mmdit_create_ex(cfg, nullptr, out); }

int sdn_mmdit_create_ex(const sdn_mmdit_config* cfg, const sdn_mmdit_ext* ext, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  const int C = cfg->num_heads * cfg->head_dim;
  if (cfg->in_channels <= 0 || cfg->out_channels <= 0 || cfg->sample_size <= 0 || cfg->patch_size <= 0 ||
      cfg->sample_size % cfg->patch_size != 0 || cfg->num_layers <= 0 || cfg->num_heads <= 0 || cfg->head_dim != 64 ||
      C % 128 != 0 || cfg->joint_dim % 64 != 0 || cfg->pooled_dim % 64 != 0 || cfg->time_dim % 64 != 0 ||
      (cfg->in_channels * cfg->patch_size * cfg->patch_size) % 64 != 0 ||
      (cfg->out_channels * cfg->patch_size * cfg->patch_size) % 32 != 0 || cfg->text_len <= 0 || cfg->dtype < 0 ||
      cfg->dtype > 3 || C > 2560)
    return SDN_E_INVALID;
  if (ext) {                                                   // the SD-3.5 additions: NULL or all zero = the SD3 plan
    if (ext->qk_norm < 0 || ext->qk_norm > 1 || (ext->qk_norm == 1 && !(ext->qk_norm_eps > 0.f))) return SDN_E_INVALID;
    if (ext->dual_attention_mask && (cfg->num_layers > 64 || (cfg->num_layers < 64 && (ext->dual_attention_mask >> cfg->num_layers))))
      return SDN_E_INVALID;
  }
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  u->mcfg = *cfg;
  if (ext) u->mext = *ext;
  u->kind = MMDIT;
  get_plan(u, 1);
  *out = u;
  return SDN_OK;
}

int sdn_vae_decoder_create(const sdn_vae_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  if (cfg->n_levels < 1 || cfg->n_levels > 4 || cfg->layers_per_block < 1 || cfg->latent_channels <= 0 ||
      cfg->latent_channels > 16 || cfg->out_channels <= 0 || cfg->out_channels > 32 || cfg->sample_size <= 0 ||
      cfg->norm_groups <= 0 || cfg->norm_groups > 64 || cfg->dtype < 0 || cfg->dtype > 3)
    return SDN_E_INVALID;
  for (int i = 0; i < cfg->n_levels; ++i) {
    const int c = cfg->block_out_channels[i];
    if (c <= 0 || c % 64 != 0 || c % cfg->norm_groups != 0 || sdn_gemm_pick_nrep(c, SDN_ACT_NONE) == 0) return SDN_E_INVALID;
  }
  const int hw = cfg->sample_size * cfg->sample_size;         // tokens of the mid-block attention
  if (hw % 64 != 0 || hw > 16384 || (hw > 4096 && hw % 4096 != 0) || sdn_gemm_pick_nrep(hw, SDN_ACT_NONE) == 0) return SDN_E_INVALID;
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  u->cfg.norm_groups = cfg->norm_groups;
  // gn_fuse off = no activation carries a statistics slot (act_gn), so stats_of() names nothing and every GroupNorm computes its
  // own; the phase-form upsamplers are a 16-bit UNet form (Builder::conv3x3) and split-K stays off (sdn_unet_set_split_k refuses
  // these modes)
  plain_chain_for_f32(u, cfg->dtype);
  u->vcfg = *cfg;
  u->kind = VAE_DECODER;
  get_plan(u, 1);
  *out = u;
  return SDN_OK;
}

int sdn_vae_encoder_create(const sdn_vae_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  sdn_unet* u = nullptr;
  const int rc = sdn_vae_decoder_create(cfg, &u);              // same config checks; the plan is rebuilt as an encoder
  if (rc != SDN_OK) return rc;
  if (2 * cfg->latent_channels > 32) { delete u; return SDN_E_INVALID; }   // quant_conv mixes the 2L moments (sdn_latent_mix: C <= 32)
  u->kind = VAE_ENCODER;
  u->plans.clear(); u->params.clear(); u->param_index.clear(); u->weight_bytes = 0;
  get_plan(u, 1);
  *out = u;
  return SDN_OK;
}

int sdn_clip_create(const sdn_clip_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  if (cfg->vocab_size <= 0 || cfg->hidden_size <= 0 || cfg->hidden_size % 128 != 0 || cfg->hidden_size > 1024 ||
      cfg->intermediate_size <= 0 || cfg->intermediate_size % 128 != 0 || cfg->num_layers <= 0 || cfg->num_heads <= 0 ||
      cfg->hidden_size != 64 * cfg->num_heads || cfg->max_position_embeddings <= 0 || cfg->max_position_embeddings > 4096 ||
      cfg->dtype < 0 || cfg->dtype > 3)
    return SDN_E_INVALID;
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  plain_chain_for_f32(u, cfg->dtype);
  u->ccfg = *cfg;
  u->kind = CLIP;
  get_plan(u, 1);
  *out = u;
  return SDN_OK;
}

int sdn_clip_proj_create(const sdn_clip_proj_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  // widths: the CLIP plan's rules with the ceiling at bigG's 1280 (the widest size the tests run)
  if (cfg->vocab_size <= 0 || cfg->hidden_size <= 0 || cfg->hidden_size % 128 != 0 || cfg->hidden_size > 1280 ||
      cfg->intermediate_size <= 0 || cfg->intermediate_size % 128 != 0 || cfg->num_layers <= 0 || cfg->num_heads <= 0 ||
      cfg->hidden_size != 64 * cfg->num_heads || cfg->max_position_embeddings <= 0 || cfg->max_position_embeddings > 4096 ||
      cfg->dtype < 0 || cfg->dtype > 3 || cfg->projection_dim <= 0 || cfg->projection_dim % 32 != 0 ||
      (cfg->act != SDN_ACT_QUICK_GELU && cfg->act != SDN_ACT_GELU) || cfg->eos_token_id < 0 || cfg->hidden_tap < 1 ||
      cfg->hidden_tap > cfg->num_layers)
    return SDN_E_INVALID;
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  plain_chain_for_f32(u, cfg->dtype);
  u->pcfg = *cfg;
  u->ccfg.vocab_size = cfg->vocab_size; u->ccfg.hidden_size = cfg->hidden_size; u->ccfg.intermediate_size = cfg->intermediate_size;
  u->ccfg.num_layers = cfg->num_layers; u->ccfg.num_heads = cfg->num_heads; u->ccfg.max_position_embeddings = cfg->max_position_embeddings;
  u->ccfg.dtype = cfg->dtype;
  u->kind = CLIP_PROJ;
  get_plan(u, 1);
  *out = u;
  return SDN_OK;
}

int sdn_t5_create(const sdn_t5_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  if (cfg->vocab_size <= 0 || cfg->d_model <= 0 || cfg->d_model % 64 != 0 || cfg->d_kv != 64 || cfg->d_ff <= 0 || cfg->d_ff % 64 != 0 ||
      cfg->num_layers <= 0 || cfg->num_heads <= 0 || cfg->num_heads > 512 || cfg->num_buckets < 4 || cfg->num_buckets > 64 ||
      (cfg->num_buckets & 3) || cfg->max_distance <= cfg->num_buckets / 4 || !(cfg->eps > 0.f) || cfg->dtype < 0 || cfg->dtype > 1)
    return SDN_E_INVALID;                                       // (dtype 2 / 3, the fp32-storage modes, are not built yet)
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  u->tcfg = *cfg;
  u->kind = T5;
  get_plan(u, 1);                                               // registers the parameter manifest (independent of batch and n)
  *out = u;
  return SDN_OK;
}

int sdn_unet_prepare(sdn_unet* u, void* weights, void* stream) {
  if (!u || !weights) return SDN_E_INVALID;
  char* W = (char*)weights;
  const int dt = u->dtype() == 1 ? 1 : 0;
  for (const auto& j : u->fold_jobs) {
    if (j.kind == 2) {
      const int rc2 = sdn_expand3_weights((const float*)(W + j.w), j.rows, j.cols, j.group, W + j.wf, stream);
      if (rc2 != SDN_OK) return rc2;
      continue;
    }
    if (j.kind == 3) {
      const int rc3 = sdn_conv_up4_weights(dt, W + j.w, j.rows, j.cols, W + j.wf, stream);
      if (rc3 != SDN_OK) return rc3;
      continue;
    }
    if (j.kind == 1) {
      const int rc1 = sdn_linear_pair_fold(dt, W + j.w, W + j.gamma, (const float*)(W + j.beta), (const float*)(W + j.bias), j.rows, j.cols,
                                           W + j.wf, (float*)(W + j.c), stream);
      if (rc1 != SDN_OK) return rc1;
      continue;
    }
    const int rc = sdn_ln_fold(dt, W + j.w, (const float*)(W + j.gamma), (const float*)(W + j.beta),
                               j.bias >= 0 ? (const float*)(W + j.bias) : nullptr, j.rows, j.cols, W + j.wf, (float*)(W + j.c),
                               (float*)(W + j.d), stream);
    if (rc != SDN_OK) return rc;
  }
  return SDN_OK;
}

void sdn_unet_destroy(sdn_unet* u) { delete u; }

int sdn_unet_param_count(const sdn_unet* u) { return u ? (int)u->params.size() : 0; }

int sdn_unet_param_info(const sdn_unet* u, int32_t index, sdn_param_info* info) {
  if (!u || !info || index < 0 || index >= (int)u->params.size()) return SDN_E_INVALID;
  *info = u->params[index];
  return SDN_OK;
}

size_t sdn_unet_weight_bytes(const sdn_unet* u) { return u ? (size_t)u->weight_bytes : 0; }

// Images one plan invocation of a VAE takes: byte offsets inside one activation are 32-bit in the GEMM's DMA descriptors, so the
// largest tensor (batch x side^2 x widest channel count x 2 B) must stay below 4 GiB; larger batches are cut into chunks INSIDE
// the entry points (each chunk replays the same plan on the same workspace, stream-ordered).
//
// fp32-storage plans (dtype 2 / 3), what their kernels do with an offset (sdn_f32.hip, sdn_vae.hip):
//   k_gemm_f32       A rows `(long)am * ld`, conv taps `(((long)pb * Hs + sy) * Ws + sx) * Cin`, weights `(long)wn * K`, outputs
//                    `(long)m * ldc` and, NCHW, `((long)b * n_valid + n) * rows_per_batch + p`: 64-bit ELEMENT offsets on a float*;
//   k_gemm_x3        both A-gather paths: plain `abase[i] * ld + kk` with `long abase, ld`; conv `abase[i] + ((long)sy * Ws + sx) *
//                    Cin + c0` with `abase = (long)pb * Hs * Ws * Cin + 4 sc`; weights `long wbase`: 64-bit as well;
//   k_gn_rows_*      `((long)b * hw) * c1 + c`, `(long)r * ld`, `row * C` with `long row`: 64-bit;
//   k_conv_in_f32*   `long pix`, `(((long)b * cin + c) * H + iy) * W + ix`: 64-bit;
//   k_latent_mix, k_softmax_rows_f32, k_transpose32: `long` products of a row index and a leading dimension.
// What is 32-bit and signed in them are INDICES, not offsets: the output row `m` / `am` (< M = batch x side^2), the pixel index
// within an image, `hw`, and the grid size.  batch x side^2 < 2^31 holds for thousands of images, so no kernel of these modes
// forces a limit near the 16-bit plans'.  The limit is therefore chosen, from two things:
//   * the workspace: the 16-bit plans stop at 8 images; at 4 bytes per element the same budget is 4;
//   * a margin against an offset this reading missed: every activation of a chunk stays below 2^31 BYTES (the signed 32-bit
//     range, not the unsigned one of the 16-bit rule), so even a byte offset held in an `int` would still be in range.
// The largest activation is taken level by level, not as side^2 x the widest channel count (the 16-bit rule's over-estimate, kept
// as it is for those plans): at the resolution of block_out_channels[j] a map has that many channels, or the next level's behind
// the decoder's upsampler.  SD-v1.4 at 512 x 512: the 256-channel map behind up_blocks.2's upsampler, 268 MB per image; 8 images
// are 2^31 bytes, 7 fit, and the workspace rule makes it 4.  1024 x 1024: 1 GiB per image, one image per chunk.
static int vae_chunk(const sdn_unet* v) {
  const sdn_vae_config& c = v->vcfg;
  const int64_t side = (int64_t)c.sample_size << (c.n_levels - 1);
  if (c.dtype >= 2) {
    int64_t largest = 0;
    for (int j = 0; j < c.n_levels; ++j) {
      const int64_t s = side >> j, ch = std::max(c.block_out_channels[j], c.block_out_channels[j + 1 < c.n_levels ? j + 1 : j]);
      largest = std::max(largest, s * s * ch * 4);
    }
    const int64_t cap = std::min<int64_t>(4, (((int64_t)1 << 31) - 1) / largest);
    return cap < 1 ? 0 : (int)cap;
  }
  int64_t cmax = 0;
  for (int i = 0; i < c.n_levels; ++i) if (c.block_out_channels[i] > cmax) cmax = c.block_out_channels[i];
  int64_t cap = (((int64_t)1 << 32) - 1) / (side * side * cmax * 2);
  if (cap > 8) cap = 8;                                            // (beyond 8 images the kernels are saturated; bounds the workspace)
  return cap < 1 ? 0 : (int)cap;
}

size_t sdn_unet_workspace_bytes(sdn_unet* u, int32_t batch) {
  if (!u || batch <= 0) return 0;
  if (u->kind == T5) return sdn_t5_workspace_bytes(u, batch, 512);      // the sequence length is a call-time argument: the bound for any n
  if (u->is_vae()) {                                               // VAE entry points run large batches in chunks of vae_chunk()
    const int cap = vae_chunk(u);
    if (cap == 0) return 0;
    if (batch > cap) batch = cap;
  }
  const int64_t b = get_plan(u, batch)->ws_bytes;
  return b < 0 ? 0 : (size_t)b;
}

double sdn_unet_flops(sdn_unet* u, int32_t batch, double* attn) {
  if (!u || batch <= 0) return 0.0;
  Plan* p = get_plan(u, batch);
  if (attn) *attn = p->attn_flops;
  return p->flops;
}

// Runs a VAE plan over `batch` images in chunks of vae_chunk(): in / out advance by in_n / out_n floats per image.
static int vae_run(sdn_unet* v, Call call, const float* in, int64_t in_n, float* out, int64_t out_n, int32_t batch) {
  if (batch < 0 || (batch > 0 && (!in || !out))) return SDN_E_INVALID;
  const int cap = vae_chunk(v);
  if (cap == 0) return SDN_E_INVALID;                              // a single image already exceeds the 32-bit offsets
  for (int lo = 0; lo < batch; lo += cap) {
    call.batch = batch - lo < cap ? batch - lo : cap;
    call.in = in + lo * in_n; call.out = out + lo * out_n;
    const int rc = run_plan(v, call);
    if (rc != SDN_OK) return rc;
  }
  return SDN_OK;
}

int sdn_vae_decode(sdn_unet* v, const void* weights, const float* latents, float latent_scale, float* image, int32_t batch,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!v || v->kind != VAE_DECODER) return SDN_E_INVALID;
  const sdn_vae_config& c = v->vcfg;
  const int64_t side = (int64_t)c.sample_size << (c.n_levels - 1);
  Call call(weights, workspace, workspace_bytes, 0, stream);
  call.scalar = latent_scale;
  return vae_run(v, call, latents, (int64_t)c.latent_channels * c.sample_size * c.sample_size, image, (int64_t)c.out_channels * side * side, batch);
}

int sdn_vae_encode(sdn_unet* v, const void* weights, const float* image, float* moments, int32_t batch, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (!v || v->kind != VAE_ENCODER) return SDN_E_INVALID;
  const sdn_vae_config& c = v->vcfg;
  const int64_t side = (int64_t)c.sample_size << (c.n_levels - 1);
  return vae_run(v, Call(weights, workspace, workspace_bytes, 0, stream), image, (int64_t)c.out_channels * side * side, moments,
                 (int64_t)2 * c.latent_channels * c.sample_size * c.sample_size, batch);
}

int sdn_clip_forward(sdn_unet* m, const void* weights, const int32_t* input_ids, const int32_t* attention_mask,
                     void* last_hidden_state, int32_t batch, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || m->kind != CLIP || !input_ids || !last_hidden_state) return SDN_E_INVALID;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = input_ids; call.mask = attention_mask; call.out = last_hidden_state;
  return run_plan(m, call);
}

int sdn_clip_proj_forward(sdn_unet* m, const void* weights, const int32_t* input_ids, void* hidden, int64_t hidden_batch_stride,
                          int64_t hidden_row_stride, void* text_embeds, int64_t embeds_row_stride, int32_t batch, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (!m || m->kind != CLIP_PROJ || !input_ids || !hidden || !text_embeds) return SDN_E_INVALID;
  const sdn_clip_proj_config& c = m->pcfg;
  if (hidden_row_stride < c.hidden_size || hidden_batch_stride < (int64_t)c.max_position_embeddings * hidden_row_stride ||
      embeds_row_stride < c.projection_dim || embeds_row_stride > 0x7fffffff || (hidden_row_stride & 7) || (hidden_batch_stride & 7) ||
      (embeds_row_stride & 7) || (reinterpret_cast<uintptr_t>(hidden) & 15) || (reinterpret_cast<uintptr_t>(text_embeds) & 15))
    return SDN_E_INVALID;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = input_ids; call.out = hidden; call.out2 = text_embeds;
  call.out_bs = hidden_batch_stride; call.out_rs = hidden_row_stride; call.out2_rs = embeds_row_stride;
  return run_plan(m, call);
}

size_t sdn_t5_workspace_bytes(sdn_unet* m, int32_t batch, int32_t n) {
  if (!m || m->kind != T5 || batch <= 0 || batch > (1 << 20) || n < 2 || n > 512) return 0;
  const int64_t b = get_plan(m, batch, n)->ws_bytes;
  return b < 0 ? 0 : (size_t)b;
}

double sdn_t5_flops(sdn_unet* m, int32_t batch, int32_t n, double* attn) {
  if (!m || m->kind != T5 || batch <= 0 || batch > (1 << 20) || n < 2 || n > 512) return 0.0;
  Plan* p = get_plan(m, batch, n);
  if (attn) *attn = p->attn_flops;
  return p->flops;
}

int sdn_t5_forward(sdn_unet* m, const void* weights, const int32_t* input_ids, const int32_t* attention_mask, int32_t n,
                   void* out, int32_t batch, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || m->kind != T5 || n < 2 || n > 512 || batch > (1 << 20) || !input_ids || !out) return SDN_E_INVALID;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = input_ids; call.mask = attention_mask; call.n = n; call.out = out;
  return run_plan(m, call);
}

int sdn_unet_forward(sdn_unet* u, const void* weights, const float* latents, float timestep, const void* text,
                     float* out, int32_t batch, void* workspace, size_t workspace_bytes, void* stream) {
  if (!u || u->kind != UNET || !latents || !text || !out) return SDN_E_INVALID;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = latents; call.scalar = timestep; call.text = text; call.out = out;
  return run_plan(u, call);
}

int sdn_mmdit_forward(sdn_unet* u, const void* weights, const float* latents, float timestep, const void* text,
                      const void* pooled, float* out, int32_t batch, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (!u || u->kind != MMDIT || !latents || !text || !pooled || !out) return SDN_E_INVALID;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = latents; call.scalar = timestep; call.text = text; call.pooled = pooled; call.out = out;
  return run_plan(u, call);
}

void sdn_unet_set_text_version(sdn_unet* u, uint64_t version) {
  if (!u) return;
  u->text_version = version;
  if (version == 0) u->kv_version = 0;                         // undeclared: the cached K / V are dropped NOW, not at the next plain forward
}

void sdn_unet_profile_next(sdn_unet* u) { if (u) u->profile_next = true; }

void sdn_unet_set_split_k(sdn_unet* u, int32_t on) {
  if (!u || u->kind == T5 || u->kind == CLIP_PROJ || u->kind == CLIP_VISION || u->split_k == (on != 0)) return;   // (the T5 plan's GEMMs add into an f32 stream, the projected CLIP's
                                                                                       // erf-GELU is a lean epilogue only: no split-K form)
  if (u->dtype() >= 2) return;                                 // fp32-storage modes have no split-K form
  set_plan_toggle(u, &sdn_unet::split_k, on != 0);             // plans are rebuilt with / without partial buffers
}

void sdn_unet_set_conv_up4(sdn_unet* u, int32_t on) {
  if (!u || u->kind != UNET || u->dtype() >= 2 || u->conv_up4 == (on != 0)) return;   // (only the 16-bit UNet plans have the form)
  set_plan_toggle(u, &sdn_unet::conv_up4, on != 0);            // the derived regions stay registered: the manifest does not change
}

void sdn_unet_set_graph_mode(sdn_unet* u, int32_t on) {
  if (!u) return;
  u->use_graph = on != 0;
  if (!on) drop_graphs(u);
}

// ---- undeclared debug / A-B hooks (tools/ and tests): each sets one planner toggle and rebuilds the plans ----

// dtype-3 plans on the f32-staging k_gemm_x3 everywhere (0) or with triple operands on the LDS-DMA tiles (1, default).
// The expanded weight regions stay registered either way (the manifest does not change); query the workspace size again.
void sdn_debug_set_x3_expand(sdn_unet* u, int on) { if (u && u->x3_expand != (on != 0)) set_plan_toggle(u, &sdn_unet::x3_expand, on != 0); }

void sdn_debug_set_res_pre(sdn_unet* u, int on) { if (u && u->res_pre != (on != 0)) set_plan_toggle(u, &sdn_unet::res_pre, on != 0); }

// the K = 320 linears of the C = 320 transformer blocks on k_gemm_k320 (1, default) or on k_gemm_dma (0): A/B and equality tests
void sdn_debug_set_gemm_k320(sdn_unet* u, int on) { if (u && u->gemm_k320 != (on != 0)) set_plan_toggle(u, &sdn_unet::gemm_k320, on != 0); }

// run the BasicTransformerBlock LayerNorms as separate kernels again (the derived regions stay)
void sdn_debug_set_ln_fold(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::ln_fold, on != 0); }

void sdn_debug_set_ln_prepass_all(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::ln_prepass_all, on); }

// one-launch GEGLU feed-forward (C = 320) on / off: A/B and equality tests
void sdn_debug_set_ffn_fuse(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::ffn_fuse, on != 0); }

void sdn_debug_set_ff_fuse(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::ff_fuse, on != 0); }

void sdn_debug_set_ffn_own_stats(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::ffn_own_stats, on != 0); }

void sdn_debug_set_x3_pairs(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::x3_pairs, on != 0); }

void sdn_debug_set_gn_fuse(sdn_unet* u, int on) { if (u) set_plan_toggle(u, &sdn_unet::gn_fuse, on != 0); }

// size threshold of the transformer sub-batching (tools/)
void sdn_debug_set_subbatch_bytes(sdn_unet* u, long long bytes) {
  if (u && u->kind != MMDIT) set_plan_toggle(u, &sdn_unet::subbatch_bytes, (int64_t)bytes);
}

}  // extern "C"
