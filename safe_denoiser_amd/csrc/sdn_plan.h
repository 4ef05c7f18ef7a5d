// Shared declarations of the host-side launch planner (sdn_plan_*.hip): the op list and arena a plan is made of, the engine
// handle behind the C ABI's opaque `sdn_unet`, the plan builder, and the functions that cross translation units.  No kernels.
#pragma once
#include <stdio.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "sdn_common.h"
#include "sdn_ops.h"

namespace sdn_plan {

// which model a handle is: set once by its sdn_*_create, read by every entry point's guard and by get_plan
enum ModelKind { UNET, MMDIT, VAE_DECODER, VAE_ENCODER, CLIP, CLIP_PROJ, T5, CLIP_VISION, INCEPTION };

enum Space { SP_NONE = 0, SP_W = 1, SP_WS = 2, SP_IN = 3, SP_TEXT = 4, SP_OUT = 5, SP_POOLED = 6, SP_KV = 7, SP_OUT2 = 8 };
// SP_IN / SP_OUT / SP_OUT2: a Call's primary input and its two outputs; SP_KV: the workspace's persistent tail (text K / V slots: written by one op, read by one op, never recycled)
struct Ref { int space = SP_NONE; int64_t off = 0; };

// Everything one forward is given.  An entry point fills the operands its plan names and leaves the rest null; c(ref) is the address
// a plan-time Ref names in this call.
struct Call {
  const void* weights; void* workspace; size_t workspace_bytes; int32_t batch; void* stream;
  const void *in = nullptr, *text = nullptr, *pooled = nullptr;   // in: latents, token ids, pixels or image; pooled: MMDiT
  void *out = nullptr, *out2 = nullptr;     // out2: text_embeds / image_embeds; the vision tower's out is nullable (its copy is skipped)
  float scalar = 0.f; int n = 0;            // scalar: timestep, or a VAE decoder's latent_scale; n: T5 sequence length
  const int32_t* mask = nullptr;            // key-padding mask (nullable; CLIP and T5)
  int64_t out_bs = 0, out_rs = 0, out2_rs = 0;   // batch / row stride of out and row stride of out2 (elements), where the caller chooses them
  int64_t kv_base = 0;                      // not the caller's: run_plan's copy carries its plan's SP_KV base
  int in_h = 0, in_w = 0;                   // Inception tower: height / width of the caller's pixels (the resize op's source)
  Call(const void* w, void* ws, size_t ws_bytes, int32_t b, void* s) : weights(w), workspace(ws), workspace_bytes(ws_bytes), batch(b), stream(s) {}
  const char* operator()(const Ref& r) const {
    switch (r.space) {
      case SP_W: return (const char*)weights + r.off;
      case SP_WS: return (const char*)workspace + r.off;
      case SP_KV: return (const char*)workspace + kv_base + r.off;
      case SP_IN: return (const char*)in + r.off;
      case SP_TEXT: return (const char*)text + r.off;
      case SP_OUT: return (const char*)out + r.off;
      case SP_OUT2: return (const char*)out2 + r.off;
      case SP_POOLED: return (const char*)pooled + r.off;
      default: return nullptr;
    }
  }
};

enum OpKind { OP_TEMB, OP_CONV_IN, OP_GEMM, OP_GN, OP_LN, OP_ATTN, OP_PATCHIFY, OP_UNPATCHIFY, OP_LATENT_MIX, OP_SOFTMAX,
              OP_TRANSPOSE, OP_REPEAT = 12 /* 11 is unassigned: tests/golden/plan_digests.json pins the numbers */, OP_CLIP_EMBED, OP_MATTN,
              OP_ROWSTATS, OP_FFN, OP_SPLIT3,
              OP_RMSNORM, OP_EMBED, OP_T5_BIAS, OP_BATTN, OP_EOS_ROWS, OP_COPY_ROWS, OP_PATCH_ROWS, OP_VISION_EMBED, OP_CLASS_ROWS,
              OP_CONV_ROWS, OP_POOL3, OP_RESIZE, OP_SPATIAL_MEAN,
              OP_QK_RMSNORM /* a = the [q | k | v] rows (in place), w = wq, bias = wk, rows, heads, ldq = ld, eps */ };

struct Op {
  int kind;
  sdn_gemm_desc gd;
  Ref a, a2, w, bias, rowbias, rowgate, residual, out, aux;
  Ref q2, k2, v2, out2;      // joint attention: second token stream
  Ref col, cols1, cols2;     // GEMM: column partials to emit; GroupNorm: partials of its input(s) to reduce instead of reading
  Ref ln_c, ln_d, ln_stats;  // GEMM with LayerNorm folded in (sdn_gemm_ln_*); ln_stats unset = statistics inside the kernel
  int ln = 0;
  int text_kv = 0;           // cross-attention K / V projection of the TEXT operand: skipped while the caller's text version stands
  int x3t = 0;               // bf16x3 plan: this GEMM runs on sdn_gemm_bf16 over triple operands (gd holds the EXPANDED K / Cin)
  int pair_in = 0;           // bf16x3 plan: attention whose q / k / v are column blocks of ONE hi | lo pair-row buffer (sdn_attention_x3_pairs)
  int tri_out = 0;           // bf16x3 plan: GroupNorm / LayerNorm / attention write the bf16 hi|lo|hi triple a GEMM will read
  int dyn_ldc = 0;           // projected CLIP plan: the output's leading dimension is the call's out2_rs
  int k320 = 0;              // K = 320 linear of a C = 320 transformer block on its own kernel (sdn_gemm_k320) instead of sdn_gemm_* / sdn_gemm_ln_*
  int n1 = 0, mod = 0, ld_mod = 0, patch = 0;
  // GN / LN / conv_in / attention scalars
  int batch = 0, hw = 0, c1 = 0, c2 = 0, groups = 0, silu = 0;
  float eps = 0.f;
  int64_t rows = 0;
  int heads = 0, nq = 0, nk = 0, hd = 0, ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  float scale = 0.f;
  Ref k, v;
  int kh = 0, kw = 0, sh = 0, sw = 0, ph = 0, pw = 0;   // OP_CONV_ROWS: kernel, stride, padding (input map batch x hw x hw x c1, kpad = c2); OP_POOL3: sh = stride, ph = pad
  char label[24] = {0};      // kernel symbol this op launches (profiling rows are aggregated by it)
  double flops = 0.0;        // algorithmic FLOPs of this launch
  double bytes = 0.0;        // algorithmic HBM bytes of this launch (operands read once + result written once)
};

struct Arena {                      // plan-time first-fit allocator with coalescing; offsets are 256-B aligned
  std::map<int64_t, int64_t> free_;  // off -> size
  int64_t top = 0, peak = 0;
  static int64_t up(int64_t v) { return (v + 255) & ~(int64_t)255; }
  int64_t alloc(int64_t bytes) {
    bytes = up(bytes);
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second >= bytes) {
        const int64_t off = it->first, rest = it->second - bytes;
        free_.erase(it);
        if (rest > 0) free_[off + bytes] = rest;
        return off;
      }
    }
    // extend the top (merge with a free block that touches the top)
    if (!free_.empty()) {
      auto last = std::prev(free_.end());
      if (last->first + last->second == top) {
        const int64_t off = last->first;
        free_.erase(last);
        top = off + bytes;
        if (top > peak) peak = top;
        return off;
      }
    }
    const int64_t off = top;
    top += bytes;
    if (top > peak) peak = top;
    return off;
  }
  void release(int64_t off, int64_t bytes) {
    bytes = up(bytes);
    auto it = free_.emplace(off, bytes).first;
    auto nx = std::next(it);
    if (nx != free_.end() && it->first + it->second == nx->first) { it->second += nx->second; free_.erase(nx); }
    if (it != free_.begin()) {
      auto pv = std::prev(it);
      if (pv->first + pv->second == it->first) { pv->second += it->second; free_.erase(it); }
    }
  }
};

struct Act {                         // a bf16 [rows, C] activation living in the workspace
  int64_t off = -1, bytes = 0; int C = 0, hw = 0, side = 0;
  int64_t content = 0;               // bytes of the tensor in the plan's storage type (== bytes except in the bf16x3 plan, whose
                                     // slots are sized for the 6-byte-per-element triple form as well)
  int64_t st_off = -1, st_bytes = 0;   // column partials its producing GEMM leaves for the GroupNorm that reads it
};

struct Plan {
  int batch = 0;
  int64_t tscalar_off = -1;          // 256-byte workspace slot holding the step's timestep (graph mode)
  std::vector<Op> ops;
  int64_t ws_bytes = 0;
  int64_t kv_base = 0;               // byte offset of the persistent tail inside the workspace (= the recycled arena's peak)
  double flops = 0.0, attn_flops = 0.0;
};

}  // namespace sdn_plan

// The engine handle behind the C ABI's opaque `sdn_unet`: one model of `kind` with its config, parameter manifest, cached plans and
// captured graphs.  Only the config of its kind is live.
struct sdn_unet {
  sdn_plan::ModelKind kind = sdn_plan::UNET;   // set once by the creator
  sdn_unet_config cfg;                  // UNET; a VAE mirrors its norm_groups here (the shared GroupNorm emitter reads cfg.norm_groups)
  sdn_mmdit_config mcfg;
  sdn_mmdit_ext mext = {0, 0.f, 0};     // MMDIT: the SD-3.5 additions (sdn_mmdit_create_ex); all zero = the SD3 plan
  sdn_vae_config vcfg;
  sdn_clip_config ccfg;
  sdn_clip_proj_config pcfg;            // CLIP_PROJ: ccfg mirrors its encoder fields (same layers as CLIP)
  sdn_t5_config tcfg;
  sdn_clip_vision_config vis;           // CLIP_VISION
  sdn_inception_config icfg;            // INCEPTION
  std::vector<sdn_inception_conv> convs;   // INCEPTION: the trunk's convolutions in manifest order (sdn_inception_conv_info)
  std::vector<sdn_param_info> params;
  std::map<std::string, int> param_index;
  int64_t weight_bytes = 0;
  std::map<int, sdn_plan::Plan> plans;            // by batch (T5: by batch * 1024 + n)
  int tproj_total = 0;
  int64_t subbatch_bytes = 0;            // >0: run transformer blocks on batch slices of at most this many bytes per
                                         // activation.  Measured at B = 64 (tools/profile_ops.py, SUBBATCH=...): 48 MB
                                         // -> +5 %, 24 MB -> +10 % forward time, i.e. no cache-residency win -> OFF.
  bool profile_next = false;
  // graph mode (sdn_unet_set_graph_mode): one captured hipGraph per (batch, operand addresses); replays cost one launch
  bool use_graph = false;
  bool gn_fuse = true;                  // GroupNorm statistics from the producing GEMMs' column partials (hw % 128 == 0)
  bool ln_fold = true;                  // BasicTransformerBlock LayerNorms folded into their consumer GEMMs where it pays
  int ln_prepass_all = 0;               // debug A/B: 1 = every folded LayerNorm takes its row statistics from the pre-pass
  bool ff_fuse = true;                  // FeedForward's output linear and the block's proj_out (no nonlinearity between them)
  bool ffn_own_stats = true;            // k_ffn320 takes norm3's row statistics from its own operand fragments (no sdn_row_stats pass)
  bool ffn_fuse = true;                 // ... and the GEGLU projection in front of them: one launch, hidden activation in LDS (C = 320)
                                        // contracted into ONE GEMM over [ff | h3] with the product weight (sdn_linear_pair_fold)
  struct FoldJob { int64_t w, gamma, beta, bias, wf, c, d; int rows, cols; int kind = 0; int group = 0; };   // kind 0: LayerNorm fold; 1: linear pair; 2: bf16x3 weight expansion (sdn_expand3_weights); 3: upsampler phase weights (sdn_conv_up4_weights: rows = N, cols = Cin)
  std::vector<FoldJob> fold_jobs;       // what sdn_unet_prepare has to compute into the SDN_P_DERIVED regions
  // Cross-attention K / V of the text (16 projections per forward, M = batch x 77) depend on the text operand alone, which the
  // denoising loop changes a handful of times in 50 steps: their outputs live in never-recycled workspace slots and the launches
  // are skipped while the caller-declared text version (sdn_unet_set_text_version; 0 = undeclared) equals the one they were
  // computed for, on the same batch / weights / text / workspace addresses.  Same bits: the skipped launches would rewrite them.
  uint64_t text_version = 0, kv_version = 0;
  int kv_batch = 0;
  const void *kv_w = nullptr, *kv_text = nullptr, *kv_ws = nullptr;
  bool x3_pairs = true;                 // bf16x3 plan: self-attention on pre-split operands (qkv projection writes hi | lo pair rows)
  bool res_pre = true;                  // attention output projections: residual into the accumulators before the k loop (sdn_gemm_desc.res_pre)
  bool gemm_k320 = true;                // sdn_debug_set_gemm_k320: the K = 320 linears of the C = 320 transformer blocks (16-bit plans) on k_gemm_k320
  bool x3_expand = true;                // dtype 3: GEMM operands as bf16 triples on the LDS-DMA tiles (false: the f32-staging k_gemm_x3 everywhere)
  bool split_k = false;                 // sdn_unet_set_split_k: small-M GEMMs of the plan take the split-K form (off by
                                        // default: it changes fp32 summation order with the batch size, and batch rows are
                                        // otherwise bit-identical whatever the batch)
  bool conv_up4 = true;                 // sdn_unet_set_conv_up4: qualifying upsampler convs of the 16-bit UNet plans in phase form (K = 4 Cin);
                                        // the choice is a function of the architecture alone -- never of the batch
  struct GraphKey {
    int batch; const void *w, *lat, *text, *pooled, *out, *ws;
    bool operator<(const GraphKey& o) const {
      return std::tie(batch, w, lat, text, pooled, out, ws) < std::tie(o.batch, o.w, o.lat, o.text, o.pooled, o.out, o.ws);
    }
  };
  std::map<GraphKey, hipGraphExec_t> graphs;
  hipStream_t cap_stream = nullptr;     // capture happens here (the caller's stream may be the legacy null stream)
  ~sdn_unet() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto e : ev) (void)hipEventDestroy(e);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
  }
  std::vector<hipEvent_t> ev;          // 2 per op of the profiled forward
  int profiled_batch = 0;
  int profiled_n = 0;                  // T5: sequence length of the profiled forward
  // storage dtype of the live config: 0 bf16, 1 f16, 2 fp32, 3 fp32 storage with bf16x3 contractions
  int dtype() const {
    switch (kind) {
      case sdn_plan::MMDIT: return mcfg.dtype;
      case sdn_plan::VAE_DECODER: case sdn_plan::VAE_ENCODER: return vcfg.dtype;
      case sdn_plan::CLIP: return ccfg.dtype;
      case sdn_plan::CLIP_PROJ: return pcfg.dtype;
      case sdn_plan::T5: return tcfg.dtype;
      case sdn_plan::CLIP_VISION: return vis.dtype;
      case sdn_plan::INCEPTION: return icfg.dtype;
      default: return cfg.dtype;
    }
  }
  bool is_vae() const { return kind == sdn_plan::VAE_DECODER || kind == sdn_plan::VAE_ENCODER; }
  bool is_clip() const { return kind == sdn_plan::CLIP || kind == sdn_plan::CLIP_PROJ; }
};

namespace sdn_plan {

// Which forms of the K = 320 linears Builder::transformer_body puts on k_gemm_k320 (sdn_gemm_k320.hip): decided per variant from the
// measured table of DESIGN 10.20 -- a form that measures slower than k_gemm_dma stays there.
constexpr bool kK320Plain = true, kK320Ln = true, kK320Rp = true;

// What one GEMM of a plan is asked to do: the operands every GEMM has (constructor), and by name everything only some have.  The
// emitters (Builder::gemm, gemm_ex, t5_gemm, gemm_ln) take nothing else: no option reaches them from an earlier statement.  An option
// an emitter has no form for makes the plan bad (Builder::plan_bad); res_pre and k320 are requests the chosen form's conditions may decline.
struct GemmSpec {
  int64_t M; int N, K;
  Ref a, w, bias, out;
  Ref a2; int K1 = 0;                      // second source of A: columns [K1, K)
  Ref rowbias, rowgate; int rows_per_batch = 0, ld_row = 0;   // per-sample rows [B, ld_row] added to / multiplied into the result
  Ref residual; int residual_bcast = 0;    // 1 = residual is [rows_per_batch, N], shared by every sample
  int act = SDN_ACT_NONE, out_kind = SDN_OUT_BF16, n_valid = 0;
  Ref cols;                                // column partials to emit for the GroupNorm that reads `out` (Builder::stats_of)
  bool res_pre = false;                    // add the residual into the accumulators before the k loop (sdn_gemm_desc.res_pre) where the form allows
  bool k320 = false;                       // may go to sdn_gemm_k320 (the C = 320 projections of transformer_body)
  bool triple_out = false;                 // bf16x3 plan: write the triple of the result (its only reader is another x3 GEMM)
  bool pair_out = false;                   // bf16x3 plan: write hi | lo pair rows (its only reader is sdn_attention_x3_pairs)
  bool force_x3t = false;                  // bf16x3 plan: operand-expansion form although A is not a workspace tensor (text states)
  bool text_kv = false;                    // K / V projection of the TEXT operand (Op::text_kv)
  bool dyn_ldc = false;                    // the output's leading dimension is the call's out2_rs (Op::dyn_ldc)
  bool f32_stream = false;                 // out += A W^T on the F32 residual stream `out` (sdn_gemm_desc.f32_stream)
  GemmSpec(int64_t M_, int N_, int K_, Ref a_, Ref w_, Ref bias_, Ref out_) : M(M_), N(N_), K(K_), a(a_), w(w_), bias(bias_), out(out_) {}
  GemmSpec& with_a2(Ref v, int k1) { a2 = v; K1 = k1; return *this; }
  GemmSpec& with_rowbias(Ref v, int rpb, int ld) { rowbias = v; rows_per_batch = rpb; ld_row = ld; return *this; }
  GemmSpec& with_rowgate(Ref v, int rpb, int ld) { rowgate = v; rows_per_batch = rpb; ld_row = ld; return *this; }
  GemmSpec& with_residual(Ref v) { residual = v; return *this; }
  GemmSpec& with_residual_bcast(Ref v, int rpb) { residual = v; residual_bcast = 1; rows_per_batch = rpb; return *this; }
  GemmSpec& with_act(int v) { act = v; return *this; }
  GemmSpec& with_out_kind(int v) { out_kind = v; return *this; }
  GemmSpec& with_cols(Ref v) { cols = v; return *this; }
  GemmSpec& with_res_pre(bool v) { res_pre = v; return *this; }
  GemmSpec& with_k320(bool v) { k320 = v; return *this; }
  GemmSpec& with_triple_out(bool v) { triple_out = v; return *this; }
  GemmSpec& with_pair_out(bool v) { pair_out = v; return *this; }
  GemmSpec& with_force_x3t(bool v) { force_x3t = v; return *this; }
  GemmSpec& with_text_kv() { text_kv = true; return *this; }
  GemmSpec& with_dyn_ldc() { dyn_ldc = true; return *this; }
  GemmSpec& with_f32_stream(bool v) { f32_stream = v; return *this; }
};
// ... and one 3x3 convolution (Builder::conv3x3) of the map `in` to `cout` channels
struct ConvSpec {
  Act in; int cout, n_pad;                 // n_pad: rows of the (zero-padded) weight = the GEMM's N
  Ref w, bias, out;
  int stride = 1, upsample = 0, asym_pad = 0;
  Ref rowbias; int ld_row = 0;
  Ref residual;
  int out_kind = SDN_OUT_BF16, n_valid = 0;
  Ref cols;
  bool res_pre = false;
  ConvSpec(const Act& in_, int cout_, Ref w_, Ref bias_, Ref out_) : in(in_), cout(cout_), n_pad(cout_), w(w_), bias(bias_), out(out_) {}
  ConvSpec& with_stride(int v, int asym = 0) { stride = v; asym_pad = asym; return *this; }
  ConvSpec& with_upsample() { upsample = 1; return *this; }
  ConvSpec& with_rowbias(Ref v, int ld) { rowbias = v; ld_row = ld; return *this; }
  ConvSpec& with_residual(Ref v) { residual = v; return *this; }
  ConvSpec& with_nchw_out(int n_pad_) { out_kind = SDN_OUT_F32_NCHW; n_valid = cout; n_pad = n_pad_; return *this; }
  ConvSpec& with_cols(Ref v) { cols = v; return *this; }
  ConvSpec& with_res_pre(bool v) { res_pre = v; return *this; }
};

// Emits one plan: every method appends ops to `plan` and allocates / releases activations in `arena`.  The shared emitters live in
// sdn_plan_core.hip, the per-model blocks and build_*() in sdn_plan_unet / _mmdit / _vae / _text.hip.
struct Builder {
  sdn_unet* u;
  Plan* plan;
  Arena arena;
  int B;
  int seq = 0;               // T5 plans: the sequence length this plan is built for
  int es = 2;                // bytes per activation / matrix-weight element: 2 (bf16 | f16 storage) or 4 (the fp32 precision mode)
  bool x3t = false;          // bf16x3 by operand expansion (SD-v1.4 UNet plan, dtype 3): GEMM operands are bf16 hi|lo|hi triples
  bool x3t_hold = false;     // ... except inside this scope (the per-sample time-embedding GEMMs: M = batch, nothing to gain)
  std::set<int64_t> tri;     // workspace offsets that currently hold a triple (set by its producer, cleared by drop())
  Ref tproj;                 // f32 [B, tproj_total]
  int tproj_cursor = 0;      // column offset of the next resnet's slice
  Ref gn_stats;
  int64_t kv_top = 0;             // bytes of persistent text K / V slots handed out so far (space SP_KV)
  bool plan_bad = false;          // an emitter met an inconsistency, or a spec asked for what its emitter cannot do: get_plan() sets ws_bytes = -1
  std::set<int64_t> pairs;        // workspace offsets that hold pair rows
  // upsampler convs that qualify for the phase form: their derived weight regions are registered by finish_up4() AFTER every real
  // parameter (no existing manifest offset moves), which then fills in the `w` of the ops emitted in that form (op >= 0)
  struct Up4 { int64_t op; int64_t w9; int N, Cin; };
  std::vector<Up4> up4_pending;
  void finish_up4();
  struct Res { std::string pfx; int cout; };

  // ---- parameters, activations, bf16x3 helpers and shared op emitters (sdn_plan_core.hip) -----------
  Ref param(const std::string& name, int kind, int rows, int cols, int rows_padded = 0);
  Ref stacked(const std::vector<std::pair<std::string, int>>& members, int cols);   // {name, rows}; cols = 0: f32 vectors
  Ref stacked(const std::vector<std::string>& names, int rows_each, int cols);
  Ref derived(const std::string& name, int64_t bytes);
  Act act(int64_t rows, int C, int hw = 0, int side = 0, int esz = 0);
  Act act_gn(int64_t rows, int C, int hw, int side);
  static Ref stats_of(const Act& out) { return out.st_off >= 0 ? Ref{SP_WS, out.st_off} : Ref(); }   // a GemmSpec's / ConvSpec's `cols`
  void drop(Act& t);
  static Ref R(const Act& t) { return Ref{SP_WS, t.off}; }
  Ref x3_weight(Ref w, int rows, int cols, int group);
  Act split3(Ref a, Ref a2, int64_t rows, int c1, int c2, int hw = 0, int side = 0);
  bool x3t_on(const Ref& a) const { return x3t && !x3t_hold && a.space == SP_WS; }
  void emit(Op& o, bool attn = false);
  std::vector<Ref> derived_job(const std::vector<std::pair<std::string, int64_t>>& regions, sdn_unet::FoldJob job);
  void gemm(const GemmSpec& s);
  void push_gemm(Op& o, Ref cols);
  void conv3x3(const ConvSpec& s);
  void groupnorm(const Act& x, const Act* x2, float eps, int silu, Ref gamma, Ref beta, const Act& out);
  void layernorm(const Act& x, Ref gamma, Ref beta, const Act& out);
  void repeat(const Act& in, const Act& out, int rep);
  void attention(Ref q, Ref k, Ref v, Ref out, int nq, int nk, int C, int ldq, int ldk, int ldv, bool kv_pairs = false);

  // ---- SD-v1.4 UNet (sdn_plan_unet.hip) --------------------------------------------------------------
  std::vector<Ref> ln_fold_regions(const std::string& wname, Ref w, Ref gamma, Ref beta, Ref bias, int N, int K);
  void row_stats(Ref x, int64_t rows, int C, const Act& st);
  void gemm_ln(const GemmSpec& s, const std::string& wname, Ref gamma, Ref beta, bool prepass);
  Act resnet(const std::string& pfx, Act& x, Act* skip, int cout);
  Act transformer(const std::string& pfx, Act& x);
  void transformer_body(const std::string& pfx, Act& x, const Act& out, int64_t text_off, int rep = 1,
                        const Act* x_full = nullptr);
  std::vector<Res> enumerate_resnets() const;
  void build();

  // ---- SD-v3 MMDiT (sdn_plan_mmdit.hip) --------------------------------------------------------------
  void gemm_ex(const GemmSpec& s);
  void ln_mod(const Act& x, int64_t rows, int rows_per_batch, Ref scale, Ref shift, int ld, const Act& out);
  void qk_rmsnorm(const Act& qkv, int64_t rows, Ref wq, Ref wk);
  Ref fcol(int col) const { return Ref{SP_WS, tproj.off + (int64_t)col * 4}; }   // column of the stacked adaLN output
  void build_mmdit();

  // ---- AutoencoderKL decoder and encoder (sdn_plan_vae.hip) ------------------------------------------
  Act vae_resnet(const std::string& pfx, Act& x, int cout);
  Act vae_attention(const std::string& pfx, Act& x);
  void vae_f32_rows();       // fp32-storage plans: the kernel labels and 4-byte operand traffic of the finished op list
  void build_vae();
  void build_vae_encoder();

  // ---- CLIP (plain and projected) and T5 text encoders (sdn_plan_text.hip) ---------------------------
  void build_clip();
  Ref glu_pair(const std::string& value_name, const std::string& gate_name, int F, int K);
  void t5_gemm(const GemmSpec& s);
  void t5_rmsnorm(Ref x, bool x_f32, int64_t rows, int C, Ref w, Ref out);
  void build_t5();

  // ---- CLIP ViT vision tower with projection (sdn_plan_vision.hip) -----------------------------------
  void build_clip_vision();

  // ---- Inception-v3 pool3 tower (sdn_plan_inception.hip) ---------------------------------------------
  void inception_conv(const std::string& name, const Act& in, int cout, int kh, int kw, int stride, int ph, int pw, const Act& out,
                      int c0);
  Act inception_conv_new(const std::string& name, const Act& in, int cout, int kh = 1, int kw = 1, int stride = 1, int ph = 0, int pw = 0);
  void inception_pool(int mode, const Act& in, int stride, int pad, const Act& out, int c0);
  void build_inception();
};

// n: the sequence length of a T5 plan (ignored by every other plan); 0 = the longest one (512), which bounds the workspace of any n
Plan* get_plan(sdn_unet* u, int batch, int n = 0);
// checks what every kind needs (handle, weights, workspace, batch, plan, workspace size); an entry point rejects a null operand of its own plan first
int run_plan(sdn_unet* u, const Call& c);
void drop_graphs(sdn_unet* u);

}  // namespace sdn_plan
