// Launch planner, shared part: the parameter manifest and activation arena behind Builder, the bf16x3 operand-expansion helpers,
// the op emitters more than one model uses (GEMM, conv3x3, GroupNorm, LayerNorm, repeat, attention), and get_plan(), which builds
// and caches one plan per batch size.
#include <math.h>

#include "sdn_plan.h"

namespace sdn_plan {

// ---- parameters -------------------------------------------------------------------------------
Ref Builder::param(const std::string& name, int kind, int rows, int cols, int rows_padded) {
  auto it = u->param_index.find(name);
  if (it != u->param_index.end()) return Ref{SP_W, u->params[it->second].offset};
  sdn_param_info pi;
  memset(&pi, 0, sizeof(pi));
  snprintf(pi.name, sizeof(pi.name), "%s", name.c_str());
  pi.kind = kind; pi.rows = rows; pi.cols = cols; pi.rows_padded = rows_padded > rows ? rows_padded : rows;
  const int64_t esz = (kind == SDN_P_VEC_F32 || kind == SDN_P_GEGLU_VEC) ? 4 : es;
  const int64_t bytes = (int64_t)pi.rows_padded * (cols > 0 ? cols : 1) * esz;
  pi.offset = u->weight_bytes;
  u->weight_bytes += (bytes + 255) & ~(int64_t)255;
  u->param_index[name] = (int)u->params.size();
  u->params.push_back(pi);
  return Ref{SP_W, pi.offset};
}
// members {name, rows} of a stacked matrix [sum rows, cols] (cols = 0: of a stacked f32 vector) must be byte-contiguous: their sizes
// are multiples of 256 B for every SD width
Ref Builder::stacked(const std::vector<std::pair<std::string, int>>& members, int cols) {
  Ref first;
  int64_t expect = -1;
  for (size_t i = 0; i < members.size(); ++i) {
    const int rows = members[i].second;
    Ref r = cols ? param(members[i].first, SDN_P_MAT, rows, cols) : param(members[i].first, SDN_P_VEC_F32, rows, 0);
    if (i == 0) first = r;
    else if (r.off != expect) { fprintf(stderr, "libsdn: stacked parameter %s is not contiguous\n", members[i].first.c_str()); abort(); }
    expect = r.off + (cols ? (int64_t)rows * cols * es : (int64_t)rows * 4);
  }
  return first;
}
Ref Builder::stacked(const std::vector<std::string>& names, int rows_each, int cols) {
  std::vector<std::pair<std::string, int>> members;
  for (const std::string& n : names) members.push_back({n, rows_each});
  return stacked(members, cols);
}
Ref Builder::derived(const std::string& name, int64_t bytes) {
  auto it = u->param_index.find(name);
  if (it != u->param_index.end()) return Ref{SP_W, u->params[it->second].offset};
  sdn_param_info pi; memset(&pi, 0, sizeof(pi));
  snprintf(pi.name, sizeof(pi.name), "%s", name.c_str());
  pi.kind = SDN_P_DERIVED; pi.rows = (int)bytes; pi.cols = 0; pi.rows_padded = (int)bytes;
  pi.offset = u->weight_bytes;
  u->weight_bytes += (bytes + 255) & ~(int64_t)255;
  u->param_index[name] = (int)u->params.size();
  u->params.push_back(pi);
  return Ref{SP_W, pi.offset};
}
// The derived regions (name, bytes) one fold job writes -- its wf, c and d, in that order, as many as are given -- and, the first
// time they are registered, the job itself (the rest of `job` is the caller's).
std::vector<Ref> Builder::derived_job(const std::vector<std::pair<std::string, int64_t>>& regions, sdn_unet::FoldJob job) {
  const bool fresh = u->param_index.find(regions[0].first) == u->param_index.end();
  std::vector<Ref> r;
  for (const auto& g : regions) r.push_back(derived(g.first, g.second));
  if (fresh) {
    job.wf = r[0].off;
    if (r.size() > 1) job.c = r[1].off;
    if (r.size() > 2) job.d = r[2].off;
    u->fold_jobs.push_back(job);
  }
  return r;
}

// ---- activations ------------------------------------------------------------------------------
Act Builder::act(int64_t rows, int C, int hw, int side, int esz) {
  const bool dflt = esz == 0;
  if (esz == 0) esz = es;
  Act t; t.content = rows * C * esz;
  t.bytes = (x3t && dflt) ? rows * C * 6 : t.content;      // a default-typed slot may hold the f32 tensor or its triple
  t.off = arena.alloc(t.bytes); t.C = C; t.hw = hw; t.side = side; return t;
}
// an activation a GroupNorm will read: its producer (a GEMM) also emits per-128-row-block column sums
Act Builder::act_gn(int64_t rows, int C, int hw, int side) {
  Act t = act(rows, C, hw, side);
  if (u->gn_fuse && !u->split_k && hw > 0 && hw % 128 == 0) {
    t.st_bytes = ((rows + 127) / 128) * (int64_t)C * 8;
    t.st_off = arena.alloc(t.st_bytes);
  }
  return t;
}
void Builder::drop(Act& t) {
  if (t.off >= 0) { arena.release(t.off, t.bytes); tri.erase(t.off); pairs.erase(t.off); }
  if (t.st_off >= 0) arena.release(t.st_off, t.st_bytes);
  t.off = -1; t.st_off = -1;
}

// ---- bf16x3 by operand expansion (include/sdn.h) -------------------------------------------------
// expanded copy of an f32 weight region [rows, cols] (stacked matrices are contiguous, so w.off names the whole operand)
Ref Builder::x3_weight(Ref w, int rows, int cols, int group) {
  return derived_job({{"x3@" + std::to_string((long long)w.off), (int64_t)rows * 3 * cols * 2}}, {w.off, -1, -1, -1, -1, -1, -1, rows, cols, 2, group})[0];
}
// the triple of an f32 tensor that no producer could write in that form (a raw residual-stream tensor, a skip concatenation)
Act Builder::split3(Ref a, Ref a2, int64_t rows, int c1, int c2, int hw, int side) {
  Act t = act(rows, c1 + c2, hw, side);
  Op o; o.kind = OP_SPLIT3; o.a = a; o.a2 = a2; o.rows = rows; o.c1 = c1; o.c2 = c2; o.out = R(t);
  o.bytes = 10.0 * (double)rows * (c1 + c2);
  snprintf(o.label, sizeof(o.label), "k_split3");
  emit(o);
  tri.insert(t.off);
  return t;
}

// ---- op emitters ------------------------------------------------------------------------------
// Every op of a plan is appended here.  attn: a GEMM that is part of an attention (the attention kinds count themselves).
void Builder::emit(Op& o, bool attn) {
  plan->ops.push_back(o);
  plan->flops += o.flops;
  if (attn || o.kind == OP_ATTN || o.kind == OP_MATTN || o.kind == OP_BATTN) plan->attn_flops += o.flops;
}
// The UNet's, VAE's and CLIP towers' GEMM: 16-bit bytes, the residual read charged; the bf16x3 plan's operand-expansion form.
void Builder::gemm(const GemmSpec& s) {
  if (s.rowgate.space != SP_NONE || s.residual_bcast || s.f32_stream) plan_bad = true;      // gemm_ex's and t5_gemm's
  const int64_t M = s.M; const int N = s.N, K = s.K, act_ = s.act;
  const Ref& residual = s.residual;
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.text_kv = s.text_kv; o.dyn_ldc = s.dyn_ldc;
  o.gd.M = (int)M; o.gd.N = N; o.gd.a_mode = SDN_A_PLAIN; o.gd.act = act_; o.gd.rows_per_batch = s.rows_per_batch; o.gd.ld_rowbias = s.ld_row;
  o.bias = s.bias; o.rowbias = s.rowbias; o.residual = residual; o.out = s.out;
  if ((x3t_on(s.a) || (s.force_x3t && x3t && !x3t_hold)) && (act_ == SDN_ACT_NONE || act_ == SDN_ACT_GEGLU) &&
      s.out_kind != SDN_OUT_F32_NCHW && s.n_valid == 0) {
    // A' = [hi | lo | hi] (written by the producing GroupNorm / LayerNorm / attention / GEGLU epilogue, or by a split pass),
    // W' = [hi | hi | lo]: one bf16 GEMM with three times the k loop; F32 residual, F32 (or, for GEGLU, triple) output.
    // (fp32 storage: no res_pre; never on sdn_gemm_k320)
    const bool two = s.a2.space != SP_NONE;
    Act tmp; Ref au = s.a;
    if (s.a.space != SP_WS || !tri.count(s.a.off)) { tmp = split3(s.a, s.a2, M, two ? s.K1 : K, two ? K - s.K1 : 0); au = R(tmp); }
    o.x3t = 1; o.gd.K = 3 * K; o.gd.out_kind = SDN_OUT_F32;
    const bool tri_o = s.triple_out && act_ == SDN_ACT_NONE;
    const bool pair_o = s.pair_out && act_ == SDN_ACT_NONE && !tri_o && residual.space == SP_NONE;
    o.gd.x3_out = act_ == SDN_ACT_GEGLU ? 2 : (tri_o ? 3 : (pair_o ? 4 : 1));
    if (pair_o && s.out.space == SP_WS) pairs.insert(s.out.off);
    o.a = au; o.w = x3_weight(s.w, N, K, K);
    o.flops = 2.0 * (double)M * (double)N * (double)K;
    o.bytes = 6.0 * ((double)M * K + (double)N * K) + 4.0 * (double)M * (act_ == SDN_ACT_GEGLU ? 0.75 * N : N) +
              (residual.space != SP_NONE ? 4.0 * (double)M * N : 0.0);
    snprintf(o.label, sizeof(o.label), "k_gemm<%d>x3", sdn_gemm_pick_tile((int)M, N, 3 * K, act_));
    push_gemm(o, s.cols);
    if ((act_ == SDN_ACT_GEGLU || tri_o) && s.out.space == SP_WS) tri.insert(s.out.off);
    if (tmp.off >= 0) drop(tmp);                            // stream order: the next op may reuse it
    return;
  }
  if (s.triple_out || s.pair_out || s.force_x3t) plan_bad = true;                           // output forms of the branch above only
  const bool rp = s.res_pre && residual.space != SP_NONE && act_ == SDN_ACT_NONE && s.out_kind == SDN_OUT_BF16 && s.n_valid == 0 && es == 2;
  o.gd.res_pre = rp ? 1 : 0; o.gd.K = K; o.gd.K1 = s.K1; o.gd.out_kind = s.out_kind; o.gd.n_valid = s.n_valid;
  o.a = s.a; o.a2 = s.a2; o.w = s.w;
  o.flops = 2.0 * (double)M * (double)(s.n_valid > 0 ? s.n_valid : N) * (double)K;
  // algorithmic bytes: A + W + the output, + the residual operand when the epilogue adds one (it is read once, 16 bit)
  o.bytes = 2.0 * ((double)M * K + (double)N * K + (double)M * (act_ == SDN_ACT_GEGLU ? N / 2 : N)) +
            (residual.space != SP_NONE ? 2.0 * (double)M * N : 0.0);
  snprintf(o.label, sizeof(o.label), "k_gemm<%d>%s", sdn_gemm_pick_tile((int)M, N, K, act_, residual.space != SP_NONE && !rp), rp ? "/rp" : "");
  // the forms sdn_gemm_k320 takes: bias and a pre-added residual at most, whole-width 16-bit output, no column statistics
  if (s.k320 && !x3t && K == 320 && N % 320 == 0 && act_ == SDN_ACT_NONE && s.out_kind == SDN_OUT_BF16 && s.n_valid == 0 && s.a2.space == SP_NONE &&
      s.rowbias.space == SP_NONE && (residual.space == SP_NONE || rp) && s.cols.space == SP_NONE && !u->split_k &&
      (rp ? kK320Rp : kK320Plain)) {
    o.k320 = 1;
    snprintf(o.label, sizeof(o.label), "k_gemm_k320%s", rp ? "/rp" : "");
  }
  push_gemm(o, s.cols);
}
// Small-M / long-K GEMMs (one-prompt batches) run in split-K form: the partial buffer lives only for this op.
void Builder::push_gemm(Op& o, Ref cols) {
  o.col = cols;
  const int nv = o.gd.n_valid > 0 ? o.gd.n_valid : o.gd.N;
  const int split = (!u->split_k || nv != o.gd.N || (o.gd.a_mode == SDN_A_CONV3X3 && o.gd.upsample == 2)) ? 1
                    : sdn_gemm_pick_split(o.gd.M, o.gd.N, o.gd.K, o.gd.act, o.gd.out_kind);
  if (split > 1) {
    const int64_t bytes = (int64_t)split * o.gd.M * o.gd.N * 4;
    const int64_t off = arena.alloc(bytes);
    o.gd.split_k = split; o.aux = Ref{SP_WS, off}; o.rows = bytes;
    arena.release(off, bytes);                              // stream order: the next op may reuse it
    const size_t L = strlen(o.label);
    if (L + 3 < sizeof(o.label)) snprintf(o.label + L, sizeof(o.label) - L, "/s%d", split);
  }
  emit(o);
}
void Builder::conv3x3(const ConvSpec& s) {
  const Act& in = s.in;
  const int cout = s.cout, n_pad = s.n_pad, stride = s.stride, upsample = s.upsample, asym_pad = s.asym_pad;
  const Ref& residual = s.residual;
  const int Hi = upsample ? in.side * 2 : in.side;
  const int Ho = (Hi + (asym_pad ? 1 : 2) - 3) / stride + 1;
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.gd.M = B * Ho * Ho; o.gd.N = n_pad; o.gd.a_mode = SDN_A_CONV3X3;
  o.gd.Hs = in.side; o.gd.Ws = in.side; o.gd.Ho = Ho; o.gd.Wo = Ho; o.gd.stride = stride;
  o.gd.upsample = upsample; o.gd.asym_pad = asym_pad; o.gd.n_valid = s.n_valid; o.gd.rows_per_batch = Ho * Ho; o.gd.ld_rowbias = s.ld_row;
  o.bias = s.bias; o.rowbias = s.rowbias; o.residual = residual; o.out = s.out;
  if (x3t_on(R(in))) {
    // the same convolution over an input with 3 Cin channels per pixel ([hi | lo | hi]) and per-tap weights [hi | hi | lo]
    // (fp32 storage: no res_pre)
    Act tmp; Ref au = R(in);
    if (!tri.count(in.off)) { tmp = split3(R(in), Ref(), (int64_t)B * in.side * in.side, in.C, 0, in.hw, in.side); au = R(tmp); }
    o.x3t = 1;
    o.gd.K = 27 * in.C; o.gd.Cin = 3 * in.C;
    if (s.out_kind == SDN_OUT_F32_NCHW) { o.gd.out_kind = s.out_kind; o.gd.x3_out = 0; }     // conv_out: the general epilogue's NCHW f32 form
    else { o.gd.out_kind = SDN_OUT_F32; o.gd.x3_out = 1; }
    o.a = au; o.w = x3_weight(s.w, n_pad, 9 * in.C, in.C);
    o.flops = 2.0 * (double)o.gd.M * (double)cout * 9.0 * in.C;
    o.bytes = 6.0 * ((double)B * in.side * in.side * in.C + (double)n_pad * 9 * in.C) + 4.0 * (double)o.gd.M * cout +
              (residual.space != SP_NONE ? 4.0 * (double)o.gd.M * cout : 0.0);
    if (Ho == in.side && sdn_conv_slab_shape_ok(o.gd.M, n_pad, 3 * in.C, in.side, stride, upsample, asym_pad, SDN_OUT_BF16, s.n_valid) &&
        sdn_gemm_pick_tile(o.gd.M, n_pad, o.gd.K, SDN_ACT_NONE) == 10)
      snprintf(o.label, sizeof(o.label), "k_conv_slab<%d>/x3", in.side);
    else
      snprintf(o.label, sizeof(o.label), "k_gemm<%d>x3", sdn_gemm_pick_tile(o.gd.M, n_pad, o.gd.K, SDN_ACT_NONE));
    push_gemm(o, s.cols);
    if (tmp.off >= 0) drop(tmp);
    return;
  }
  o.gd.res_pre = (s.res_pre && residual.space != SP_NONE && s.out_kind == SDN_OUT_BF16 && s.n_valid == 0 && es == 2) ? 1 : 0;
  o.gd.K = 9 * in.C; o.gd.Cin = in.C; o.gd.out_kind = s.out_kind;
  o.a = R(in); o.w = s.w;
  o.flops = 2.0 * (double)o.gd.M * (double)cout * (double)o.gd.K;
  o.bytes = 2.0 * ((double)B * in.side * in.side * in.C + (double)n_pad * o.gd.K + (double)o.gd.M * cout) +
            (residual.space != SP_NONE ? 2.0 * (double)o.gd.M * cout : 0.0);      // + the residual map the epilogue adds
  // Upsampler of a 16-bit UNet plan whose shape qualifies (architecture only, never the batch): the phase form -- four 2x2 convs
  // over the stored map, K = 4 Cin, weights = the derived region finish_up4() registers.  o.flops stays the nine-tap (algorithmic)
  // count, so the per-launch TFLOP/s of these rows is above what the matrix pipe executed.  Never split-K (push_gemm).
  const int up4 = (upsample == 1 && u->kind == UNET && es == 2 && stride == 1 && !asym_pad && s.out_kind == SDN_OUT_BF16 && s.n_valid == 0 &&
                   n_pad == cout && residual.space == SP_NONE && s.rowbias.space == SP_NONE && s.w.space == SP_W)
                      ? sdn_conv_up4_tile(in.side, in.side, in.C, n_pad) : 0;
  if (up4) {
    up4_pending.push_back({u->conv_up4 ? (int64_t)plan->ops.size() : -1, s.w.off, n_pad, in.C});
    if (u->conv_up4) {
      o.gd.K = 4 * in.C; o.gd.upsample = 2; o.gd.res_pre = 0;
      o.bytes = 2.0 * ((double)B * in.side * in.side * in.C + 4.0 * n_pad * o.gd.K + (double)o.gd.M * cout);
      snprintf(o.label, sizeof(o.label), "k_conv_up4<%d>", up4);
      push_gemm(o, s.cols);
      return;
    }
  }
  if (Ho == in.side && sdn_conv_slab_shape_ok(o.gd.M, n_pad, in.C, in.side, stride, upsample, asym_pad, s.out_kind, s.n_valid) &&
      sdn_gemm_pick_tile(o.gd.M, n_pad, o.gd.K, SDN_ACT_NONE) == 10)
    snprintf(o.label, sizeof(o.label), "k_conv_slab<%d>", in.side);
  else
    snprintf(o.label, sizeof(o.label), "k_gemm<%d>", sdn_gemm_pick_tile(o.gd.M, n_pad, o.gd.K, SDN_ACT_NONE));
  push_gemm(o, s.cols);
}
// End of a build: the phase-weight regions of the qualifying upsamplers go behind every real parameter, in plan order.
void Builder::finish_up4() {
  for (const Up4& p : up4_pending) {
    Ref d = derived_job({{"up4@" + std::to_string((long long)p.w9), (int64_t)16 * p.N * p.Cin * 2}}, {p.w9, -1, -1, -1, -1, -1, -1, p.N, p.Cin, 3})[0];
    if (p.op >= 0) plan->ops[(size_t)p.op].w = d;
  }
  up4_pending.clear();
}
void Builder::groupnorm(const Act& x, const Act* x2, float eps, int silu, Ref gamma, Ref beta, const Act& out) {
  Op o; o.kind = OP_GN; o.a = R(x); if (x2) o.a2 = R(*x2);
  o.batch = B; o.hw = x.hw; o.c1 = x.C; o.c2 = x2 ? x2->C : 0; o.groups = u->cfg.norm_groups; o.eps = eps;
  o.silu = silu; o.w = gamma; o.bias = beta; o.out = R(out); o.aux = gn_stats;
  if (x3t) { o.tri_out = 1; tri.insert(out.off); }            // every GroupNorm of the UNet feeds a conv / linear
  if (x.st_off >= 0 && (!x2 || x2->st_off >= 0)) {             // statistics come with the inputs: apply pass only
    o.cols1 = Ref{SP_WS, x.st_off};
    if (x2) o.cols2 = Ref{SP_WS, x2->st_off};
  }
  o.bytes = 2.0 * (o.cols1.space != SP_NONE ? 2.0 : 3.0) * (double)B * x.hw * (o.c1 + o.c2);   // reads (stats?, apply) + one write
  snprintf(o.label, sizeof(o.label), o.cols1.space != SP_NONE ? "k_gn_apply" : "k_gn_stats+apply");
  emit(o);
}
void Builder::layernorm(const Act& x, Ref gamma, Ref beta, const Act& out) {
  Op o; o.kind = OP_LN; o.a = R(x); o.rows = (int64_t)B * x.hw; o.c1 = x.C; o.eps = 1e-5f; o.w = gamma; o.bias = beta;
  o.out = R(out);
  if (x3t) { o.tri_out = 1; tri.insert(out.off); }            // ... and every LayerNorm a projection
  o.bytes = 2.0 * 2.0 * (double)o.rows * x.C;
  snprintf(o.label, sizeof(o.label), "k_layernorm");
  emit(o);
}
void Builder::repeat(const Act& in, const Act& out, int rep) {          // out = cat([in] * rep) along the batch
  Op o; o.kind = OP_REPEAT; o.a = R(in); o.out = R(out); o.rows = in.content; o.c1 = rep;     // (stream tensors: never triples)
  o.bytes = (double)in.content * (1 + rep);
  snprintf(o.label, sizeof(o.label), "k_repeat");
  emit(o);
}
void Builder::attention(Ref q, Ref k, Ref v, Ref out, int nq, int nk, int C, int ldq, int ldk, int ldv, bool kv_pairs) {
  Op o; o.kind = OP_ATTN; o.a = q; o.k = k; o.v = v; o.out = out; o.batch = B; o.heads = u->cfg.n_heads;
  o.nq = nq; o.nk = nk; o.hd = C / u->cfg.n_heads; o.ldq = ldq; o.ldk = ldk; o.ldv = ldv; o.ldo = C;
  o.scale = 1.0f / sqrtf((float)o.hd);
  if (x3t && out.space == SP_WS) { o.tri_out = 1; tri.insert(out.off); }   // its only reader is the to_out projection
  if (q.space == SP_WS && pairs.count(q.off)) {               // 1: q / k / v = column blocks of ONE pair-row buffer (self-attention);
    o.pair_in = kv_pairs ? 2 : 1; pairs.erase(q.off);         // 2: q = [hi(C) | lo(C)], k / v = column blocks of the text projection's pair rows
  } else if (kv_pairs) {
    plan_bad = true;                                          // K / V were written as pairs but Q was not: refuse the plan (forward rejects it)
  }
  o.flops = 4.0 * (double)B * o.heads * (double)nq * (double)nk * (double)o.hd;
  o.bytes = 2.0 * (double)B * C * (2.0 * nq + 2.0 * nk);
  snprintf(o.label, sizeof(o.label), "k_attn<%d>", o.hd);
  emit(o);
}

Plan* get_plan(sdn_unet* u, int batch, int n) {
  if (u->kind == T5 && n == 0) n = 512;
  const int key = u->kind == T5 ? batch * 1024 + n : batch;
  auto it = u->plans.find(key);
  if (it != u->plans.end()) return &it->second;
  if (u->kind == T5 && u->plans.size() >= 64) {                      // ragged lengths: bounded cache (no forward is in flight on the host side)
    u->plans.clear();
    u->profiled_batch = 0;                                      // ... and a profiled forward's plan is gone with it: nothing left to read
  }
  Plan& p = u->plans[key];
  p.batch = batch;
  Builder b{u, &p};
  b.B = batch;
  b.seq = n;
  b.es = u->dtype() >= 2 ? 4 : 2;                               // fp32 storage: SD-v1.4 UNet, CLIP, MMDiT and VAE plans
  b.x3t = u->kind == UNET && u->dtype() == 3 && u->x3_expand;
  switch (u->kind) {
    case UNET: b.build(); break;
    case MMDIT: b.build_mmdit(); break;
    case VAE_DECODER: b.build_vae(); break;
    case VAE_ENCODER: b.build_vae_encoder(); break;
    case CLIP: case CLIP_PROJ: b.build_clip(); break;
    case T5: b.build_t5(); break;
    case CLIP_VISION: b.build_clip_vision(); break;
    case INCEPTION: b.build_inception(); break;
  }
  if (b.plan_bad) p.ws_bytes = -1;                              // every entry point rejects the plan
  return &p;
}

}  // namespace sdn_plan
