// UNet2DConditionModel forward (row U1/U2) as a static launch plan over libsdn's operators.
//
// Host-only logic: from the config it derives (a) the parameter manifest -- every diffusers state_dict key the
// network needs, with the layout it takes inside ONE packed weight buffer -- and (b) per batch size, a linear
// list of kernel launches with all activation addresses resolved at plan time inside ONE workspace (liveness-
// based reuse so the hot working set stays L2 / Infinity-Cache resident).  sdn_unet_forward() then only walks
// the list and launches; it never allocates or synchronises (hipGraph-capturable).
//
// Wiring follows the reference's vendored spec: models/unet.py:683-932 (forward), models/unet_2d_blocks.py
// :769-924 (mid), :1174-1426 (down), :2416-2704 (up), models/transformer_2d.py:239-359,505-540,810-858, and the
// diffusers-0.29.0 leaf definitions restated in SURVEY.md appendix A.
//
// Fusions relative to the reference graph (results identical up to rounding):
//   * to_q/to_k/to_v of self-attention = one GEMM over the stacked [3C, C] weight; to_k/to_v of cross-attention
//     = one GEMM over [2C, 768];
//   * all 22 ResnetBlock2D time_emb_proj linears = ONE GEMM per forward ([B,1280] x [sum Cout, 1280]); its f32
//     rows are added inside conv1's epilogue together with the conv bias;
//   * SiLU(temb) folded into time_embedding.linear_2's epilogue (temb is only ever consumed through SiLU);
//   * residual adds, shortcut adds, GEGLU, bias: GEMM epilogues; torch.cat([h, skip]) is never materialised for
//     the 1x1 shortcut (two-source A operand) and is written once, already normalised, by GroupNorm for conv1;
//   * nearest-2x upsample and the stride-2 downsample are index arithmetic inside the conv's im2col loader;
//   * conv_out writes the fp32 NCHW latent layout directly.
//
// This file: the UNet's blocks (resnet, transformer, the LayerNorm-folded GEMM) and its build().  The types, the shared emitters
// and the other models' builders are in sdn_plan.h and the sdn_plan_*.hip files next to this one.
#include <math.h>

#include "sdn_plan.h"

namespace sdn_plan {

// LayerNorm(x; gamma, beta) -> GEMM(W, bias) with the norm folded into the GEMM (sdn_gemm_ln_*).  Registers the derived
// weight regions once; `prepass` = row statistics from a read-only pass instead of inside the kernel (wide N).
void Builder::gemm_ln(const Act& x, int64_t rows, int N, int K, const std::string& wname, Ref w, Ref gamma, Ref beta, Ref bias,
                      Ref out, int act_, bool prepass) {
  const bool fresh = u->param_index.find(wname + "#ln") == u->param_index.end();
  Ref wf = derived(wname + "#ln", (int64_t)N * K * 2), c = derived(wname + "#ln_c", (int64_t)N * 4), d = derived(wname + "#ln_d", (int64_t)N * 4);
  if (fresh) u->fold_jobs.push_back({w.off, gamma.off, beta.off, bias.space == SP_NONE ? -1 : bias.off, wf.off, c.off, d.off, N, K});
  Act st;
  if (prepass) {
    st = act(rows, 2, 0, 0, 4);
    Op o; o.kind = OP_ROWSTATS; o.a = R(x); o.rows = rows; o.c1 = K; o.eps = 1e-5f; o.out = R(st);
    o.bytes = 2.0 * rows * K; snprintf(o.label, sizeof(o.label), "k_row_stats"); plan->ops.push_back(o);
  }
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.gd.M = (int)rows; o.gd.N = N; o.gd.K = K; o.gd.a_mode = SDN_A_PLAIN; o.gd.act = act_; o.gd.out_kind = SDN_OUT_BF16;
  o.a = R(x); o.w = wf; o.out = out; o.ln = 1; o.ln_c = c; o.ln_d = d; o.eps = 1e-5f;
  if (prepass) o.ln_stats = R(st);
  o.flops = 2.0 * (double)rows * N * K;
  o.bytes = 2.0 * ((double)rows * K + (double)N * K + (double)rows * (act_ == SDN_ACT_GEGLU ? N / 2 : N));
  { int t = sdn_gemm_pick_tile((int)rows, N, K, act_);
    if (t == 8 && N % 320 == 0) t = 10;                        // (sdn_gemm_impl: the folded forms have no 256-wide instantiation)
    snprintf(o.label, sizeof(o.label), "k_gemm<%d>/ln%d", t, prepass ? 2 : 1); }   // /lnL: L = the symbol's LNF
  if (k320_next && !prepass && K == 320 && N % 320 == 0 && act_ == SDN_ACT_NONE && pending_cols.space == SP_NONE && kK320Ln) {
    o.k320 = 1;                                                // statistics from the fragments, as LNF = 1: sdn_gemm_k320
    snprintf(o.label, sizeof(o.label), "k_gemm_k320/ln1");
  }
  k320_next = false;
  plan->ops.push_back(o);
  plan->flops += o.flops;
  if (prepass) drop(st);
}

// ---- blocks --------------------------------------------------------------------------------------
// ResnetBlock2D: GN-SiLU-conv3x3(+temb) - GN-SiLU-conv3x3 + shortcut.  Input = x (++ skip).
Act Builder::resnet(const std::string& pfx, Act& x, Act* skip, int cout) {
  const int cin = x.C + (skip ? skip->C : 0);
  Ref n1g = param(pfx + ".norm1.weight", SDN_P_VEC_F32, cin, 0), n1b = param(pfx + ".norm1.bias", SDN_P_VEC_F32, cin, 0);
  Ref c1w = param(pfx + ".conv1.weight", SDN_P_CONV3X3, cout, 9 * cin), c1b = param(pfx + ".conv1.bias", SDN_P_VEC_F32, cout, 0);
  const int tcol = tproj_cursor; tproj_cursor += cout;       // time_emb_proj registered up-front (stacked)
  Ref n2g = param(pfx + ".norm2.weight", SDN_P_VEC_F32, cout, 0), n2b = param(pfx + ".norm2.bias", SDN_P_VEC_F32, cout, 0);
  Ref c2w = param(pfx + ".conv2.weight", SDN_P_CONV3X3, cout, 9 * cout), c2b = param(pfx + ".conv2.bias", SDN_P_VEC_F32, cout, 0);
  const int64_t rows = (int64_t)B * x.hw;
  Act g1 = act(rows, cin, x.hw, x.side);
  groupnorm(x, skip, 1e-5f, 1, n1g, n1b, g1);
  Act h = act_gn(rows, cout, x.hw, x.side);
  want_stats(h);
  conv3x3(g1, cout, cout, c1w, c1b, R(h), 1, 0, Ref(), Ref{SP_WS, tproj.off + (int64_t)tcol * 4}, u->tproj_total);
  drop(g1);
  Act g2 = act(rows, cout, x.hw, x.side);
  groupnorm(h, nullptr, 1e-5f, 1, n2g, n2b, g2);
  drop(h);
  Act out = act_gn(rows, cout, x.hw, x.side);
  if (cin != cout) {
    Ref scw = param(pfx + ".conv_shortcut.weight", SDN_P_MAT, cout, cin), scb = param(pfx + ".conv_shortcut.bias", SDN_P_VEC_F32, cout, 0);
    Act sc = act(rows, cout, x.hw, x.side);
    gemm(rows, cout, cin, R(x), scw, scb, R(sc), SDN_ACT_NONE, Ref(), SDN_OUT_BF16, 0, skip ? R(*skip) : Ref(),
         skip ? x.C : 0);
    want_stats(out);
    res_pre_next = u->res_pre;
    conv3x3(g2, cout, cout, c2w, c2b, R(out), 1, 0, R(sc), Ref(), 0);
    drop(sc);
  } else {
    want_stats(out);
    res_pre_next = u->res_pre;
    conv3x3(g2, cout, cout, c2w, c2b, R(out), 1, 0, R(x), Ref(), 0);
  }
  drop(g2);
  return out;
}

// Transformer2DModel (continuous) with one BasicTransformerBlock.
// Optional sub-batching of the transformer blocks (every op of a block is per-sample independent; results are
// bit-identical).  It was built to test whether slicing the 168 MB activations of the 64x64 level keeps the chain of
// short-K projections Infinity-Cache resident; it does not pay (see subbatch_bytes), so it is off by default.
Act Builder::transformer(const std::string& pfx, Act& x) {
  const int64_t bytes_full = (int64_t)B * x.hw * x.C * es;
  int nsub = 1;
  if (u->subbatch_bytes > 0)
    while (nsub < B && bytes_full / nsub > u->subbatch_bytes && B % (nsub * 2) == 0) nsub *= 2;
  Act out = nsub == 1 ? act_gn((int64_t)B * x.hw, x.C, x.hw, x.side) : act((int64_t)B * x.hw, x.C, x.hw, x.side);
  const int Bfull = B, Bs = B / nsub;
  for (int sb = 0; sb < nsub; ++sb) {
    B = Bs;
    Act xs = x, os = out;                                   // views: never dropped
    xs.off += (int64_t)sb * Bs * x.hw * x.C * es; os.off += (int64_t)sb * Bs * x.hw * x.C * es;
    transformer_body(pfx, xs, os, (int64_t)sb * Bs * u->cfg.text_len * u->cfg.cross_dim * es);
  }
  B = Bfull;
  return out;
}

// rep > 1 (sdn_unet_config.latent_repeat, first block only): `x` holds the B / rep samples the guidance branches share
// and `x_full` their repetition; everything up to the cross-attention's query is computed once and repeated.
void Builder::transformer_body(const std::string& pfx, Act& x, const Act& out, int64_t text_off, int rep,
                               const Act* x_full) {
  const int C = x.C, hw = x.hw, T = u->cfg.text_len, X = u->cfg.cross_dim;
  const int Bfull = B;
  B = Bfull / rep;
  int64_t rows = (int64_t)B * hw;
  const std::string tb = pfx + ".transformer_blocks.0";
  Ref ng = param(pfx + ".norm.weight", SDN_P_VEC_F32, C, 0), nb = param(pfx + ".norm.bias", SDN_P_VEC_F32, C, 0);
  Ref piw = param(pfx + ".proj_in.weight", SDN_P_MAT, C, C), pib = param(pfx + ".proj_in.bias", SDN_P_VEC_F32, C, 0);
  Ref l1g = param(tb + ".norm1.weight", SDN_P_VEC_F32, C, 0), l1b = param(tb + ".norm1.bias", SDN_P_VEC_F32, C, 0);
  Ref qkv = stacked({tb + ".attn1.to_q.weight", tb + ".attn1.to_k.weight", tb + ".attn1.to_v.weight"}, C, C);
  Ref o1w = param(tb + ".attn1.to_out.0.weight", SDN_P_MAT, C, C), o1b = param(tb + ".attn1.to_out.0.bias", SDN_P_VEC_F32, C, 0);
  Ref l2g = param(tb + ".norm2.weight", SDN_P_VEC_F32, C, 0), l2b = param(tb + ".norm2.bias", SDN_P_VEC_F32, C, 0);
  Ref q2w = param(tb + ".attn2.to_q.weight", SDN_P_MAT, C, C);
  Ref kv2 = stacked({tb + ".attn2.to_k.weight", tb + ".attn2.to_v.weight"}, C, X);
  Ref o2w = param(tb + ".attn2.to_out.0.weight", SDN_P_MAT, C, C), o2b = param(tb + ".attn2.to_out.0.bias", SDN_P_VEC_F32, C, 0);
  Ref l3g = param(tb + ".norm3.weight", SDN_P_VEC_F32, C, 0), l3b = param(tb + ".norm3.bias", SDN_P_VEC_F32, C, 0);
  Ref f1w = param(tb + ".ff.net.0.proj.weight", SDN_P_GEGLU_MAT, 8 * C, C), f1b = param(tb + ".ff.net.0.proj.bias", SDN_P_GEGLU_VEC, 8 * C, 0);
  Ref f2w = param(tb + ".ff.net.2.weight", SDN_P_MAT, C, 4 * C), f2b = param(tb + ".ff.net.2.bias", SDN_P_VEC_F32, C, 0);
  Ref pow_ = param(pfx + ".proj_out.weight", SDN_P_MAT, C, C), pob = param(pfx + ".proj_out.bias", SDN_P_VEC_F32, C, 0);

  Act gn = act(rows, C, hw, x.side);
  groupnorm(x, nullptr, 1e-6f, 0, ng, nb, gn);
  Act h = act(rows, C, hw, x.side);
  // the five K = 320 linears of a C = 320 block (16-bit plans, whole batch) run on k_gemm_k320: proj_in, qkv,
  // attn1.to_out, attn2.to_q, attn2.to_out -- same bits as the k_gemm_dma launches they replace
  const bool k320 = u->gemm_k320 && C == 320 && es == 2 && !x3t && u->subbatch_bytes == 0;
  k320_next = k320;
  gemm(rows, C, C, R(gn), piw, pib, R(h));
  drop(gn);
  // LayerNorm folding (gemm_ln): measured per shape (tools/bench_lnfold.py) -- it pays at C = 320 / 640 for the
  // attention projections (statistics inside the kernel while N <= 960, from a read-only pre-pass above) and at
  // C = 320 for the GEGLU projection; the wide, MFMA-bound projections of the lower levels keep the LayerNorm kernel.
  const bool fold12 = u->ln_fold && C <= 640, fold3 = u->ln_fold && C == 320;
  const int hdx = C / u->cfg.n_heads;
  const bool x3p_cross = x3t && u->x3_pairs && u->subbatch_bytes == 0 && (hdx == 40 || hdx == 80 || hdx == 160);   // sdn_attention_x3_pairs on the cross-attention too
  // self-attention
  Act ln;
  if (!fold12 || !fold3) ln = act(rows, C, hw, x.side);
  Act qkvb = act(rows, 3 * C, hw, x.side);
  k320_next = k320;
  if (fold12) {
    gemm_ln(h, rows, 3 * C, C, tb + ".attn1.to_q.weight", qkv, l1g, l1b, Ref(), R(qkvb), SDN_ACT_NONE, 3 * C > 960 || u->ln_prepass_all);
  } else {
    layernorm(h, l1g, l1b, ln);
    const int hd1 = C / u->cfg.n_heads;
    if (x3t && u->x3_pairs && (hd1 == 40 || hd1 == 80 || hd1 == 160) && (int64_t)hw * 6 * C * 2 < (1LL << 31)) pair_out_next = true;
    gemm(rows, 3 * C, C, R(ln), qkv, Ref(), R(qkvb));
  }
  Act at = act(rows, C, hw, x.side);
  attention(R(qkvb), Ref{SP_WS, qkvb.off + (int64_t)C * es}, Ref{SP_WS, qkvb.off + (int64_t)2 * C * es}, R(at), hw, hw, C,
            3 * C, 3 * C, 3 * C);
  drop(qkvb);
  Act h2 = act(rows, C, hw, x.side);
  res_pre_next = u->res_pre;
  k320_next = k320;
  gemm(rows, C, C, R(at), o1w, o1b, R(h2), SDN_ACT_NONE, R(h));
  drop(h);
  // cross-attention
  Act qb = act(rows, C, hw, x.side);
  k320_next = k320;
  if (fold12) {
    gemm_ln(h2, rows, C, C, tb + ".attn2.to_q.weight", q2w, l2g, l2b, Ref(), R(qb), SDN_ACT_NONE, u->ln_prepass_all != 0);
  } else {
    layernorm(h2, l2g, l2b, ln);
    if (x3p_cross) pair_out_next = true;
    gemm(rows, C, C, R(ln), q2w, Ref(), R(qb));
  }
  if (rep > 1) {                                 // from here on the branches differ (their text does)
    if (ln.off >= 0) drop(ln);
    drop(at);
    B = Bfull; rows = (int64_t)B * hw;
    Act h2f = act(rows, C, hw, x.side), qbf = act(rows, C, hw, x.side);
    repeat(h2, h2f, rep); repeat(qb, qbf, rep);
    const bool q_is_pairs = pairs.count(qb.off) > 0;         // (a byte-wise copy: pair rows stay pair rows)
    drop(h2); drop(qb);
    h2 = h2f; qb = qbf;
    if (q_is_pairs) pairs.insert(qb.off);
    if (!fold3) ln = act(rows, C, hw, x.side);
    at = act(rows, C, hw, x.side);
  }
  if (u->subbatch_bytes > 0) {
    Act kvb = act((int64_t)B * T, 2 * C);
    gemm((int64_t)B * T, 2 * C, X, Ref{SP_TEXT, text_off}, kv2, Ref(), R(kvb));
    attention(R(qb), R(kvb), Ref{SP_WS, kvb.off + (int64_t)C * es}, R(at), hw, T, C, C, 2 * C, 2 * C);
    drop(qb); drop(kvb);
  } else {
    // the text's keys / values live in the workspace's persistent tail: no other op ever writes there, so a forward that is
    // handed the same text version can skip this projection and read the previous forward's output (sdn_unet::text_version)
    const Ref kvr{SP_KV, kv_top};
    kv_top += Arena::up((int64_t)B * T * 2 * C * es);
    if (x3p_cross) { force_x3t_next = true; pair_out_next = true; }       // text K / V as pair rows [hi(2C) | lo(2C)] (same bytes as f32)
    gemm((int64_t)B * T, 2 * C, X, Ref{SP_TEXT, text_off}, kv2, Ref(), kvr);
    plan->ops.back().text_kv = 1;
    attention(R(qb), kvr, Ref{SP_KV, kvr.off + (int64_t)C * es}, R(at), hw, T, C, C, 2 * C, 2 * C, x3p_cross);
    drop(qb);
  }
  Act h3 = act(rows, C, hw, x.side);
  res_pre_next = u->res_pre;
  k320_next = k320;
  gemm(rows, C, C, R(at), o2w, o2b, R(h3), SDN_ACT_NONE, R(h2));
  drop(h2); drop(at);
  // GEGLU feed-forward
  if (fold3 && u->ff_fuse && u->ffn_fuse && C == 320) {
    // norm3 -> GEGLU projection -> [ff | h3] . [Wpo W2 | Wpo]^T + residual as ONE launch (sdn_ffn.hip): the [rows, 4C] hidden
    // activation stays in LDS.  Same derived weights as the two launches below, same bits.
    if (ln.off >= 0) drop(ln);
    const std::string wname = tb + ".ff.net.0.proj.weight";
    const bool fresh1 = u->param_index.find(wname + "#ln") == u->param_index.end();
    Ref wf = derived(wname + "#ln", (int64_t)8 * C * C * 2), c1 = derived(wname + "#ln_c", (int64_t)8 * C * 4), d1 = derived(wname + "#ln_d", (int64_t)8 * C * 4);
    if (fresh1) u->fold_jobs.push_back({f1w.off, l3g.off, l3b.off, f1b.off, wf.off, c1.off, d1.off, 8 * C, C});
    const bool fresh2 = u->param_index.find(pfx + ".proj_out.weight#ff") == u->param_index.end();
    Ref wcat = derived(pfx + ".proj_out.weight#ff", (int64_t)C * 5 * C * 2), bcat = derived(pfx + ".proj_out.bias#ff", (int64_t)C * 4);
    if (fresh2) { sdn_unet::FoldJob j{f2w.off, pow_.off, f2b.off, pob.off, wcat.off, bcat.off, -1, C, 4 * C}; j.kind = 1; u->fold_jobs.push_back(j); }
    // norm3's row statistics: from the operand fragments inside k_ffn320 (ffn_own_stats), or by a read-only pre-pass over h3
    Act st;
    if (!u->ffn_own_stats) {
      st = act(rows, 2, 0, 0, 4);
      Op o; o.kind = OP_ROWSTATS; o.a = R(h3); o.rows = rows; o.c1 = C; o.eps = 1e-5f; o.out = R(st);
      o.bytes = 2.0 * rows * C; snprintf(o.label, sizeof(o.label), "k_row_stats"); plan->ops.push_back(o);
    }
    want_stats(out);
    Op o; o.kind = OP_FFN; o.a = R(h3); if (st.off >= 0) o.ln_stats = R(st); o.w = wf; o.ln_c = c1; o.ln_d = d1; o.a2 = wcat; o.bias = bcat;
    o.residual = R(rep > 1 ? *x_full : x); o.out = R(out); o.rows = rows; o.c1 = C;
    o.col = pending_cols; pending_cols = Ref();
    o.flops = 2.0 * (double)rows * ((double)8 * C * C + (double)C * 5 * C);
    o.bytes = 2.0 * ((double)rows * C * 3 + (double)8 * C * C + (double)5 * C * C);
    snprintf(o.label, sizeof(o.label), "k_ffn320");
    plan->ops.push_back(o);
    plan->flops += o.flops;
    if (st.off >= 0) drop(st);
    drop(h3);
    return;
  }
  Act ff = act(rows, 4 * C, hw, x.side);
  if (fold3) {
    // (the two-launch form of the C = 320 feed-forward is the fallback / equality partner of k_ffn320: it takes its statistics
    //  the way that kernel does -- from the fragments when ffn_own_stats, else from the pre-pass)
    gemm_ln(h3, rows, 8 * C, C, tb + ".ff.net.0.proj.weight", f1w, l3g, l3b, f1b, R(ff), SDN_ACT_GEGLU, !u->ffn_own_stats);
  } else {
    layernorm(h3, l3g, l3b, ln);
    gemm(rows, 8 * C, C, R(ln), f1w, f1b, R(ff), SDN_ACT_GEGLU);
  }
  if (ln.off >= 0) drop(ln);
  if (u->ff_fuse) {
    // out = x + Wpo (h3 + W2 ff + b2) + bpo = x + [ff | h3] . [Wpo W2 | Wpo]^T + (Wpo b2 + bpo): the FeedForward output linear
    // and proj_out are one GEMM (two-source A operand, K = 5C); the [M, C] tensor between them is never written or re-read
    // and the worst-shaped launch of the block (M x C x C) disappears.  The product weight is derived once per weight set.
    const bool fresh = u->param_index.find(pfx + ".proj_out.weight#ff") == u->param_index.end();
    Ref wcat = derived(pfx + ".proj_out.weight#ff", (int64_t)C * 5 * C * 2), bcat = derived(pfx + ".proj_out.bias#ff", (int64_t)C * 4);
    if (fresh) { sdn_unet::FoldJob j{f2w.off, pow_.off, f2b.off, pob.off, wcat.off, bcat.off, -1, C, 4 * C}; j.kind = 1; u->fold_jobs.push_back(j); }
    want_stats(out);
    res_pre_next = u->res_pre && C != 320;       // (C = 320 must keep the bits of the one-launch k_ffn320, which adds it in its epilogue)
    gemm(rows, C, 5 * C, R(ff), wcat, bcat, R(out), SDN_ACT_NONE, R(rep > 1 ? *x_full : x), SDN_OUT_BF16, 0, R(h3), 4 * C);
    drop(ff); drop(h3);
    return;
  }
  Act h4 = act(rows, C, hw, x.side);
  triple_out_next = x3t;                                  // (bf16x3 plan: proj_out is its only reader)
  gemm(rows, C, 4 * C, R(ff), f2w, f2b, R(h4), SDN_ACT_NONE, R(h3));
  drop(ff); drop(h3);
  want_stats(out);
  gemm(rows, C, C, R(h4), pow_, pob, R(out), SDN_ACT_NONE, R(rep > 1 ? *x_full : x));
  drop(h4);
}

// Walk the architecture once to list every resnet (execution order) -> stacked time_emb_proj.
std::vector<Builder::Res> Builder::enumerate_resnets() const {
  const sdn_unet_config& c = u->cfg;
  std::vector<Res> v;
  char buf[96];
  for (int i = 0; i < c.n_levels; ++i)
    for (int j = 0; j < c.layers_per_block; ++j) {
      snprintf(buf, sizeof(buf), "down_blocks.%d.resnets.%d", i, j);
      v.push_back({buf, c.block_out_channels[i]});
    }
  const int top = c.block_out_channels[c.n_levels - 1];
  v.push_back({"mid_block.resnets.0", top});
  v.push_back({"mid_block.resnets.1", top});
  for (int i = 0; i < c.n_levels; ++i)
    for (int j = 0; j <= c.layers_per_block; ++j) {
      snprintf(buf, sizeof(buf), "up_blocks.%d.resnets.%d", i, j);
      v.push_back({buf, c.block_out_channels[c.n_levels - 1 - i]});
    }
  return v;
}

void Builder::build() {
  const sdn_unet_config& c = u->cfg;
  const int S = c.sample_size, ch0 = c.block_out_channels[0], tdim = 4 * ch0;
  char buf[96];

  // ---- time embedding + stacked time_emb_proj ----
  Ref l1w = param("time_embedding.linear_1.weight", SDN_P_MAT, tdim, ch0), l1b = param("time_embedding.linear_1.bias", SDN_P_VEC_F32, tdim, 0);
  Ref l2w = param("time_embedding.linear_2.weight", SDN_P_MAT, tdim, tdim), l2b = param("time_embedding.linear_2.bias", SDN_P_VEC_F32, tdim, 0);
  const std::vector<Res> rs = enumerate_resnets();
  int total = 0;
  Ref tpw, tpb;
  {
    int64_t expect = -1;
    for (size_t i = 0; i < rs.size(); ++i) {
      Ref r = param(rs[i].pfx + ".time_emb_proj.weight", SDN_P_MAT, rs[i].cout, tdim);
      if (i == 0) tpw = r; else if (r.off != expect) { fprintf(stderr, "libsdn: time_emb_proj not contiguous\n"); abort(); }
      expect = r.off + (int64_t)rs[i].cout * tdim * es;
      total += rs[i].cout;
    }
    expect = -1;
    for (size_t i = 0; i < rs.size(); ++i) {
      Ref r = param(rs[i].pfx + ".time_emb_proj.bias", SDN_P_VEC_F32, rs[i].cout, 0);
      if (i == 0) tpb = r; else if (r.off != expect) { fprintf(stderr, "libsdn: time_emb_proj bias not contiguous\n"); abort(); }
      expect = r.off + (int64_t)rs[i].cout * 4;
    }
  }
  u->tproj_total = total;
  gn_stats = Ref{SP_WS, arena.alloc((int64_t)B * 129 * 64 * 2 * 4)};
  plan->tscalar_off = arena.alloc(256);
  Act tsin = act(B, ch0);
  { Op o; o.kind = OP_TEMB; o.batch = B; o.c1 = ch0; o.out = R(tsin); snprintf(o.label, sizeof(o.label), "k_temb"); plan->ops.push_back(o); }
  x3t_hold = true;                                            // M = batch: the per-sample time-embedding linears
  Act t1 = act(B, tdim);
  gemm(B, tdim, ch0, R(tsin), l1w, l1b, R(t1), SDN_ACT_SILU);
  drop(tsin);
  Act semb = act(B, tdim);
  gemm(B, tdim, tdim, R(t1), l2w, l2b, R(semb), SDN_ACT_SILU);
  drop(t1);
  Act tp = act(B, total, 0, 0, 4);
  tproj = R(tp);
  gemm(B, total, tdim, R(semb), tpw, tpb, R(tp), SDN_ACT_NONE, Ref(), SDN_OUT_F32);
  drop(semb);
  x3t_hold = false;

  // ---- conv_in ----
  Ref ciw = param("conv_in.weight", SDN_P_CONV3X3, ch0, 9 * c.in_channels), cib = param("conv_in.bias", SDN_P_VEC_F32, ch0, 0);
  // latent_repeat: the r guidance branches share their latents -> conv_in, the first resnet and the first transformer
  // block up to its cross-attention query run on B / r samples (see transformer_body)
  const int rep = (c.latent_repeat > 1 && c.level_has_attn[0] && u->subbatch_bytes == 0) ? c.latent_repeat : 1;
  if (B % rep != 0) { plan->ws_bytes = -1; return; }            // forward rejects this batch
  const int Bfull = B, Bp = B / rep;
  Act hp = act((int64_t)Bp * S * S, ch0, S * S, S);
  { Op o; o.kind = OP_CONV_IN; o.batch = Bp; o.c1 = c.in_channels; o.c2 = ch0; o.hw = S; o.a = Ref{SP_IN, 0}; o.w = ciw; o.bias = cib; o.out = R(hp);
    o.flops = 2.0 * Bp * S * S * (double)ch0 * 9 * c.in_channels; o.bytes = (double)Bp * S * S * (4.0 * c.in_channels + 2.0 * ch0);
    snprintf(o.label, sizeof(o.label), "k_conv_in"); plan->ops.push_back(o);
    plan->flops += o.flops; }
  Act h = hp;
  if (rep > 1) { h = act((int64_t)B * S * S, ch0, S * S, S); repeat(hp, h, rep); }

  std::vector<Act> skips;
  skips.push_back(h);                       // h stays alive as a skip; keep using it as the running tensor
  Act cur = h;
  bool cur_is_skip = true;

  // ---- down path ----
  for (int i = 0; i < c.n_levels; ++i) {
    const int cout = c.block_out_channels[i];
    for (int j = 0; j < c.layers_per_block; ++j) {
      snprintf(buf, sizeof(buf), "down_blocks.%d.resnets.%d", i, j);
      if (rep > 1 && i == 0 && j == 0) {        // shared prefix: resnet 0 and the head of transformer 0 at B / rep
        B = Bp;
        Act rp = resnet(buf, hp, nullptr, cout);
        B = Bfull;
        drop(hp);
        Act rf = act((int64_t)B * rp.hw, cout, rp.hw, rp.side);
        repeat(rp, rf, rep);
        snprintf(buf, sizeof(buf), "down_blocks.%d.attentions.%d", i, j);
        Act t = act_gn((int64_t)B * rp.hw, cout, rp.hw, rp.side);
        transformer_body(buf, rp, t, 0, rep, &rf);
        drop(rp); drop(rf);
        cur = t; skips.push_back(cur); cur_is_skip = true;
        continue;
      }
      Act r = resnet(buf, cur, nullptr, cout);
      if (!cur_is_skip) drop(cur);
      cur = r; cur_is_skip = false;
      if (c.level_has_attn[i]) {
        snprintf(buf, sizeof(buf), "down_blocks.%d.attentions.%d", i, j);
        Act t = transformer(buf, cur);
        drop(cur);
        cur = t;
      }
      skips.push_back(cur); cur_is_skip = true;
    }
    if (i + 1 < c.n_levels) {
      snprintf(buf, sizeof(buf), "down_blocks.%d.downsamplers.0.conv", i);
      Ref w = param(std::string(buf) + ".weight", SDN_P_CONV3X3, cout, 9 * cout), bb = param(std::string(buf) + ".bias", SDN_P_VEC_F32, cout, 0);
      const int s2 = cur.side / 2;
      Act d = act_gn((int64_t)B * s2 * s2, cout, s2 * s2, s2);
      want_stats(d);
      conv3x3(cur, cout, cout, w, bb, R(d), 2, 0, Ref(), Ref(), 0);
      cur = d; skips.push_back(cur); cur_is_skip = true;
    }
  }
  // ---- mid ----
  {
    Act r = resnet("mid_block.resnets.0", cur, nullptr, cur.C);
    cur = r; cur_is_skip = false;
    Act t = transformer("mid_block.attentions.0", cur);
    drop(cur); cur = t;
    Act r2 = resnet("mid_block.resnets.1", cur, nullptr, cur.C);
    drop(cur); cur = r2;
  }
  // ---- up path ----
  for (int i = 0; i < c.n_levels; ++i) {
    const int lvl = c.n_levels - 1 - i, cout = c.block_out_channels[lvl];
    for (int j = 0; j <= c.layers_per_block; ++j) {
      Act skip = skips.back(); skips.pop_back();
      snprintf(buf, sizeof(buf), "up_blocks.%d.resnets.%d", i, j);
      Act r = resnet(buf, cur, &skip, cout);
      drop(cur); drop(skip);
      cur = r;
      if (c.level_has_attn[lvl]) {
        snprintf(buf, sizeof(buf), "up_blocks.%d.attentions.%d", i, j);
        Act t = transformer(buf, cur);
        drop(cur); cur = t;
      }
    }
    if (i + 1 < c.n_levels) {
      snprintf(buf, sizeof(buf), "up_blocks.%d.upsamplers.0.conv", i);
      Ref w = param(std::string(buf) + ".weight", SDN_P_CONV3X3, cout, 9 * cout), bb = param(std::string(buf) + ".bias", SDN_P_VEC_F32, cout, 0);
      const int s2 = cur.side * 2;
      Act up = act_gn((int64_t)B * s2 * s2, cout, s2 * s2, s2);
      want_stats(up);
      conv3x3(cur, cout, cout, w, bb, R(up), 1, 1, Ref(), Ref(), 0);
      drop(cur); cur = up;
    }
  }
  // ---- tail: GN + SiLU + conv_out -> fp32 NCHW ----
  Ref og = param("conv_norm_out.weight", SDN_P_VEC_F32, ch0, 0), ob = param("conv_norm_out.bias", SDN_P_VEC_F32, ch0, 0);
  const int npad = 32;
  Ref cow = param("conv_out.weight", SDN_P_CONV3X3, c.out_channels, 9 * ch0, npad);
  Ref cob = param("conv_out.bias", SDN_P_VEC_F32, c.out_channels, 0, npad);
  Act g = act((int64_t)B * S * S, ch0, S * S, S);
  groupnorm(cur, nullptr, 1e-5f, 1, og, ob, g);
  drop(cur);
  conv3x3(g, c.out_channels, npad, cow, cob, Ref{SP_OUT, 0}, 1, 0, Ref(), Ref(), 0, SDN_OUT_F32_NCHW, c.out_channels);
  drop(g);
  finish_up4();
  plan->kv_base = Arena::up(arena.peak);
  plan->ws_bytes = plan_bad ? -1 : plan->kv_base + kv_top;
}

}  // namespace sdn_plan
