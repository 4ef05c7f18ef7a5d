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

// the derived regions {folded weight, c, d} of a linear [N, K] behind a LayerNorm, and the job that fills them
std::vector<Ref> Builder::ln_fold_regions(const std::string& wname, Ref w, Ref gamma, Ref beta, Ref bias, int N, int K) {
  return derived_job({{wname + "#ln", (int64_t)N * K * 2}, {wname + "#ln_c", (int64_t)N * 4}, {wname + "#ln_d", (int64_t)N * 4}},
                     {w.off, gamma.off, beta.off, bias.space == SP_NONE ? -1 : bias.off, -1, -1, -1, N, K});
}
// row statistics of x [rows, C] by a read-only pass, for a folded LayerNorm that does not take them from its own fragments
void Builder::row_stats(Ref x, int64_t rows, int C, const Act& st) {
  Op o; o.kind = OP_ROWSTATS; o.a = x; o.rows = rows; o.c1 = C; o.eps = 1e-5f; o.out = R(st);
  o.bytes = 2.0 * rows * C; snprintf(o.label, sizeof(o.label), "k_row_stats");
  emit(o);
}
// LayerNorm(a; gamma, beta) -> GEMM(w, bias) with the norm folded into the GEMM (sdn_gemm_ln_*): s names the linear's own a / w /
// bias (the op runs on the folded forms); beyond them it can take act and k320.  `prepass` = row statistics from a read-only pass
// instead of inside the kernel (wide N).
void Builder::gemm_ln(const GemmSpec& s, const std::string& wname, Ref gamma, Ref beta, bool prepass) {
  if (s.cols.space != SP_NONE || s.a2.space != SP_NONE || s.residual.space != SP_NONE || s.rowbias.space != SP_NONE || s.rowgate.space != SP_NONE ||
      s.out_kind != SDN_OUT_BF16 || s.n_valid || s.res_pre || s.triple_out || s.pair_out || s.force_x3t || s.text_kv || s.dyn_ldc || s.f32_stream)
    plan_bad = true;                                           // sdn_gemm_ln_* has neither a statistics output nor any of the others
  const int64_t rows = s.M; const int N = s.N, K = s.K;
  const std::vector<Ref> f = ln_fold_regions(wname, s.w, gamma, beta, s.bias, N, K);
  Act st;
  if (prepass) { st = act(rows, 2, 0, 0, 4); row_stats(s.a, rows, K, st); }
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.gd.M = (int)rows; o.gd.N = N; o.gd.K = K; o.gd.a_mode = SDN_A_PLAIN; o.gd.act = s.act; o.gd.out_kind = SDN_OUT_BF16;
  o.a = s.a; o.w = f[0]; o.out = s.out; o.ln = 1; o.ln_c = f[1]; o.ln_d = f[2]; o.eps = 1e-5f;
  if (prepass) o.ln_stats = R(st);
  o.flops = 2.0 * (double)rows * N * K;
  o.bytes = 2.0 * ((double)rows * K + (double)N * K + (double)rows * (s.act == SDN_ACT_GEGLU ? N / 2 : N));
  { int t = sdn_gemm_pick_tile((int)rows, N, K, s.act);
    if (t == 8 && N % 320 == 0) t = 10;                        // (sdn_gemm_impl: the folded forms have no 256-wide instantiation)
    snprintf(o.label, sizeof(o.label), "k_gemm<%d>/ln%d", t, prepass ? 2 : 1); }   // /lnL: L = the symbol's LNF
  if (s.k320 && !prepass && K == 320 && N % 320 == 0 && s.act == SDN_ACT_NONE && kK320Ln) {
    o.k320 = 1;                                                // statistics from the fragments, as LNF = 1: sdn_gemm_k320
    snprintf(o.label, sizeof(o.label), "k_gemm_k320/ln1");
  }
  emit(o);
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
  conv3x3(ConvSpec(g1, cout, c1w, c1b, R(h)).with_rowbias(Ref{SP_WS, tproj.off + (int64_t)tcol * 4}, u->tproj_total).with_cols(stats_of(h)));
  drop(g1);
  Act g2 = act(rows, cout, x.hw, x.side);
  groupnorm(h, nullptr, 1e-5f, 1, n2g, n2b, g2);
  drop(h);
  Act out = act_gn(rows, cout, x.hw, x.side);
  Act sc;                                                    // the shortcut: x itself, or its 1x1 conv
  if (cin != cout) {
    Ref scw = param(pfx + ".conv_shortcut.weight", SDN_P_MAT, cout, cin), scb = param(pfx + ".conv_shortcut.bias", SDN_P_VEC_F32, cout, 0);
    sc = act(rows, cout, x.hw, x.side);
    gemm(GemmSpec(rows, cout, cin, R(x), scw, scb, R(sc)).with_a2(skip ? R(*skip) : Ref(), skip ? x.C : 0));
  }
  conv3x3(ConvSpec(g2, cout, c2w, c2b, R(out)).with_residual(cin != cout ? R(sc) : R(x)).with_res_pre(u->res_pre).with_cols(stats_of(out)));
  drop(sc); drop(g2);
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
  gemm(GemmSpec(rows, C, C, R(gn), piw, pib, R(h)).with_k320(k320));
  drop(gn);
  // LayerNorm folding (gemm_ln): measured per shape (tools/bench_lnfold.py) -- it pays at C = 320 / 640 for the
  // attention projections (statistics inside the kernel while N <= 960, from a read-only pre-pass above) and at
  // C = 320 for the GEGLU projection; the wide, MFMA-bound projections of the lower levels keep the LayerNorm kernel.
  const bool fold12 = u->ln_fold && C <= 640, fold3 = u->ln_fold && C == 320;
  const int hd = C / u->cfg.n_heads;
  const bool x3p = x3t && u->x3_pairs && (hd == 40 || hd == 80 || hd == 160);     // head sizes of sdn_attention_x3_pairs
  const bool x3p_self = x3p && (int64_t)hw * 6 * C * 2 < (1LL << 31), x3p_cross = x3p && u->subbatch_bytes == 0;   // ... on the cross-attention too
  // a projection behind a LayerNorm: folded into the GEMM, or the norm's own launch into `ln` in front of it
  Act ln;
  auto ln_gemm = [&](bool fold, const Act& in, const char* wname, Ref g, Ref b, bool prepass, GemmSpec s) {
    if (fold) { s.a = R(in); gemm_ln(s, tb + wname, g, b, prepass); }
    else { layernorm(in, g, b, ln); s.a = R(ln); gemm(s); }
  };
  // self-attention
  if (!fold12 || !fold3) ln = act(rows, C, hw, x.side);
  Act qkvb = act(rows, 3 * C, hw, x.side);
  ln_gemm(fold12, h, ".attn1.to_q.weight", l1g, l1b, 3 * C > 960 || u->ln_prepass_all,
          GemmSpec(rows, 3 * C, C, Ref(), qkv, Ref(), R(qkvb)).with_k320(k320).with_pair_out(!fold12 && x3p_self));
  Act at = act(rows, C, hw, x.side);
  attention(R(qkvb), Ref{SP_WS, qkvb.off + (int64_t)C * es}, Ref{SP_WS, qkvb.off + (int64_t)2 * C * es}, R(at), hw, hw, C,
            3 * C, 3 * C, 3 * C);
  drop(qkvb);
  Act h2 = act(rows, C, hw, x.side);
  gemm(GemmSpec(rows, C, C, R(at), o1w, o1b, R(h2)).with_residual(R(h)).with_res_pre(u->res_pre).with_k320(k320));
  drop(h);
  // cross-attention
  Act qb = act(rows, C, hw, x.side);
  ln_gemm(fold12, h2, ".attn2.to_q.weight", l2g, l2b, u->ln_prepass_all != 0,
          GemmSpec(rows, C, C, Ref(), q2w, Ref(), R(qb)).with_k320(k320).with_pair_out(!fold12 && x3p_cross));
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
    gemm(GemmSpec((int64_t)B * T, 2 * C, X, Ref{SP_TEXT, text_off}, kv2, Ref(), R(kvb)));
    attention(R(qb), R(kvb), Ref{SP_WS, kvb.off + (int64_t)C * es}, R(at), hw, T, C, C, 2 * C, 2 * C);
    drop(qb); drop(kvb);
  } else {
    // the text's keys / values live in the workspace's persistent tail: no other op ever writes there, so a forward that is
    // handed the same text version can skip this projection and read the previous forward's output (sdn_unet::text_version).
    // x3p_cross: text K / V as pair rows [hi(2C) | lo(2C)] (same bytes as f32)
    const Ref kvr{SP_KV, kv_top};
    kv_top += Arena::up((int64_t)B * T * 2 * C * es);
    gemm(GemmSpec((int64_t)B * T, 2 * C, X, Ref{SP_TEXT, text_off}, kv2, Ref(), kvr).with_text_kv().with_force_x3t(x3p_cross).with_pair_out(x3p_cross));
    attention(R(qb), kvr, Ref{SP_KV, kvr.off + (int64_t)C * es}, R(at), hw, T, C, C, 2 * C, 2 * C, x3p_cross);
    drop(qb);
  }
  Act h3 = act(rows, C, hw, x.side);
  gemm(GemmSpec(rows, C, C, R(at), o2w, o2b, R(h3)).with_residual(R(h2)).with_res_pre(u->res_pre).with_k320(k320));
  drop(h2); drop(at);
  // GEGLU feed-forward
  const Ref xres = R(rep > 1 ? *x_full : x);     // the block's residual
  // out = x + Wpo (h3 + W2 ff + b2) + bpo = x + [ff | h3] . [Wpo W2 | Wpo]^T + (Wpo b2 + bpo): the FeedForward output linear and
  // proj_out as one contraction over K = 5C, with the product weight / bias {wcat, bcat} derived once per weight set
  auto ff_pair = [&] {
    return derived_job({{pfx + ".proj_out.weight#ff", (int64_t)C * 5 * C * 2}, {pfx + ".proj_out.bias#ff", (int64_t)C * 4}},
                       {f2w.off, pow_.off, f2b.off, pob.off, -1, -1, -1, C, 4 * C, 1});
  };
  if (fold3 && u->ff_fuse && u->ffn_fuse && C == 320) {
    // norm3 -> GEGLU projection -> [ff | h3] . [Wpo W2 | Wpo]^T + residual as ONE launch (sdn_ffn.hip): the [rows, 4C] hidden
    // activation stays in LDS.  Same derived weights as the two launches below, same bits.
    if (ln.off >= 0) drop(ln);
    const std::vector<Ref> f1 = ln_fold_regions(tb + ".ff.net.0.proj.weight", f1w, l3g, l3b, f1b, 8 * C, C), f2 = ff_pair();
    // norm3's row statistics: from the operand fragments inside k_ffn320 (ffn_own_stats), or by a read-only pre-pass over h3
    Act st;
    if (!u->ffn_own_stats) { st = act(rows, 2, 0, 0, 4); row_stats(R(h3), rows, C, st); }
    Op o; o.kind = OP_FFN; o.a = R(h3); if (st.off >= 0) o.ln_stats = R(st); o.w = f1[0]; o.ln_c = f1[1]; o.ln_d = f1[2]; o.a2 = f2[0]; o.bias = f2[1];
    o.residual = xres; o.out = R(out); o.rows = rows; o.c1 = C;
    o.col = stats_of(out);
    o.flops = 2.0 * (double)rows * ((double)8 * C * C + (double)C * 5 * C);
    o.bytes = 2.0 * ((double)rows * C * 3 + (double)8 * C * C + (double)5 * C * C);
    snprintf(o.label, sizeof(o.label), "k_ffn320");
    emit(o);
    if (st.off >= 0) drop(st);
    drop(h3);
    return;
  }
  Act ff = act(rows, 4 * C, hw, x.side);
  // (fold3: the two-launch form of the C = 320 feed-forward is the fallback / equality partner of k_ffn320: it takes its statistics
  //  the way that kernel does -- from the fragments when ffn_own_stats, else from the pre-pass)
  ln_gemm(fold3, h3, ".ff.net.0.proj.weight", l3g, l3b, !u->ffn_own_stats, GemmSpec(rows, 8 * C, C, Ref(), f1w, f1b, R(ff)).with_act(SDN_ACT_GEGLU));
  if (ln.off >= 0) drop(ln);
  if (u->ff_fuse) {
    // two-source A operand: the [M, C] tensor between the two linears is never written or re-read and the worst-shaped launch
    // of the block (M x C x C) disappears.  (C = 320 must keep the bits of the one-launch k_ffn320, which adds x in its epilogue)
    const std::vector<Ref> f2 = ff_pair();
    gemm(GemmSpec(rows, C, 5 * C, R(ff), f2[0], f2[1], R(out)).with_a2(R(h3), 4 * C).with_residual(xres).with_res_pre(u->res_pre && C != 320)
             .with_cols(stats_of(out)));
    drop(ff); drop(h3);
    return;
  }
  Act h4 = act(rows, C, hw, x.side);
  gemm(GemmSpec(rows, C, 4 * C, R(ff), f2w, f2b, R(h4)).with_residual(R(h3)).with_triple_out(x3t));   // (bf16x3 plan: proj_out is its only reader)
  drop(ff); drop(h3);
  gemm(GemmSpec(rows, C, C, R(h4), pow_, pob, R(out)).with_residual(xres).with_cols(stats_of(out)));
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
  std::vector<std::pair<std::string, int>> tw, tb;
  for (const Res& r : rs) { tw.push_back({r.pfx + ".time_emb_proj.weight", r.cout}); tb.push_back({r.pfx + ".time_emb_proj.bias", r.cout}); total += r.cout; }
  Ref tpw = stacked(tw, tdim), tpb = stacked(tb, 0);
  u->tproj_total = total;
  gn_stats = Ref{SP_WS, arena.alloc((int64_t)B * 129 * 64 * 2 * 4)};
  plan->tscalar_off = arena.alloc(256);
  Act tsin = act(B, ch0);
  { Op o; o.kind = OP_TEMB; o.batch = B; o.c1 = ch0; o.out = R(tsin); snprintf(o.label, sizeof(o.label), "k_temb"); emit(o); }
  x3t_hold = true;                                            // M = batch: the per-sample time-embedding linears
  Act t1 = act(B, tdim);
  gemm(GemmSpec(B, tdim, ch0, R(tsin), l1w, l1b, R(t1)).with_act(SDN_ACT_SILU));
  drop(tsin);
  Act semb = act(B, tdim);
  gemm(GemmSpec(B, tdim, tdim, R(t1), l2w, l2b, R(semb)).with_act(SDN_ACT_SILU));
  drop(t1);
  Act tp = act(B, total, 0, 0, 4);
  tproj = R(tp);
  gemm(GemmSpec(B, total, tdim, R(semb), tpw, tpb, R(tp)).with_out_kind(SDN_OUT_F32));
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
    snprintf(o.label, sizeof(o.label), "k_conv_in"); emit(o); }
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
      conv3x3(ConvSpec(cur, cout, w, bb, R(d)).with_stride(2).with_cols(stats_of(d)));
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
      conv3x3(ConvSpec(cur, cout, w, bb, R(up)).with_upsample().with_cols(stats_of(up)));
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
  conv3x3(ConvSpec(g, c.out_channels, cow, cob, Ref{SP_OUT, 0}).with_nchw_out(npad));
  drop(g);
  finish_up4();
  plan->kv_base = Arena::up(arena.peak);
  plan->ws_bytes = plan->kv_base + kv_top;
}

}  // namespace sdn_plan
