// Launch planner, SD-v3 MMDiT: the modulated LayerNorm and general GEMM emitters only this model uses, and build_mmdit().
#include <math.h>

#include "sdn_plan.h"

namespace sdn_plan {

// =====================================================================================================
//  SD-v3 MMDiT (SD3Transformer2DModel, diffusers 0.29.0; row U7) -- reached through self.transformer(...) at
//  models/sdv3/safe_denoiser_pipeline.py:1120-1127.  Two token streams (image, text) with adaLN-zero
//  modulation from (timestep, pooled text); joint attention over both streams without concatenating them.
// =====================================================================================================
// The MMDiT's GEMM: per-sample row bias / gate and a broadcast residual; bytes at the storage width, the residual not charged.
void Builder::gemm_ex(const GemmSpec& s) {
  if (s.a2.space != SP_NONE || s.n_valid || s.res_pre || s.k320 || s.triple_out || s.pair_out || s.force_x3t || s.text_kv || s.dyn_ldc || s.f32_stream)
    plan_bad = true;                                           // forms of gemm() / t5_gemm()
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.gd.M = (int)s.M; o.gd.N = s.N; o.gd.K = s.K; o.gd.a_mode = SDN_A_PLAIN; o.gd.act = s.act; o.gd.out_kind = s.out_kind;
  o.gd.rows_per_batch = s.rows_per_batch; o.gd.ld_rowbias = s.ld_row; o.gd.ld_rowgate = s.ld_row;
  o.gd.residual_bcast = s.residual_bcast;
  o.a = s.a; o.w = s.w; o.bias = s.bias; o.rowbias = s.rowbias; o.rowgate = s.rowgate; o.residual = s.residual; o.out = s.out;
  o.flops = 2.0 * (double)s.M * s.N * s.K;
  o.bytes = es * ((double)s.M * s.K + (double)s.N * s.K + (double)s.M * s.N);
  if (es == 4)                      // MMDiT fp32-storage plans: sdn_gemm_f32, or sdn_gemm_x3 (its f32 tile below 64 rows)
    snprintf(o.label, sizeof(o.label), (u->mcfg.dtype == 3 && s.M >= 64) ? "k_gemm_x3" : "k_gemm_f32");
  else
    snprintf(o.label, sizeof(o.label), "k_gemm<%d>", sdn_gemm_pick_tile((int)s.M, s.N, s.K, s.act, s.residual.space != SP_NONE || s.rowgate.space != SP_NONE));
  push_gemm(o, s.cols);
}
void Builder::ln_mod(const Act& x, int64_t rows, int rows_per_batch, Ref scale, Ref shift, int ld, const Act& out) {
  Op o; o.kind = OP_LN; o.a = R(x); o.rows = rows; o.c1 = x.C; o.eps = 1e-6f; o.w = scale; o.bias = shift; o.out = R(out);
  o.mod = 1; o.ld_mod = ld; o.hw = rows_per_batch;
  o.bytes = 2.0 * es * (double)rows * x.C;
  snprintf(o.label, sizeof(o.label), es == 4 ? "k_layernorm_mod_f32" : "k_layernorm");
  emit(o);
}
// SD-3.5 q/k RMS norm, in place on the q and k thirds of a stacked QKV projection's rows (sdn_qk_rmsnorm): reads and writes 2C per row
void Builder::qk_rmsnorm(const Act& qkv, int64_t rows, Ref wq, Ref wk) {
  Op o; o.kind = OP_QK_RMSNORM; o.a = R(qkv); o.w = wq; o.bias = wk; o.rows = rows; o.heads = u->mcfg.num_heads; o.ldq = qkv.C;
  o.eps = u->mext.qk_norm_eps;
  o.bytes = 2.0 * es * (double)rows * 2.0 * (o.heads * u->mcfg.head_dim);
  snprintf(o.label, sizeof(o.label), "k_qk_rmsnorm");
  emit(o);
}

void Builder::build_mmdit() {
  const sdn_mmdit_config& c = u->mcfg;
  const bool qkn = u->mext.qk_norm == 1;                                         // the SD-3.5 additions (sdn_mmdit_create_ex)
  auto dual = [&](int i) { return i < 64 && ((u->mext.dual_attention_mask >> i) & 1) != 0; };
  const int C = c.num_heads * c.head_dim, S = c.sample_size, ps = c.patch_size, hp = S / ps, N = hp * hp;
  const int T = c.text_len, L = c.num_layers, KP = c.in_channels * ps * ps;
  char buf[128];
  auto nm = [&](int i, const char* suffix) { snprintf(buf, sizeof(buf), "transformer_blocks.%d.%s", i, suffix); return std::string(buf); };

  // ---- parameters of the conditioning path ----
  Ref pew = param("pos_embed.proj.weight", SDN_P_MAT, C, KP), peb = param("pos_embed.proj.bias", SDN_P_VEC_F32, C, 0);
  Ref pos = param("pos_embed.pos_embed", SDN_P_POS_CROP, N, C);
  Ref t1w = param("time_text_embed.timestep_embedder.linear_1.weight", SDN_P_MAT, C, c.time_dim), t1b = param("time_text_embed.timestep_embedder.linear_1.bias", SDN_P_VEC_F32, C, 0);
  Ref t2w = param("time_text_embed.timestep_embedder.linear_2.weight", SDN_P_MAT, C, C), t2b = param("time_text_embed.timestep_embedder.linear_2.bias", SDN_P_VEC_F32, C, 0);
  Ref p1w = param("time_text_embed.text_embedder.linear_1.weight", SDN_P_MAT, C, c.pooled_dim), p1b = param("time_text_embed.text_embedder.linear_1.bias", SDN_P_VEC_F32, C, 0);
  Ref p2w = param("time_text_embed.text_embedder.linear_2.weight", SDN_P_MAT, C, C), p2b = param("time_text_embed.text_embedder.linear_2.bias", SDN_P_VEC_F32, C, 0);
  Ref cew = param("context_embedder.weight", SDN_P_MAT, C, c.joint_dim), ceb = param("context_embedder.bias", SDN_P_VEC_F32, C, 0);

  // ---- ALL adaLN linears stacked into one [sum, C] matrix: one GEMM per forward ----
  // column layout per block i: img 6C (9C in a dual-attention block) at col_img[i], ctx 6C (2C for the last, context_pre_only block) at col_ctx[i]
  std::vector<int> col_img(L), col_ctx(L);
  int total = 0;
  std::vector<std::pair<std::string, int>> lins, adws, adbs;
  for (int i = 0; i < L; ++i) {
    const int ni = dual(i) ? 9 * C : 6 * C;
    col_img[i] = total; lins.push_back({nm(i, "norm1.linear"), ni}); total += ni;
    const int nc = (i == L - 1) ? 2 * C : 6 * C;
    col_ctx[i] = total; lins.push_back({nm(i, "norm1_context.linear"), nc}); total += nc;
  }
  lins.push_back({"norm_out.linear", 2 * C}); total += 2 * C;                       // at column total - 2C
  for (const auto& m : lins) { adws.push_back({m.first + ".weight", m.second}); adbs.push_back({m.first + ".bias", m.second}); }
  Ref adw = stacked(adws, C), adb = stacked(adbs, 0);
  u->tproj_total = total;
  // The 16-bit GEMM addresses an operand with 31-bit byte offsets (sdn_gemm_impl refuses N K 2 >= 2^31).  Where the whole stacked
  // matrix passes that (38 blocks of 2432: 5.4 GB; every SD3 / SD-3.5-medium plan stays one group) the GEMM is emitted per group of
  // whole members, each group into a modulation buffer of its own; a member's columns then live at (buffer, leading dimension) of
  // its group.  The parameters stay one contiguous stack either way.
  struct ModGroup { int col0, cols; Act buf; };
  std::vector<ModGroup> groups(1, ModGroup{0, 0, Act{}});
  for (const auto& m : lins) {
    if (es == 2 && groups.back().cols > 0 && ((int64_t)groups.back().cols + m.second) * C * es >= ((int64_t)1 << 31))
      groups.push_back(ModGroup{groups.back().col0 + groups.back().cols, 0, Act{}});
    groups.back().cols += m.second;
  }

  // ---- conditioning: silu(time_emb + pooled_emb) -> all modulation vectors ----
  plan->tscalar_off = arena.alloc(256);
  Act tsin = act(B, c.time_dim);
  { Op o; o.kind = OP_TEMB; o.batch = B; o.c1 = c.time_dim; o.out = R(tsin); snprintf(o.label, sizeof(o.label), es == 4 ? "k_temb_f32" : "k_temb"); emit(o); }
  Act th = act(B, C);
  gemm_ex(GemmSpec(B, C, c.time_dim, R(tsin), t1w, t1b, R(th)).with_act(SDN_ACT_SILU));
  drop(tsin);
  Act temb = act(B, C, 0, 0, 4);                                                 // f32 [B, C]
  gemm_ex(GemmSpec(B, C, C, R(th), t2w, t2b, R(temb)).with_out_kind(SDN_OUT_F32));
  drop(th);
  Act ph = act(B, C);
  gemm_ex(GemmSpec(B, C, c.pooled_dim, Ref{SP_POOLED, 0}, p1w, p1b, R(ph)).with_act(SDN_ACT_SILU));
  Act scond = act(B, C);                                                         // silu(time_emb + pooled_emb)
  gemm_ex(GemmSpec(B, C, C, R(ph), p2w, p2b, R(scond)).with_act(SDN_ACT_SILU).with_rowbias(R(temb), 1, C));
  drop(ph); drop(temb);
  for (ModGroup& g : groups) {
    g.buf = act(B, g.cols, 0, 0, 4);
    gemm_ex(GemmSpec(B, g.cols, C, R(scond), Ref{SP_W, adw.off + (int64_t)g.col0 * C * es}, Ref{SP_W, adb.off + (int64_t)g.col0 * 4}, R(g.buf))
                .with_out_kind(SDN_OUT_F32));
  }
  tproj = R(groups[0].buf);
  drop(scond);
  // column `col` of the stacked modulation: the buffer of its group and that group's leading dimension
  auto group_of = [&](int col) -> const ModGroup& { size_t i = groups.size() - 1; while (groups[i].col0 > col) --i; return groups[i]; };
  auto fcol = [&](int col) { const ModGroup& g = group_of(col); return Ref{SP_WS, g.buf.off + (int64_t)(col - g.col0) * 4}; };
  auto fld = [&](int col) { return group_of(col).cols; };

  // ---- token streams ----
  Act patches = act((int64_t)B * N, KP);
  { Op o; o.kind = OP_PATCHIFY; o.batch = B; o.c1 = c.in_channels; o.hw = S; o.patch = ps; o.a = Ref{SP_IN, 0}; o.out = R(patches);
    o.bytes = (double)B * N * KP * (4.0 + es); snprintf(o.label, sizeof(o.label), es == 4 ? "k_patchify_f32" : "k_patchify"); emit(o); }
  Act x = act((int64_t)B * N, C, N);
  gemm_ex(GemmSpec((int64_t)B * N, C, KP, R(patches), pew, peb, R(x)).with_residual_bcast(pos, N));
  drop(patches);
  Act ctx = act((int64_t)B * T, C, T);
  gemm_ex(GemmSpec((int64_t)B * T, C, c.joint_dim, Ref{SP_TEXT, 0}, cew, ceb, R(ctx)));

  for (int i = 0; i < L; ++i) {
    const bool last = (i == L - 1);
    const int ci = col_img[i], cc = col_ctx[i];
    // AdaLayerNormZero chunk order: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp (SD35AdaLayerNormZeroX of a
    // dual-attention block: the same six, then shift_msa2, scale_msa2, gate_msa2)
    // AdaLayerNormContinuous (last block's context): scale, shift
    Ref qkvw = stacked({nm(i, "attn.to_q.weight"), nm(i, "attn.to_k.weight"), nm(i, "attn.to_v.weight")}, C, C);
    Ref qkvb; { Ref r0 = param(nm(i, "attn.to_q.bias"), SDN_P_VEC_F32, C, 0); param(nm(i, "attn.to_k.bias"), SDN_P_VEC_F32, C, 0); param(nm(i, "attn.to_v.bias"), SDN_P_VEC_F32, C, 0); qkvb = r0; }
    Ref aqkvw = stacked({nm(i, "attn.add_q_proj.weight"), nm(i, "attn.add_k_proj.weight"), nm(i, "attn.add_v_proj.weight")}, C, C);
    Ref aqkvb; { Ref r0 = param(nm(i, "attn.add_q_proj.bias"), SDN_P_VEC_F32, C, 0); param(nm(i, "attn.add_k_proj.bias"), SDN_P_VEC_F32, C, 0); param(nm(i, "attn.add_v_proj.bias"), SDN_P_VEC_F32, C, 0); aqkvb = r0; }
    Ref ow = param(nm(i, "attn.to_out.0.weight"), SDN_P_MAT, C, C), ob = param(nm(i, "attn.to_out.0.bias"), SDN_P_VEC_F32, C, 0);
    Ref f1w = param(nm(i, "ff.net.0.proj.weight"), SDN_P_MAT, 4 * C, C), f1b = param(nm(i, "ff.net.0.proj.bias"), SDN_P_VEC_F32, 4 * C, 0);
    Ref f2w = param(nm(i, "ff.net.2.weight"), SDN_P_MAT, C, 4 * C), f2b = param(nm(i, "ff.net.2.bias"), SDN_P_VEC_F32, C, 0);
    // SD-3.5: per-head RMS-norm gains of q / k (the last block's norm_added_q is in the checkpoint although its text output is
    // discarded), and the dual-attention block's image-only attn2; its chunks of norm1.linear: 6 shift_msa2, 7 scale_msa2, 8 gate_msa2
    Ref nq, nk, naq, nak, q2w, q2b, o2w, o2b, n2q, n2k;
    if (qkn) {
      nq = param(nm(i, "attn.norm_q.weight"), SDN_P_VEC_F32, c.head_dim, 0); nk = param(nm(i, "attn.norm_k.weight"), SDN_P_VEC_F32, c.head_dim, 0);
      naq = param(nm(i, "attn.norm_added_q.weight"), SDN_P_VEC_F32, c.head_dim, 0); nak = param(nm(i, "attn.norm_added_k.weight"), SDN_P_VEC_F32, c.head_dim, 0);
    }
    if (dual(i)) {
      q2w = stacked({nm(i, "attn2.to_q.weight"), nm(i, "attn2.to_k.weight"), nm(i, "attn2.to_v.weight")}, C, C);
      { Ref r0 = param(nm(i, "attn2.to_q.bias"), SDN_P_VEC_F32, C, 0); param(nm(i, "attn2.to_k.bias"), SDN_P_VEC_F32, C, 0); param(nm(i, "attn2.to_v.bias"), SDN_P_VEC_F32, C, 0); q2b = r0; }
      o2w = param(nm(i, "attn2.to_out.0.weight"), SDN_P_MAT, C, C); o2b = param(nm(i, "attn2.to_out.0.bias"), SDN_P_VEC_F32, C, 0);
      if (qkn) { n2q = param(nm(i, "attn2.norm_q.weight"), SDN_P_VEC_F32, c.head_dim, 0); n2k = param(nm(i, "attn2.norm_k.weight"), SDN_P_VEC_F32, c.head_dim, 0); }
    }

    Act xn = act((int64_t)B * N, C, N);
    ln_mod(x, (int64_t)B * N, N, fcol(ci + 1 * C), fcol(ci + 0 * C), fld(ci), xn);
    Act cn = act((int64_t)B * T, C, T);
    if (last) ln_mod(ctx, (int64_t)B * T, T, fcol(cc + 0 * C), fcol(cc + 1 * C), fld(cc), cn);
    else ln_mod(ctx, (int64_t)B * T, T, fcol(cc + 1 * C), fcol(cc + 0 * C), fld(cc), cn);
    Act qx = act((int64_t)B * N, 3 * C, N), qc = act((int64_t)B * T, 3 * C, T);
    gemm_ex(GemmSpec((int64_t)B * N, 3 * C, C, R(xn), qkvw, qkvb, R(qx)));
    gemm_ex(GemmSpec((int64_t)B * T, 3 * C, C, R(cn), aqkvw, aqkvb, R(qc)));
    drop(xn); drop(cn);
    if (qkn) { qk_rmsnorm(qx, (int64_t)B * N, nq, nk); qk_rmsnorm(qc, (int64_t)B * T, naq, nak); }
    Act ax = act((int64_t)B * N, C, N), ac = act((int64_t)B * T, C, T);
    {
      Op o; o.kind = OP_ATTN; o.batch = B; o.heads = c.num_heads; o.nq = N + T; o.nk = N + T; o.hd = c.head_dim;
      o.a = R(qx); o.k = Ref{SP_WS, qx.off + (int64_t)C * es}; o.v = Ref{SP_WS, qx.off + (int64_t)2 * C * es}; o.out = R(ax);
      o.q2 = R(qc); o.k2 = Ref{SP_WS, qc.off + (int64_t)C * es}; o.v2 = Ref{SP_WS, qc.off + (int64_t)2 * C * es}; o.out2 = R(ac);
      o.n1 = N; o.ldq = o.ldk = o.ldv = 3 * C; o.ldo = C; o.scale = 1.0f / sqrtf((float)c.head_dim);
      o.flops = 4.0 * (double)B * o.heads * (double)(N + T) * (double)(N + T) * o.hd;
      o.bytes = es * (double)B * (N + T) * C * 4.0;
      if (es == 4) snprintf(o.label, sizeof(o.label), u->mcfg.dtype == 3 ? "k_attention_x3/seg" : "k_attention_f32/seg");
      else snprintf(o.label, sizeof(o.label), "k_attn<%d>", o.hd);
      emit(o);
    }
    drop(qx); drop(qc);
    // image stream: x += gate_msa * to_out(attn);  x += gate_mlp * ff(LNmod(x))
    Act x2 = act((int64_t)B * N, C, N);
    gemm_ex(GemmSpec((int64_t)B * N, C, C, R(ax), ow, ob, R(x2)).with_residual(R(x)).with_rowgate(fcol(ci + 2 * C), N, fld(ci)));
    drop(ax);
    if (dual(i)) {
      // x2 += gate_msa2 * attn2.to_out(attn2(LN(x) (1 + scale_msa2) + shift_msa2)): self-attention over the image tokens alone;
      // both modulated inputs come from the block's input x, which therefore lives until here
      Act xn2 = act((int64_t)B * N, C, N);
      ln_mod(x, (int64_t)B * N, N, fcol(ci + 7 * C), fcol(ci + 6 * C), fld(ci), xn2);
      drop(x);
      Act q2 = act((int64_t)B * N, 3 * C, N);
      gemm_ex(GemmSpec((int64_t)B * N, 3 * C, C, R(xn2), q2w, q2b, R(q2)));
      drop(xn2);
      if (qkn) qk_rmsnorm(q2, (int64_t)B * N, n2q, n2k);
      Act a2 = act((int64_t)B * N, C, N);
      {
        Op o; o.kind = OP_ATTN; o.batch = B; o.heads = c.num_heads; o.nq = N; o.nk = N; o.hd = c.head_dim;
        o.a = R(q2); o.k = Ref{SP_WS, q2.off + (int64_t)C * es}; o.v = Ref{SP_WS, q2.off + (int64_t)2 * C * es}; o.out = R(a2);
        o.ldq = o.ldk = o.ldv = 3 * C; o.ldo = C; o.scale = 1.0f / sqrtf((float)c.head_dim);
        o.flops = 4.0 * (double)B * o.heads * (double)N * (double)N * o.hd;
        o.bytes = es * (double)B * N * C * 4.0;
        if (es == 4) snprintf(o.label, sizeof(o.label), u->mcfg.dtype == 3 ? "k_attention_x3" : "k_attention_f32");
        else snprintf(o.label, sizeof(o.label), "k_attn<%d>", o.hd);
        emit(o);
      }
      drop(q2);
      Act x2b = act((int64_t)B * N, C, N);
      gemm_ex(GemmSpec((int64_t)B * N, C, C, R(a2), o2w, o2b, R(x2b)).with_residual(R(x2)).with_rowgate(fcol(ci + 8 * C), N, fld(ci)));
      drop(a2); drop(x2);
      x2 = x2b;
    } else {
      drop(x);
    }
    Act xm = act((int64_t)B * N, C, N);
    ln_mod(x2, (int64_t)B * N, N, fcol(ci + 4 * C), fcol(ci + 3 * C), fld(ci), xm);
    Act hx = act((int64_t)B * N, 4 * C, N);
    gemm_ex(GemmSpec((int64_t)B * N, 4 * C, C, R(xm), f1w, f1b, R(hx)).with_act(SDN_ACT_GELU_TANH));
    drop(xm);
    Act x3 = act((int64_t)B * N, C, N);
    gemm_ex(GemmSpec((int64_t)B * N, C, 4 * C, R(hx), f2w, f2b, R(x3)).with_residual(R(x2)).with_rowgate(fcol(ci + 5 * C), N, fld(ci)));
    drop(hx); drop(x2);
    x = x3;
    // text stream (skipped in the last block: context_pre_only)
    if (!last) {
      Ref aow = param(nm(i, "attn.to_add_out.weight"), SDN_P_MAT, C, C), aob = param(nm(i, "attn.to_add_out.bias"), SDN_P_VEC_F32, C, 0);
      Ref g1w = param(nm(i, "ff_context.net.0.proj.weight"), SDN_P_MAT, 4 * C, C), g1b = param(nm(i, "ff_context.net.0.proj.bias"), SDN_P_VEC_F32, 4 * C, 0);
      Ref g2w = param(nm(i, "ff_context.net.2.weight"), SDN_P_MAT, C, 4 * C), g2b = param(nm(i, "ff_context.net.2.bias"), SDN_P_VEC_F32, C, 0);
      Act c2 = act((int64_t)B * T, C, T);
      gemm_ex(GemmSpec((int64_t)B * T, C, C, R(ac), aow, aob, R(c2)).with_residual(R(ctx)).with_rowgate(fcol(cc + 2 * C), T, fld(cc)));
      drop(ctx);
      Act cm = act((int64_t)B * T, C, T);
      ln_mod(c2, (int64_t)B * T, T, fcol(cc + 4 * C), fcol(cc + 3 * C), fld(cc), cm);
      Act hc = act((int64_t)B * T, 4 * C, T);
      gemm_ex(GemmSpec((int64_t)B * T, 4 * C, C, R(cm), g1w, g1b, R(hc)).with_act(SDN_ACT_GELU_TANH));
      drop(cm);
      Act c3 = act((int64_t)B * T, C, T);
      gemm_ex(GemmSpec((int64_t)B * T, C, 4 * C, R(hc), g2w, g2b, R(c3)).with_residual(R(c2)).with_rowgate(fcol(cc + 5 * C), T, fld(cc)));
      drop(hc); drop(c2);
      ctx = c3;
    } else {
      drop(ctx);
    }
    drop(ac);
  }
  // ---- norm_out (AdaLayerNormContinuous: scale, shift) + proj_out + unpatchify ----
  const int col_out = total - 2 * C;
  Act xo = act((int64_t)B * N, C, N);
  ln_mod(x, (int64_t)B * N, N, fcol(col_out), fcol(col_out + C), fld(col_out), xo);
  drop(x);
  const int PO = ps * ps * c.out_channels;
  Ref pw = param("proj_out.weight", SDN_P_MAT, PO, C), pb = param("proj_out.bias", SDN_P_VEC_F32, PO, 0);
  Act tok = act((int64_t)B * N, PO, N, 0, 4);
  gemm_ex(GemmSpec((int64_t)B * N, PO, C, R(xo), pw, pb, R(tok)).with_out_kind(SDN_OUT_F32));
  drop(xo);
  { Op o; o.kind = OP_UNPATCHIFY; o.batch = B; o.c1 = c.out_channels; o.hw = S; o.patch = ps; o.a = R(tok); o.out = Ref{SP_OUT, 0};
    o.bytes = (double)B * N * PO * 8.0; snprintf(o.label, sizeof(o.label), "k_unpatchify"); emit(o); }
  drop(tok);
  for (ModGroup& g : groups) drop(g.buf);
  plan->ws_bytes = arena.peak;
}

}  // namespace sdn_plan
