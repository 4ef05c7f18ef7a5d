// One staging pass of the GEMM epilogue; textually included with SDN_PASS = 0 / 1 (compile-time constant, so the
// accumulator array keeps constant indices and stays in registers).  See sdn_gemm.hip.
{
  constexpr int pass = SDN_PASS;
  if (pass > 0) __syncthreads();                             // previous pass fully stored before its LDS is reused
#ifndef SDN_EPI_RES_PRELOADED                                 // (sdn_ffn.hip fills the slab itself, under its trailing k-tiles)
  if (res_lds) {
    constexpr int CPR = BN / 8;                              // 16-byte chunks per row
    constexpr int RES_PIECES = ROWS_PER_PASS * CPR / 64 / NWAVES;
    static_assert(RES_PIECES * 64 * NWAVES == ROWS_PER_PASS * CPR, "residual slab must split into whole 1-KiB pieces per wave");
#pragma unroll
    for (int q = 0; q < RES_PIECES; ++q) {
      const int piece = wid * RES_PIECES + q;
      const int e = piece * 64 + lane;
      const int r = e / CPR, c = e - r * CPR;
      const int m = m0 + pass * ROWS_PER_PASS + r;
      const int rrow = g.residual_bcast ? m % g.rows_per_batch : m;
      const unsigned off = m < g.M ? (unsigned)(((long)rrow * g.ldc + n0 + c * 8) * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_res, (lds_ptr_t)(smem + piece * 1024), 16, off, 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#endif
  if (wm / WM_PER_PASS == pass) {
  // The mode is decided ONCE, outside the unrolled (i, j) loops: with every option tested inside each of the 40-80
  // fragment bodies the epilogue was ~25 k instructions of straight-line code per kernel, executed once per tile, i.e.
  // fetched past the instruction cache every time (in-kernel stamps: 7-33 k cycles to move the accumulators to LDS).
  if (g.x3_out) {
    // bf16x3 plan: the accumulators (bias + f32 residual already inside, see the kernel prologue) go straight to global memory --
    // f32 rows (16 B per lane, the four lane groups of a row fragment are 64 contiguous bytes), or bf16 hi | lo | hi triples
    // (the A operand of the next x3 GEMM: row = [hi(ldc) | lo(ldc) | hi(ldc)], 8 B per lane per plane).
    if (g.x3_out == 1) {
      float* outf = reinterpret_cast<float*>(g.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + pass * ROWS_PER_PASS + (wm % WM_PER_PASS) * 64 + i * 16 + fr;
        if (m < g.M) {
          float* op = outf + (long)m * g.ldc + n0 + wn * 16 * NREP + fq * 4;
#pragma unroll
          for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(op + j * 16) = acc[i][j];
        }
      }
    } else if (g.x3_out == 2) {                               // GEGLU (exact-erf GELU: this is the precision mode)
      unsigned short* out16 = reinterpret_cast<unsigned short*>(g.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + pass * ROWS_PER_PASS + (wm % WM_PER_PASS) * 64 + i * 16 + fr;
        if (m < g.M) {
          unsigned short* op = out16 + (long)m * 3 * g.ldc + (n0 >> 1) + fq * 4;
#pragma unroll
          for (int j = 0; j + 1 < NREP; j += 2) {
            const f32x4 hv = acc[i][j], gv = acc[i][j + 1];
            const f32x4 v = {hv[0] * gelu_erf_ref(gv[0]), hv[1] * gelu_erf_ref(gv[1]), hv[2] * gelu_erf_ref(gv[2]), hv[3] * gelu_erf_ref(gv[3])};
            uint2 hi, lo;
            split_hi_lo4(v, hi, lo);
            unsigned short* q = op + ((wn * 16 * NREP + j * 16) >> 1);
            *reinterpret_cast<uint2*>(q) = hi;
            *reinterpret_cast<uint2*>(q + g.ldc) = lo;
            *reinterpret_cast<uint2*>(q + 2 * g.ldc) = hi;
          }
        }
      }
    } else if (g.x3_out == 4) {                               // hi | lo PAIR rows [M, 2 ldc]: operands of the pre-split attention
      unsigned short* out16 = reinterpret_cast<unsigned short*>(g.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + pass * ROWS_PER_PASS + (wm % WM_PER_PASS) * 64 + i * 16 + fr;
        if (m < g.M) {
          unsigned short* op = out16 + (long)m * 2 * g.ldc + n0 + wn * 16 * NREP + fq * 4;
#pragma unroll
          for (int j = 0; j < NREP; ++j) {
            uint2 hi, lo;
            split_hi_lo4(acc[i][j], hi, lo);
            *reinterpret_cast<uint2*>(op + j * 16) = hi;
            *reinterpret_cast<uint2*>(op + j * 16 + g.ldc) = lo;
          }
        }
      }
    } else {
      unsigned short* out16 = reinterpret_cast<unsigned short*>(g.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + pass * ROWS_PER_PASS + (wm % WM_PER_PASS) * 64 + i * 16 + fr;
        if (m < g.M) {
          unsigned short* op = out16 + (long)m * 3 * g.ldc + n0 + wn * 16 * NREP + fq * 4;
#pragma unroll
          for (int j = 0; j < NREP; ++j) {
            uint2 hi, lo;
            split_hi_lo4(acc[i][j], hi, lo);
            *reinterpret_cast<uint2*>(op + j * 16) = hi;
            *reinterpret_cast<uint2*>(op + j * 16 + g.ldc) = lo;
            *reinterpret_cast<uint2*>(op + j * 16 + 2 * g.ldc) = hi;
          }
        }
      }
    }
  } else if constexpr (LNF) {                                 // LayerNorm folded in: v = rstd * (acc - mean * c[n]) + d[n]
    // (column fragment j OUTER: only its c / d vectors are live -- the 256 x 320 tile has no room for 2 x NREP of them)
    const float* cp = g.ln_c + n0 + wn * 16 * NREP + fq * 4;
    const float* dp = g.ln_d + n0 + wn * 16 * NREP + fq * 4;
    if (g.act == 2) {
#pragma unroll
      for (int j = 0; j + 1 < NREP; j += 2) {
        const f32x4 cv0 = *reinterpret_cast<const f32x4*>(cp + j * 16), cv1 = *reinterpret_cast<const f32x4*>(cp + (j + 1) * 16);
        const f32x4 dv0 = *reinterpret_cast<const f32x4*>(dp + j * 16), dv1 = *reinterpret_cast<const f32x4*>(dp + (j + 1) * 16);
        const int nl = ((wn * 16 * NREP + j * 16) >> 1) + fq * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ml = (wm % WM_PER_PASS) * 64 + i * 16 + fr;
          const float mu = ln_mu[i], rs = ln_rs[i];
          const f32x4 hv = (acc[i][j] - mu * cv0) * rs + dv0, gv = (acc[i][j + 1] - mu * cv1) * rs + dv1;
          uint2 pk;
          pk.x = T::pack2(hv[0] * gelu_erf(gv[0]), hv[1] * gelu_erf(gv[1]));
          pk.y = T::pack2(hv[2] * gelu_erf(gv[2]), hv[3] * gelu_erf(gv[3]));
          *reinterpret_cast<uint2*>(smem + ml * CW_PAD + nl * 2) = pk;
        }
      }
    } else {
      unsigned char* slot0 = smem + ((wm % WM_PER_PASS) * 64 + fr) * CW_PAD + (wn * 16 * NREP + fq * 4) * 2;
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const f32x4 cvj = *reinterpret_cast<const f32x4*>(cp + j * 16), dvj = *reinterpret_cast<const f32x4*>(dp + j * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 v = (acc[i][j] - ln_mu[i] * cvj) * ln_rs[i] + dvj;
          uint2 pk; pk.x = T::pack2(v[0], v[1]); pk.y = T::pack2(v[2], v[3]);
          *reinterpret_cast<uint2*>(slot0 + i * 16 * CW_PAD + j * 32) = pk;
        }
      }
    }
  } else if (g.act == 2 && (g.dbg & 16)) {                    // timing-only ablation: GEGLU with a free GELU
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ml = (wm % WM_PER_PASS) * 64 + i * 16 + fr;
#pragma unroll
      for (int j = 0; j + 1 < NREP; j += 2) {
        const f32x4 hv = acc[i][j], gv = acc[i][j + 1];
        uint2 pk;
        pk.x = T::pack2(hv[0] * gv[0], hv[1] * gv[1]);
        pk.y = T::pack2(hv[2] * gv[2], hv[3] * gv[3]);
        const int nl = ((wn * 16 * NREP + j * 16) >> 1) + fq * 4;
        *reinterpret_cast<uint2*>(smem + ml * CW_PAD + nl * 2) = pk;
      }
    }
  } else if (g.act == 2 && g.glu_tanh) {                      // gated tanh-GELU (T5 gelu_new): same column pairs, same half-width tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ml = (wm % WM_PER_PASS) * 64 + i * 16 + fr;
#pragma unroll
      for (int j = 0; j + 1 < NREP; j += 2) {
        const f32x4 hv = acc[i][j], gv = acc[i][j + 1];
        uint2 pk;
        pk.x = T::pack2(hv[0] * gelu_tanh(gv[0]), hv[1] * gelu_tanh(gv[1]));
        pk.y = T::pack2(hv[2] * gelu_tanh(gv[2]), hv[3] * gelu_tanh(gv[3]));
        const int nl = ((wn * 16 * NREP + j * 16) >> 1) + fq * 4;
        *reinterpret_cast<uint2*>(smem + ml * CW_PAD + nl * 2) = pk;
      }
    }
  } else if (g.act == 2) {                                    // GEGLU: value / gate column pairs -> half-width tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ml = (wm % WM_PER_PASS) * 64 + i * 16 + fr;
#pragma unroll
      for (int j = 0; j + 1 < NREP; j += 2) {
        const f32x4 hv = acc[i][j], gv = acc[i][j + 1];
        uint2 pk;
        pk.x = T::pack2(hv[0] * gelu_erf(gv[0]), hv[1] * gelu_erf(gv[1]));
        pk.y = T::pack2(hv[2] * gelu_erf(gv[2]), hv[3] * gelu_erf(gv[3]));
        const int nl = ((wn * 16 * NREP + j * 16) >> 1) + fq * 4;        // column inside the (half-width) tile
        *reinterpret_cast<uint2*>(smem + ml * CW_PAD + nl * 2) = pk;
      }
    }
  } else if (lean && res_lds) {                               // 16-bit staged output, + residual already in the slab
    unsigned char* slot0 = smem + ((wm % WM_PER_PASS) * 64 + fr) * (BN * 2) + (wn * 16 * NREP + fq * 4) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        uint2* slot = reinterpret_cast<uint2*>(slot0 + i * 16 * (BN * 2) + j * 32);
        const uint2 rr = *slot;
        const f32x4 v = acc[i][j];
        uint2 pk;
        pk.x = T::pack2(v[0] + T::to_f(rr.x & 0xffff), v[1] + T::to_f(rr.x >> 16));
        pk.y = T::pack2(v[2] + T::to_f(rr.y & 0xffff), v[3] + T::to_f(rr.y >> 16));
        *slot = pk;
      }
  } else if (lean) {                                          // 16-bit staged output, nothing to add
    unsigned char* slot0 = smem + ((wm % WM_PER_PASS) * 64 + fr) * CW_PAD + (wn * 16 * NREP + fq * 4) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const f32x4 v = acc[i][j];
        uint2 pk; pk.x = T::pack2(v[0], v[1]); pk.y = T::pack2(v[2], v[3]);
        *reinterpret_cast<uint2*>(slot0 + i * 16 * CW_PAD + j * 32) = pk;
      }
  } else if (lean_gelu) {                                     // 16-bit staged output of tanh-GELU (MMDiT feed-forward)
    unsigned char* slot0 = smem + ((wm % WM_PER_PASS) * 64 + fr) * CW_PAD + (wn * 16 * NREP + fq * 4) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const f32x4 v = acc[i][j];
        uint2 pk; pk.x = T::pack2(gelu_tanh(v[0]), gelu_tanh(v[1])); pk.y = T::pack2(gelu_tanh(v[2]), gelu_tanh(v[3]));
        *reinterpret_cast<uint2*>(slot0 + i * 16 * CW_PAD + j * 32) = pk;
      }
  } else if (lean_erf) {                                      // 16-bit staged output of erf-GELU (OpenCLIP bigG's MLP)
    unsigned char* slot0 = smem + ((wm % WM_PER_PASS) * 64 + fr) * CW_PAD + (wn * 16 * NREP + fq * 4) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const f32x4 v = acc[i][j];
        uint2 pk; pk.x = T::pack2(gelu_erf(v[0]), gelu_erf(v[1])); pk.y = T::pack2(gelu_erf(v[2]), gelu_erf(v[3]));
        *reinterpret_cast<uint2*>(slot0 + i * 16 * CW_PAD + j * 32) = pk;
      }
  } else if (lean_gate) {                                     // adaLN-zero: out = residual + gate[sample] * (acc)
    unsigned char* slot0 = smem + ((wm % WM_PER_PASS) * 64 + fr) * (BN * 2) + (wn * 16 * NREP + fq * 4) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + pass * ROWS_PER_PASS + (wm % WM_PER_PASS) * 64 + i * 16 + fr;
      const int b = m < g.M ? m / g.rows_per_batch : 0;
      const float* gp = g.rowgate + (long)b * g.ld_rowgate + n0 + wn * 16 * NREP + fq * 4;
      f32x4 gt[NREP];
#pragma unroll
      for (int j = 0; j < NREP; ++j) gt[j] = *reinterpret_cast<const f32x4*>(gp + j * 16);
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        uint2* slot = reinterpret_cast<uint2*>(slot0 + i * 16 * (BN * 2) + j * 32);
        const uint2 rr = *slot;
        const f32x4 v = acc[i][j] * gt[j];
        uint2 pk;
        pk.x = T::pack2(v[0] + T::to_f(rr.x & 0xffff), v[1] + T::to_f(rr.x >> 16));
        pk.y = T::pack2(v[2] + T::to_f(rr.y & 0xffff), v[3] + T::to_f(rr.y >> 16));
        *slot = pk;
      }
    }
  } else {                                                    // everything else (SiLU, fp32 / ragged outputs, unaligned residual)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ml = (wm % WM_PER_PASS) * 64 + i * 16 + fr;    // row inside this pass's staged slab
    const int m = m0 + pass * ROWS_PER_PASS + ml;
    const bool row_ok = m < g.M;
    const int b = (g.rows_per_batch > 0 && row_ok) ? m / g.rows_per_batch : 0;
    unsigned short* out16 = reinterpret_cast<unsigned short*>(g.out);
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int nl = wn * 16 * NREP + j * 16 + fq * 4;
      const int n = n0 + nl;
      f32x4 v = acc[i][j];
      if (g.rowgate && row_ok) {                              // adaLN-zero gate: per-sample vector, applied before the residual
        const float4 gt = *reinterpret_cast<const float4*>(g.rowgate + (long)b * g.ld_rowgate + n);
        v[0] *= gt.x; v[1] *= gt.y; v[2] *= gt.z; v[3] *= gt.w;
      }
      if (res_lds) {
        const uint2 rr = *reinterpret_cast<const uint2*>(smem + ml * CW + nl * 2);
        v[0] += T::to_f(rr.x & 0xffff); v[1] += T::to_f(rr.x >> 16); v[2] += T::to_f(rr.y & 0xffff); v[3] += T::to_f(rr.y >> 16);
      } else if (g.residual && row_ok) {
        const long rrow = g.residual_bcast ? (long)(m - b * g.rows_per_batch) : (long)m;     // bcast: same rows for every sample
        const uint2 rr = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(g.residual) + rrow * g.ldc + n);
        v[0] += T::to_f(rr.x & 0xffff); v[1] += T::to_f(rr.x >> 16); v[2] += T::to_f(rr.y & 0xffff); v[3] += T::to_f(rr.y >> 16);
      }
      if (g.act == 1) { v[0] = silu_f(v[0]); v[1] = silu_f(v[1]); v[2] = silu_f(v[2]); v[3] = silu_f(v[3]); }
      if (g.act == 3) { v[0] = gelu_tanh(v[0]); v[1] = gelu_tanh(v[1]); v[2] = gelu_tanh(v[2]); v[3] = gelu_tanh(v[3]); }
      if (g.act == 4) { v[0] = quick_gelu(v[0]); v[1] = quick_gelu(v[1]); v[2] = quick_gelu(v[2]); v[3] = quick_gelu(v[3]); }
      if (staged) {
        uint2 pk; pk.x = T::pack2(v[0], v[1]); pk.y = T::pack2(v[2], v[3]);
        *reinterpret_cast<uint2*>(smem + ml * CW + nl * 2) = pk;
      } else if (!row_ok) {
      } else if (g.out_kind == 0) {
        for (int e = 0; e < 4; ++e)
          if (n + e < g.n_valid) out16[(long)m * g.ldc + n + e] = (unsigned short)(T::pack2(v[e], 0.f) & 0xffff);
      } else if (g.out_kind == 1) {
        float* outf = reinterpret_cast<float*>(reinterpret_cast<char*>(g.out) + (long)blockIdx.y * g.split_stride);   // split-K slice
        if (g.n_valid == g.N && (g.ldc & 3) == 0) {
          *reinterpret_cast<f32x4*>(outf + (long)m * g.ldc + n) = v;
        } else {
          for (int e = 0; e < 4; ++e)
            if (n + e < g.n_valid) outf[(long)m * g.ldc + n + e] = v[e];
        }
      } else {
        const int p = m - b * g.rows_per_batch;
        for (int e = 0; e < 4; ++e)
          if (n + e < g.n_valid)
            reinterpret_cast<float*>(g.out)[((long)b * g.n_valid + n + e) * g.rows_per_batch + p] = v[e];
      }
    }
  }
  }
  }  // waves of this pass
  if (pass == 0) SDN_STAMP(4)
  if ((staged || g.act == 2) && !g.x3_out) {
    __syncthreads();
    if (pass == 0) SDN_STAMP(5)
    const int cpr = out_cols / 8;                            // 16-byte chunks per staged row
    const int col0 = g.act == 2 ? (n0 >> 1) : n0;
    unsigned short* out16 = reinterpret_cast<unsigned short*>(g.out);
    for (int e = tid; e < ROWS_PER_PASS * cpr; e += THREADS) {
      const int r = e / cpr, c = e - r * cpr;
      const int m = m0 + pass * ROWS_PER_PASS + r;
#ifdef SDN_EPI_OUT_ROW                                        // (k_gemm_up4: GEMM row -> row of the upsampled map)
      // ONLY this staged store remaps rows: the direct stores above (f32 / NCHW / ragged / x3 outputs) index by GEMM row, so the
      // phase mode must never reach them -- sdn_gemm_impl admits it with a whole-width 16-bit output only; relax that check and these paths need the remap too
      if (m < g.M && !(g.dbg & 1))
        *reinterpret_cast<u32x4*>(out16 + (long)SDN_EPI_OUT_ROW(m) * g.ldc + col0 + c * 8) = *reinterpret_cast<const u32x4*>(smem + r * CW + c * 16);
#else
      if (m < g.M && !(g.dbg & 1))
        *reinterpret_cast<u32x4*>(out16 + (long)m * g.ldc + col0 + c * 8) = *reinterpret_cast<const u32x4*>(smem + r * CW + c * 16);
#endif
    }
    // (after the stores have been issued: they drain while the sums are taken)
    if (g.col_stats) {                                       // column sums of this pass's staged slab (16-bit values, as stored)
      // a thread sums one 16-byte chunk (8 columns) over a stride of rows; the RG row groups are combined through a
      // scratch area at the top of the (free) LDS, then BN threads write the block's partials
      constexpr int CPR = BN / 8, RG = 8;              // RG is the SAME for every tile family: the fp32 summation order of a
                                                       // block's 128 rows (and so the GroupNorm) must not depend on the tile the
                                                       // batch size happened to select
      static_assert(RG * CPR <= THREADS, "column-sum mapping needs RG * CPR threads");
      float* scr = reinterpret_cast<float*>(smem + NSTAGE * STAGE - RG * BN * 8);
      static_assert(NSTAGE * STAGE - RG * BN * 8 >= ROWS_PER_PASS * CW_PAD, "column-sum scratch must not overlap the staged slab");
      int rows_here = g.M - (m0 + pass * ROWS_PER_PASS);
      rows_here = rows_here > ROWS_PER_PASS ? ROWS_PER_PASS : rows_here;
      if (tid < RG * CPR) {
        const int rg = tid / CPR, c = tid - rg * CPR;
        float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int r = rg; r < rows_here; r += RG) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(smem + r * CW + c * 16);
          const unsigned w4[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float lo = T::to_f(w4[k] & 0xffff), hi = T::to_f(w4[k] >> 16);
            cs[2 * k] += lo; cq[2 * k] = fmaf(lo, lo, cq[2 * k]);
            cs[2 * k + 1] += hi; cq[2 * k + 1] = fmaf(hi, hi, cq[2 * k + 1]);
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float2*>(scr + 2 * (rg * BN + c * 8 + k)) = make_float2(cs[k], cq[k]);
      }
      __syncthreads();
      if (tid < BN && rows_here > 0) {
        float ts = 0.f, tq = 0.f;
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) { const float2 v = *reinterpret_cast<const float2*>(scr + 2 * (rg * BN + tid)); ts += v.x; tq += v.y; }
        const long blk = (long)(m0 / 128) + pass * (ROWS_PER_PASS / 128);
        *reinterpret_cast<float2*>(g.col_stats + 2 * (blk * g.N + n0 + tid)) = make_float2(ts, tq);
      }
    }
    if (pass == 0) SDN_STAMP(6)
  }
}
