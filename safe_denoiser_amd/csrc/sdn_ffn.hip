// GEGLU feed-forward of a C = 320 transformer block as ONE kernel (rows U5 / U4, the 64 x 64 level of SD-v1.4):
//
//   out = x + [ GEGLU(LN3(h3) W1^T + b1) | h3 ] . [ Wpo W2 | Wpo ]^T + (Wpo b2 + bpo)
//
// i.e. LayerNorm-folded GEGLU projection (sdn_gemm_ln_*, N = 8C) followed by the FeedForward output linear already
// contracted with the block's proj_out (two-source GEMM, K = 5C) -- what sdn_plan_unet.hip emitted as two launches.  Between
// them sat the [M, 4C] hidden tensor: 1.34 GB written and re-read per block at B = 128 samples, and ablations of the two
// launches (tools/bench_gemm.py, VARIANTS=0,32,16: in-loop DMA off / stores off) put 23-38 % of their time on exactly that
// traffic and on the L2 -> LDS re-streaming of A by 20 column tiles (13.4 GB per launch, 60 % of what the L2s can deliver).
// Here a workgroup keeps a 128-row block of h3 in LDS for its whole life and the hidden activation never leaves the CU:
//
//   X      [128 x 320]  h3 rows, 5 swizzled k-tile images (80 KB), loaded once: A operand of the projection AND of the
//                       trailing [h3 | Wpo] k-tiles
//   for each chunk of 64 hidden units (20 chunks; = 128 value/gate-interleaved columns of W1):
//       acc1[128 x 128]  = X . W1_chunk^T           5 k-tiles of W1 (16 KB each)
//       H[128 x 64]      = (LN fold) value * gelu(gate), 16 bit, written as ONE k-tile image into a 16 KB buffer of its own
//       acc[128 x 320] += H . Wcat[:, chunk]^T      the 40 KB k-tile of the contracted output weight, by column fragments
//   acc += X . Wcat[:, 4C:]^T (5 k-tiles, double-buffered), + bias + residual x -> staged 16-bit store (+ GroupNorm column sums)
//
// 8 waves as 2 (M) x 4 (N): a wave owns 64 x 32 of acc1 (one value/gate fragment pair -> 16 hidden columns) and 64 x 80 of
// acc.  Per 128 rows the L2 -> LDS traffic is 2.7 MB for 682 MFLOP (4 B/kFLOP against 15.6 for the 128 x 128 projection tile).
//
// All weights of the chunk loop arrive through ONE ring of four 16 KB stages, requested three slots ahead.  A chunk is 8 slots of
// (at most) 16 MFMAs per wave, each reading one ring entry: u = 0..4 the W1 k-tiles, u = 5, 6, 7 the contraction k-tile cut by
// output columns -- fragments {0, 1}, {2, 3}, {4} of every wave's 80 columns (16 + 16 + 8 KB; both k-steps of a fragment inside
// its slot, so an accumulator still sees k-step 0, then 1).  Entry u lives in stage u & 3; the request for entry u + 3 is issued
// at the top of slot u, so it has three slots (>= 1500 MFMA cycles at two waves per SIMD) to land.
// LDS: X 80 KB | ring 4 x 16 KB | H 16 KB = 160 KB; the tail reuses ring + H as its two 40 KB weight buffers.
//
// Arithmetic is IDENTICAL to the two-launch path, bit for bit: same k order per output element (16x16x32 MFMA chains over
// k-tiles 0..4 for the projection, 0..24 for the contraction, accumulators started from the bias), same LayerNorm-fold /
// GELU / pack expressions, same residual add, same row-group order of the column sums -- tests/test_gpu_ops.py and
// tests/test_gpu_ffn_ring.py check equality.
//
// LDS hazards, in program order (every wave executes the same sequence; E(u) = ring entry u of the current chunk, E(8..10) =
// E(0..2) of the next; pieces per wave: 2 per entry, 1 for E(7)):
//   prologue   X, E(0), E(1), E(2) requested; vmcnt(0) + barrier.
//   slot u     top: request E(u + 3) into stage (u + 3) & 3 = (u - 1) & 3, last read in slot u - 1, which ended with a barrier
//              (slot 0: the previous chunk's slot 7).  For slot 5 the request is issued before the GEGLU arithmetic.
//              Slot 0 first issues the 4 fold-coefficient loads of the chunk (plain loads: they count in vmcnt, between E(2), E(3)).
//              end: E(u + 1) must have landed; E(u + 2), E(u + 3) may stay in flight:
//                  u = 0: vmcnt(8) (E(2), the 4 coefficient loads, E(3)) | 1, 2, 3: vmcnt(4) | 4: vmcnt(3) (E(6), E(7)) |
//                  5: vmcnt(3) (E(7), E(8)) | 6, 7: vmcnt(4).  The last chunk has no E(8..10): its slots 5..7 wait for vmcnt(0).
//              then lgkmcnt(0) (this wave's fragment reads of stage u & 3 are done) and the barrier: every wave's pieces of
//              E(u + 1) are visible, stage u & 3 may be refilled.
//   H          written after slot 4's barrier, read (into registers, for all three contraction slots) in slot 5 only: its readers
//              are behind slot 5's barrier, a whole chunk before the next write.  lgkmcnt(0) + a raw barrier publish it; neither
//              that barrier nor the store may wait for vmcnt (the store is an asm statement for that reason, see there).
//   tail       starts behind the last chunk's vmcnt(0) + barrier: nothing in flight, no reader left in ring or H.
#include "sdn_gemm_common.h"

namespace sdn_gemm_detail {

#define SDN_STAMP(IDX) {}
// Diagnostics build (-DSDN_FFN_STAMPS, `make stamps`, tools/ffn_stamps.py): per-wave cycle sums of the chunk loop's phases.
#ifdef SDN_FFN_STAMPS
__device__ unsigned long long* g_ffn_stamps = nullptr;
#define SDN_FTS_DECL unsigned long long fts_prev = 0, fts_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define SDN_FTS_MARK(I)                                                                         \
  {                                                                                             \
    unsigned long long t_;                                                                      \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                  \
    if ((I) >= 0) fts_sum[(I) < 0 ? 0 : (I)] += t_ - fts_prev;                                  \
    fts_prev = t_;                                                                              \
  }
#define SDN_FTS_FLUSH                                                                           \
  if (g_ffn_stamps && lane == 0)                                                                \
    for (int i_ = 0; i_ < 8; ++i_) g_ffn_stamps[((long)blockIdx.x * 8 + wid) * 8 + i_] = fts_sum[i_];
#else
#define SDN_FTS_DECL
#define SDN_FTS_MARK(I)
#define SDN_FTS_FLUSH
#endif

struct FfnArgs {
  const void* x;            // h3 [M, C] 16 bit
  const float* stats;       // [M][2] (mean, rstd) of the rows of x (sdn_row_stats_*); nullptr = taken from the A fragments of the
                            // first chunk's projection (k_gemm_dma's LNF = 1 arithmetic, eps = 1e-5: no pre-pass over x)
  const void* w1;           // [8C, C] 16 bit: value/gate rows interleaved in groups of 16, LayerNorm gamma folded in
  const float* c1; const float* d1;   // [8C] fold coefficients (sdn_ln_fold)
  const void* w2;           // [C, 5C] 16 bit: [Wpo W2 | Wpo]
  const float* b2;          // [C]
  const void* residual;     // [M, C] 16 bit
  void* out;                // [M, C] 16 bit
  float* col_stats;         // nullable: [ceil(M / 128)][C][2]
  int M;
};

// acc[4][5] += A[64 x 64] . W[80 x 64]^T for one k-tile: the W fragments are consumed in groups of two (2, 2, 1 per k-step) and
// the next group's ds_reads are issued ahead of the current group's MFMAs (as in the 256 x 320 GEMM tile).
#define SDN_FFN_CONTRACT(SA, SW)                                                                                           \
      {                                                                                                                    \
        typename T::v8 fa[2][4], fw[2][2];                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                      \
          fa[0][i] = *reinterpret_cast<const typename T::v8*>((SA) + lds_off(i * 16 + fr, fq));                            \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                      \
          fw[0][j] = *reinterpret_cast<const typename T::v8*>((SW) + lds_off(j * 16 + fr, fq));                            \
        _Pragma("unroll") for (int gi = 0; gi < 6; ++gi) {                                                                 \
          const int ks = gi / 3, g = gi % 3, nj = g == 2 ? 1 : 2;                                                          \
          if (gi + 1 < 6) {                                                                                                \
            const int ks1 = (gi + 1) / 3, g1 = (gi + 1) % 3, nj1 = g1 == 2 ? 1 : 2;                                        \
            _Pragma("unroll") for (int j = 0; j < nj1; ++j)                                                                \
              fw[(gi + 1) & 1][j] = *reinterpret_cast<const typename T::v8*>((SW) + lds_off((2 * g1 + j) * 16 + fr, ks1 * 4 + fq)); \
          }                                                                                                                \
          if (gi == 1) {                                                                                                   \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                  \
              fa[1][i] = *reinterpret_cast<const typename T::v8*>((SA) + lds_off(i * 16 + fr, 4 + fq));                    \
          }                                                                                                                \
          __builtin_amdgcn_s_setprio(1);                                                                                   \
          _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                    \
            _Pragma("unroll") for (int j = 0; j < nj; ++j)                                                                 \
              acc[i][2 * g + j] = T::mfma16(fw[gi & 1][j], fa[ks][i], acc[i][2 * g + j]);                                  \
          __builtin_amdgcn_s_setprio(0);                                                                                   \
        }                                                                                                                  \
      }

template <typename T>
__global__ void __launch_bounds__(512, 1)
k_ffn320(const FfnArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int C = 320, HID = 4 * C, KT1 = C / BK, NCH = HID / 64, KT2 = NCH + KT1;      // 5 / 20 chunks / 25 contraction k-tiles
  constexpr int BM = 128, BN = C, THREADS = 512, NWAVES = 8, NREP = 5;
  constexpr int XIMG = BM * 128;                             // one k-tile image of X or H, one ring stage: 16 KB
  constexpr int W2IMG = C * 128;                             // one whole k-tile of the contraction weight (tail): 40 KB
  constexpr int NSLOT = 8, NRING = 4;                        // slots per chunk (5 W1 k-tiles + W2 slices A, B, C), ring stages
  constexpr int OFF_RING = KT1 * XIMG;                       // 81920: ring stages 0..3 (16 KB each)
  constexpr int OFF_H = OFF_RING + NRING * XIMG;             // 147456: H (16 KB)
  constexpr int OFF_TA = OFF_RING, OFF_TB = OFF_RING + W2IMG;   // tail: the same 80 KB as two 40 KB weight buffers
  constexpr int LDS_BYTES = OFF_H + XIMG;                    // 163840
  static_assert(OFF_TB + W2IMG == LDS_BYTES && NSLOT % NRING == 0, "ring + H = the tail's two weight buffers; stage = slot & 3");
  constexpr unsigned OOB = 0x80000000u;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  SDN_FTS_DECL
  SDN_FTS_MARK(-1)
  const int wm = wid >> 2, wn = wid & 3;
  const int lrow = lane >> 3, lchunk = (lane & 7) ^ lrow;
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * BM, n0 = 0;

  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(a.x, (unsigned)((long)a.M * C * 2));
  const __amdgpu_buffer_rsrc_t rs_w1 = make_rsrc(a.w1, (unsigned)(2 * HID * C * 2));
  const __amdgpu_buffer_rsrc_t rs_w2 = make_rsrc(a.w2, (unsigned)(C * (HID + C) * 2));

  // ---- X: 80 pieces of 1 KiB (k-tile image kt = p / 16, rows 8 (p % 16) ..), 10 per wave ----
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    const int p = wid * 10 + q;
    const int kt = p >> 4, rg = p & 15;
    const int m = m0 + rg * 8 + lrow;
    const unsigned off = m < a.M ? (unsigned)(((long)m * C + kt * BK + lchunk * 8) * 2) : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(smem + p * 1024), 16, off, 0, 0, 0);
  }
  // Ring entry `u` of chunk jc (slot 8 jc + u) -> stage u & 3.  u = 0..4: projection weight k-tile u (16 pieces, 2 per wave);
  // u = 5, 6: rows wn 80 + (u - 5) 32 .. + 31 of the chunk's contraction k-tile for every wn (fragments 0, 1 / 2, 3 of each wave
  // column: 16 pieces, 2 per wave, stage row = wn 32 + local row); u = 7: rows wn 80 + 64 .. + 15 (fragment 4: 8 pieces, 1 per wave,
  // stage row = wn 16 + local row).  u >= 8 names the next chunk's entry u - 8; past the last chunk nothing is issued.
  const unsigned w1_lane = (unsigned)(((wid * 2 * 8 + lrow) * C + lchunk * 8) * 2);
  const unsigned w2ab_lane = (unsigned)((((wid >> 1) * 16 * NREP + (wid & 1) * 16 + lrow) * (HID + C) + lchunk * 8) * 2);
  const unsigned w2c_lane = (unsigned)((((wid >> 1) * 16 * NREP + 64 + (wid & 1) * 8 + lrow) * (HID + C) + lchunk * 8) * 2);
  auto issue_slot = [&](int jc, int u) {
    if (u >= NSLOT) { u -= NSLOT; ++jc; }
    if (jc >= NCH) return;
    unsigned char* stage = smem + OFF_RING + (u & (NRING - 1)) * XIMG;
    if (u < KT1) {
      const unsigned base = w1_lane + (unsigned)((jc * 128 * C + u * BK) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, (lds_ptr_t)(stage + wid * 2048), 16, base, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, (lds_ptr_t)(stage + wid * 2048 + 1024), 16, base + (unsigned)(8 * C * 2), 0, 0, 0);
    } else if (u < NSLOT - 1) {
      const unsigned base = w2ab_lane + (unsigned)(((u - KT1) * 32 * (HID + C) + jc * BK) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, (lds_ptr_t)(stage + wid * 2048), 16, base, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, (lds_ptr_t)(stage + wid * 2048 + 1024), 16, base + (unsigned)(8 * (HID + C) * 2), 0, 0, 0);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, (lds_ptr_t)(stage + wid * 1024), 16, w2c_lane + (unsigned)(jc * BK * 2), 0, 0, 0);
    }
  };
  // contraction weight k-tile t as a whole (tail): 40 pieces, 5 per wave; slice q of a wave = piece wid * 5 + q
  const unsigned w2_lane = (unsigned)(((wid * 5 * 8 + lrow) * (HID + C) + lchunk * 8) * 2);
  auto issue_w2_slice = [&](int t, int q, int buf_off) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, (lds_ptr_t)(smem + buf_off + (wid * 5 + q) * 1024), 16,
                                             w2_lane + (unsigned)((q * 8 * (HID + C) + t * BK) * 2), 0, 0, 0);
  };

  issue_slot(0, 0); issue_slot(0, 1); issue_slot(0, 2);
  // accumulators of the contraction start from the bias; row statistics of this wave's rows
  f32x4 acc[4][NREP];
  {
    f32x4 bv[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) bv[j] = *reinterpret_cast<const f32x4*>(a.b2 + wn * 16 * NREP + j * 16 + fq * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) acc[i][j] = bv[j];
  }
  float ln_mu[4] = {0.f, 0.f, 0.f, 0.f}, ln_rs[4] = {0.f, 0.f, 0.f, 0.f};
  const bool own_stats = a.stats == nullptr;                    // wave-uniform
  if (!own_stats) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      const float2 st2 = *reinterpret_cast<const float2*>(a.stats + 2 * (long)(m < a.M ? m : 0));
      ln_mu[i] = st2.x; ln_rs[i] = st2.y;
    }
  }
  float ln_s1[4] = {0.f, 0.f, 0.f, 0.f}, ln_s2[4] = {0.f, 0.f, 0.f, 0.f};   // own_stats: per-row sum / sum of squares (chunk 0 only)
  // fold coefficients of this wave's value / gate fragment pair
  f32x4 cv[2], dv[2];
  auto load_cd = [&](int jc) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = jc * 128 + wn * 32 + j * 16 + fq * 4;
      cv[j] = *reinterpret_cast<const f32x4*>(a.c1 + n); dv[j] = *reinterpret_cast<const f32x4*>(a.d1 + n);
    }
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const unsigned char* sa_x = smem + (wm * 64) * 128;                       // + kt * XIMG
  SDN_FTS_MARK(0)                                                           // prologue: X + first W1 k-tile landed
  for (int jc = 0; jc < NCH; ++jc) {
    const bool last = jc == NCH - 1;                                         // wave-uniform: entries 8..10 of the last chunk do not exist
    f32x4 acc1[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc1[i][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc1[i][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    // ---- projection: 5 k-tiles (slots u = 0..4) ----
#pragma unroll
    for (int kt = 0; kt < KT1; ++kt) {
      if (kt == 0) load_cd(jc);                                              // 4 loads, used after the k loop; counted in slot 0's wait
      issue_slot(jc, kt + 3);
      const unsigned char* sa = sa_x + kt * XIMG;
      const unsigned char* sw = smem + OFF_RING + (kt & (NRING - 1)) * XIMG + (wn * 32) * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        typename T::v8 fa[4], fw[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const typename T::v8*>(sa + lds_off(i * 16 + fr, ks * 4 + fq));
#pragma unroll
        for (int j = 0; j < 2; ++j) fw[j] = *reinterpret_cast<const typename T::v8*>(sw + lds_off(j * 16 + fr, ks * 4 + fq));
        if (own_stats && jc == 0) {                              // the first chunk's k loop passes every column of this wave's rows
#pragma unroll
          for (int i = 0; i < 4; ++i) { ln_s1[i] = T::dot_ones(fa[i], ln_s1[i]); ln_s2[i] = T::dot_self(fa[i], ln_s2[i]); }
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc1[i][j] = T::mfma16(fw[j], fa[i], acc1[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
      SDN_FTS_MARK(1)                                                        // projection: DMA issue + fragment reads + MFMAs issued
      // entry kt + 1 has landed; entries kt + 2 and kt + 3 (2 pieces each, 1 for entry 7) stay in flight -- and in slot 0 the
      // 4 fold-coefficient loads, which sit between them in issue order
      if (kt == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (kt < KT1 - 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     // fragment reads done before the stage is refilled
      SDN_FTS_MARK(2)                                                        // ... wait for the next k-tile
      __builtin_amdgcn_s_barrier();
      SDN_FTS_MARK(3)                                                        // ... barrier
    }
    issue_slot(jc, KT1 + 3);                                                 // slot 5's request, ahead of the GEGLU arithmetic
    if (own_stats && jc == 0) {                                  // as k_gemm_dma (LNF = 1): the other three lane groups hold the rest of a row
      const float invk = 1.0f / (float)C;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float a1 = ln_s1[i], a2 = ln_s2[i];
        a1 += __shfl_xor(a1, 16, 64); a2 += __shfl_xor(a2, 16, 64);
        a1 += __shfl_xor(a1, 32, 64); a2 += __shfl_xor(a2, 32, 64);
        const float mu = a1 * invk;
        const float var = fmaxf(a2 * invk - mu * mu, 0.f);
        ln_mu[i] = mu; ln_rs[i] = __builtin_amdgcn_rsqf(var + 1e-5f);
      }
    }
    // ---- GEGLU: LayerNorm fold, value * gelu(gate), 16 bit -> H (a k-tile image of its own) ----
    unsigned char* sh = smem + OFF_H;
    unsigned h_addr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wm * 64 + i * 16 + fr;
      const float mu = ln_mu[i], rs = ln_rs[i];
      const f32x4 hv = (acc1[i][0] - mu * cv[0]) * rs + dv[0], gv = (acc1[i][1] - mu * cv[1]) * rs + dv[1];
      uint2 pk;
      pk.x = T::pack2(hv[0] * gelu_erf(gv[0]), hv[1] * gelu_erf(gv[1]));
      pk.y = T::pack2(hv[2] * gelu_erf(gv[2]), hv[3] * gelu_erf(gv[3]));
      if (i == 0) h_addr = (unsigned)(unsigned long)(lds_ptr_t)(sh + lds_off(row, wn * 2 + (fq >> 1)) + (fq & 1) * 8);
      // stored from an asm statement: before a ds_write of its own the compiler waits for vmcnt(0) (LDS-DMA may alias it), which
      // would drain the ring here once per chunk.  Rows i 16 + .. share the swizzle of row 0 + ..: 2 KiB apart
      asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(h_addr), "v"((unsigned long long)pk.y << 32 | pk.x), "i"(i * 16 * 128) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                       // the H stores above are not counted by the compiler
    SDN_FTS_MARK(4)                                                          // GEGLU epilogue (waits for the MFMAs)
    __builtin_amdgcn_s_barrier();                                            // H visible (raw: __syncthreads would drain the ring)
    asm volatile("" ::: "memory");
    SDN_FTS_MARK(5)                                                          // barrier
    // ---- contraction with this chunk's k-tile, by column fragments: slots 5, 6, 7 = fragments {0, 1}, {2, 3}, {4} of each wave,
    //      both k-steps of a fragment inside its slot (per accumulator: k-step 0, then 1, as in the whole-tile form) ----
    {
      typename T::v8 fa[2][4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          fa[ks][i] = *reinterpret_cast<const typename T::v8*>(sh + (wm * 64) * 128 + lds_off(i * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int u = KT1 + v, nj = v == 2 ? 1 : 2;
        if (v > 0) issue_slot(jc, u + 3);
        const unsigned char* sw = smem + OFF_RING + (u & (NRING - 1)) * XIMG + (wn * 16 * nj) * 128;
        typename T::v8 fw[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int j = 0; j < nj; ++j) fw[ks][j] = *reinterpret_cast<const typename T::v8*>(sw + lds_off(j * 16 + fr, ks * 4 + fq));
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < nj; ++j) acc[i][2 * v + j] = T::mfma16(fw[ks][j], fa[ks][i], acc[i][2 * v + j]);
        __builtin_amdgcn_s_setprio(0);
        SDN_FTS_MARK(6)                                                      // contraction: request + fragment reads + MFMAs issued
        // the next entry has landed; the two after it stay in flight (slot 5: entries 7 (1 piece), 8; slots 6, 7: 2 + 2 pieces).
        // The last chunk has no entries 8..10: it drains what is left
        if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (v == 0) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                        // the stage (after slot 5: H too) is free again
        SDN_FTS_MARK(5)
      }
    }
  }

  // ---- trailing k-tiles [h3 | Wpo]: A = X, weights double-buffered between the two 40 KB buffers.  The residual tile (80 KB of
  //      HBM reads the shared epilogue would only start after the last MFMA) is DMA'd into the staging slab piecewise: the slab
  //      is the X region, and X image kt is dead as soon as trailing k-tile kt has been consumed by every wave.
  const __amdgpu_buffer_rsrc_t rs_res = make_rsrc(a.residual, (unsigned)((long)a.M * C * 2));
  auto issue_residual = [&](int img) {                      // pieces 16 img .. 16 img + 15 of the linear [128][640 B] slab, 2 per wave
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int piece = img * 16 + wid * 2 + q;
      const int e = piece * 64 + lane;
      const int r = e / (BN / 8), c = e - r * (BN / 8);
      const int m = m0 + r;
      const unsigned off = m < a.M ? (unsigned)(((long)m * C + c * 8) * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_res, (lds_ptr_t)(smem + piece * 1024), 16, off, 0, 0, 0);
    }
  };
#pragma unroll
  for (int q = 0; q < 5; ++q) issue_w2_slice(NCH, q, OFF_TA);
#pragma unroll
  for (int q = 0; q < 5; ++q) issue_w2_slice(NCH + 1, q, OFF_TB);
#pragma unroll
  for (int kt = 0; kt < KT1; ++kt) {
    const int boff = (kt & 1) ? OFF_TB : OFF_TA;
    // this k-tile's weights have landed; what was issued after them may stay in flight (in issue order: kt = 0: W2[1] |
    // 1: W2[2], res0 | 2: res0?, W2[3], res1 | 3: res1, W2[4], res2 | 4: res2, res3)
    if (kt == 0) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (kt == 1) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if (kt == 2 || kt == 3) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                            // (raw: __syncthreads would drain what is in flight)
    {
      const unsigned char* sa = sa_x + kt * XIMG;
      const unsigned char* sw = smem + boff + (wn * 16 * NREP) * 128;
      SDN_FFN_CONTRACT(sa, sw)
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                            // every wave done with this weight buffer and with X image kt
    if (kt + 2 < KT1) {
#pragma unroll
      for (int q = 0; q < 5; ++q) issue_w2_slice(NCH + kt + 2, q, boff);
    }
    issue_residual(kt);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                                           // residual slab complete; weight buffers dead

  // ---- epilogue: + residual -> 16 bit, whole-row stores, GroupNorm column sums (the shared GEMM epilogue) ----
  GemmArgs g{};
  g.M = a.M; g.N = C; g.K = HID + C; g.ldc = C; g.n_valid = C; g.act = 0; g.out_kind = 0;
  g.residual = (const __bf16*)a.residual; g.out = a.out; g.col_stats = a.col_stats; g.res_lds = 1;
  g.res_bytes = (unsigned)((long)a.M * C * 2); g.rows_per_batch = 0; g.residual_bcast = 0;
  constexpr int LNF = 0, WGM = 2, NSTAGE = 2, STAGE = LDS_BYTES / 2;
  constexpr int CW_PAD = (BN + 8) * 2;
  const bool staged = true;
  const int out_cols = BN;
  const bool res_lds = true;
  const int CW = BN * 2;
  const bool lean = true, lean_gelu = false, lean_gate = false, lean_erf = false;
  constexpr int PASSES = 1, WM_PER_PASS = WGM / PASSES, ROWS_PER_PASS = 64 * WM_PER_PASS;
  static_assert(BM * CW_PAD <= NSTAGE * STAGE - 8 * BN * 8, "staged tile and the column-sum scratch must fit the LDS");
#define SDN_EPI_RES_PRELOADED
#define SDN_PASS 0
#include "sdn_gemm_epilogue.inc"
#undef SDN_PASS
#undef SDN_EPI_RES_PRELOADED
  SDN_FTS_MARK(7)                                                           // trailing k-tiles + epilogue
  SDN_FTS_FLUSH
  (void)NWAVES; (void)WGM; (void)lean_gelu; (void)lean_gate; (void)lean_erf; (void)staged; (void)CW_PAD; (void)KT2;
#endif  // __HIP_DEVICE_COMPILE__
}

}  // namespace sdn_gemm_detail
using namespace sdn_gemm_detail;

// C must be 320 (the instantiated width: SD-v1.4's 64 x 64 level); other widths keep the two-launch path.
#ifdef SDN_FFN_STAMPS
extern "C" int sdn_debug_set_ffn_stamps(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(sdn_gemm_detail::g_ffn_stamps), &p, sizeof(p)); }
#endif
extern "C" int sdn_ffn_geglu_fused(int32_t dtype, int64_t M, int32_t C, const void* x, const float* row_stats, const void* w1_folded, const float* c1,
                        const float* d1, const void* w_cat, const float* b_cat, const void* residual, void* out, float* col_stats,
                        void* stream) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (dtype < 0 || dtype > 1 || C != 320 || M < 0 || !x || !w1_folded || !c1 || !d1 || !w_cat || !b_cat || !residual || !out)
    return SDN_E_INVALID;
  if (!al16(x) || !al16(w1_folded) || !al16(c1) || !al16(d1) || !al16(w_cat) || !al16(b_cat) || !al16(residual) || !al16(out) ||
      (reinterpret_cast<uintptr_t>(row_stats) & 7) || (reinterpret_cast<uintptr_t>(col_stats) & 7))
    return SDN_E_INVALID;
  if (M * C * 2 >= (1L << 31)) return SDN_E_INVALID;          // LDS-DMA offsets are 31 bit
  if (M == 0) return SDN_OK;
  FfnArgs a{x, row_stats, w1_folded, c1, d1, w_cat, b_cat, residual, out, col_stats, (int)M};
  const unsigned grid = (unsigned)((M + 127) / 128);
  record_gemm_launch(4, dtype, 10, 2, 2, row_stats ? 2 : 1, (int)grid, 1, 1, 0);
  if (dtype == 1) hipLaunchKernelGGL((k_ffn320<SdnF16>), dim3(grid), dim3(512), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_ffn320<SdnBF16>), dim3(grid), dim3(512), 0, (hipStream_t)stream, a);
  return sdn_launch_status();
}
