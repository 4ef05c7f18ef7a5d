// K = 320 linears (the projections of the C = 320 transformer blocks): weights resident in registers, activations streamed
// through LDS as row panels by persistent workgroups.  DESIGN 10.20.
//
//   out[M, N] = A[M, 320] . W[N, 320]^T (+ bias[n]) (+ residual[m, n])          N % 320 == 0, 16-bit operands and output
//   LNF:  out = rstd[m] * (A . W'^T - mean[m] * c[n]) + d[n]                    (LayerNorm folded in, as k_gemm_dma's LNF = 1)
//
// k_gemm_dma runs these shapes as 256 x 320 tiles whose k loop (5 k-tiles) is half of the tile's life: one 147-KB workgroup per
// CU leaves nothing to cover a tile's prologue DMA round trip or its epilogue, and HBM idles between a tile's load burst and its
// store burst.  This kernel has no tile boundary:
//   * one persistent workgroup per CU, 8 waves as 2 (M) x 4 (N); wave (wm, wn) owns columns [80 wn, 80 wn + 80) of one 320-column
//     group and keeps their 5 x 10 weight fragments (16 x 16 x 32 MFMA, swapped orientation: weights = A operand) in 200 VGPRs for
//     the whole launch;
//   * the activation rows stream through a 3-slot LDS ring of 40-KB panels (64 rows x 320 K as five swizzled k-tile images, the
//     lds_off layout of k_gemm_dma), filled by LDS-DMA with two panels in flight while one is consumed.  A workgroup takes panels
//     s, s + S, s + 2S, ... of its row stream s (S = streams of the launch): the stream never drains;
//   * N = 960: three sibling workgroups (one per column group) read the same panels; sdn_k320_map puts them on one XCD.
// RES (16-bit residual pre-added into the accumulators) streams the residual rows the same way: a panel is then 32 rows of A
// (20 KB) + the same 32 rows of the residual (20 KB), the packed output is written in place over the residual image and
// leaves from there.  Register loads of the residual were not an option: with LDS-DMA in flight the compiler drains vmcnt to 0 for
// any VGPR-destination load, which would empty the ring once per panel.
//
// vmcnt discipline: LDS-DMA loads and global stores share vmcnt, and nothing on record says the two kinds retire in issue order.
// So waves 0-3 issue EVERY DMA piece (10 per wave and panel, every panel -- past the last panel the pieces are all out of range and
// move no bytes -- so one counted wait, vmcnt(10), holds for the whole stream) and waves 4-7 issue EVERY global store; a wave
// counts one kind only.  bias / c / d live in LDS: no VGPR-destination global load is issued after the first DMA piece.
//
// Arithmetic: per output element the chain of k_gemm_dma -- acc = bias, += residual (sdn_gemm.hip, res_pre), k-steps 0..9 in
// order through the same mfma16, the LNF = 1 statistics from the same lanes in the same order, the same pack -- so the result is
// bit-identical to sdn_gemm_* / sdn_gemm_ln_* on the same operands (tests/test_gpu_gemm_k320.py).
#include "sdn_common.h"
#include "sdn_ops.h"
#include "sdn_gemm_common.h"
#include "sdn_gemm_k320.h"

static int g_k320_max_wgs = 0;               // debug: cap on the grid (0 = one workgroup per CU), see sdn_debug_set_k320_max_wgs
static int g_k320_last[8] = {0};             // launch record: family (6), dtype, LNF, RES, grid, column groups, row streams, panels

namespace sdn_gemm_detail {

struct K320Args {
  const unsigned short* a; const unsigned short* w; const float* bias; const float* ln_c; const float* ln_d;
  const unsigned short* res; unsigned short* out;
  int M, ldc, ncg;
  float ln_eps;
};

template <typename T, int LNF, bool RES>
__global__ void __launch_bounds__(512)
k_gemm_k320(const K320Args g) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int ROWS = RES ? 32 : 64;                        // rows of a panel
  constexpr int G = ROWS / 32;                               // 16-row groups a wave runs per panel
  constexpr int RB = ROWS / 8;                               // 1-KiB pieces per k-tile image
  constexpr int IMG = ROWS * 128;                            // bytes of a k-tile image
  constexpr int A_PIECES = 5 * RB / 4;                       // A pieces per DMA wave and panel: 10 (5 with RES, + 5 residual pieces)
  constexpr int SLOT = 40960, RING = 3 * SLOT;
  constexpr int STG = RING;                                  // staging slab: 32 packed output rows, 20 KB (unused with RES)
  constexpr int PRM = STG + 32 * 640;                        // bias | c | d of this column group, 320 floats each
  constexpr int SMEM = PRM + 3 * 1280;
  static_assert(5 * IMG * (RES ? 2 : 1) == SLOT, "a panel fills its slot");
  static_assert(A_PIECES + (RES ? 5 : 0) == 10, "vmcnt(10) below counts ten pieces per DMA wave and panel");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;
  const int fr = lane & 15, fq = lane >> 4;
  int stream, cg;
  const int S = sdn_k320_map((int)gridDim.x, g.ncg, (int)blockIdx.x, &stream, &cg);
  if (stream < 0) return;                                    // (the whole workgroup: grid % column groups spare ones)
  const int n0 = cg * 320;

  // ---- prologue: resident weight fragments, bias / c / d to LDS.  Ordinary loads: all of them retire before the first DMA piece ----
  typename T::v8 wf[5][10];
  {
    const unsigned short* wrow = g.w + (long)(n0 + wn * 80 + fr) * 320 + fq * 8;
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int s = 0; s < 10; ++s) wf[t][s] = *reinterpret_cast<const typename T::v8*>(wrow + t * 16 * 320 + s * 32);
  }
  if (tid < 320) {
    float* prm = reinterpret_cast<float*>(smem + PRM);
    prm[tid] = g.bias ? g.bias[n0 + tid] : 0.f;
    if constexpr (LNF) { prm[320 + tid] = g.ln_c[n0 + tid]; prm[640 + tid] = g.ln_d[n0 + tid]; }
  }
  // (opaque to the compiler from here on: a fragment is neither re-fetched from memory inside the stream nor waited for there)
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int s = 0; s < 10; ++s) asm volatile("" : "+v"(wf[t][s]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // Buffer sizes are the tensors' own: a row past M lies past num_records, so the range check zero-fills it (and every piece of a
  // panel past the last one) without a compare here.  The whole offset rides in voffset: the range check does not see soffset.
  const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(g.a, (unsigned)((long)g.M * 640));
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rs_r = make_rsrc(RES ? g.res : g.a, RES ? (unsigned)((long)g.M * g.ldc * 2) : 0u);
  // one panel -> one slot.  Called by waves 0-3 only, ten pieces each.  (ln = the lane number: the stream loop hands in an opaque
  // copy, so that nothing derived from it is kept in a register across the loop -- the weights leave no room for that)
  auto issue = [&](int p, int slot, int ln) {
    const int lrow = (ln >> 3) & 7;
    const unsigned a_lane = (unsigned)(lrow * 640 + (((ln & 7) ^ lrow) << 4));     // (row, logical chunk) this lane fetches of a piece
    [[maybe_unused]] const unsigned r_lane = (unsigned)(lrow * g.ldc * 2 + (((ln & 7) ^ lrow) << 4));
    const unsigned m0 = (unsigned)p * ROWS;
    unsigned char* dst = smem + slot * SLOT;
#pragma unroll
    for (int q = 0; q < A_PIECES; ++q) {
      const int piece = wid * A_PIECES + q;
      const int kt = piece / RB, rb = piece - kt * RB;
      const unsigned off = (m0 + rb * 8) * 640u + kt * 128 + a_lane;           // (wave-uniform part + lane part)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_ptr_t)(dst + piece * 1024), 16, off, 0, 0, 0);
    }
    if constexpr (RES) {
      // the residual rows of the panel as 4 x 5 pieces: piece (rb, seg) = rows rb 8 .. + 8, bytes seg 128 .. + 128 of the 640-byte
      // row, [8][8 x 16 B] with the chunk ^ (row & 7) swizzle (out_off below)
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const unsigned off = (m0 + wid * 8) * (unsigned)(g.ldc * 2) + (unsigned)(n0 * 2 + q * 128) + r_lane;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_r, (lds_ptr_t)(dst + 5 * IMG + (wid * 5 + q) * 1024), 16, off, 0, 0, 0);
      }
    }
  };

  const int NP = (g.M + ROWS - 1) / ROWS;
  const int n_my = stream < NP ? (NP - stream + S - 1) / S : 0;
  if (wid < 4) { issue(stream, 0, tid); issue(stream + S, 1, tid); }

  const float* prm = reinterpret_cast<const float*>(smem + PRM);
  int slot = 0;
  for (int i = 0; i < n_my; ++i) {
    int tl = tid;
    asm volatile("" : "+v"(tl));                             // (see issue(): lane-derived values are recomputed per panel, not kept)
    const int fr = tl & 15, fq = (tl >> 4) & 3;
    // The 32-row output image (the staging slab; RES: the residual image, rewritten in place): 4 x 5 pieces, piece (rb, seg) = rows
    // rb 8 .. + 8, bytes seg 128 .. + 128 of the 640-byte row as [8][8 x 16 B] with the chunk ^ (row & 7) swizzle -- the image one DMA
    // piece writes, and one the row-wise readers below take 1 KiB at a time without a bank conflict.
    const int orow = wm * 16 + fr;                           // this lane's fragment row inside the image
    const int o_rowpart = (orow >> 3) * 5120 + (orow & 7) * 128;
    auto out_off = [&](int t) {                              // byte offset of this lane's 8 bytes of column tile t
      const int cb = wn * 160 + t * 32 + fq * 8;
      return o_rowpart + (cb >> 7) * 1024 + ((((cb >> 4) & 7) ^ (orow & 7)) << 4) + (cb & 8);
    };
    const int st_r = (tl >> 3) & 31;                         // store waves: image row and 16-byte chunk of this lane
    const int st_lds = (st_r >> 3) * 5120 + (st_r & 7) * 128 + (((tl & 7) ^ (st_r & 7)) << 4);
    const int p = stream + i * S;
    const int m0 = p * ROWS;
    // panel i has landed once at most panel i + 1's ten pieces are outstanding
    if (wid < 4) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (store waves: their reads of the previous panel's output are done)
    __builtin_amdgcn_s_barrier();                            // panel i visible; slot of panel i - 1 and the staging slab are free
    asm volatile("" ::: "memory");
    if (wid < 4) issue(p + 2 * S, slot == 0 ? 2 : slot - 1, tl);
    const unsigned char* sa = smem + slot * SLOT;
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      const int row_l = wm * (ROWS / 2) + gi * 16 + fr;      // this lane's row inside the panel
      f32x4 acc[5];
#pragma unroll
      for (int t = 0; t < 5; ++t) acc[t] = *reinterpret_cast<const f32x4*>(prm + wn * 80 + t * 16 + fq * 4);
      if constexpr (RES) {
        // read from asm statements: a ds_read of the compiler's own from the image the DMA fills waits for vmcnt(0) first
        const unsigned r_addr = (unsigned)(unsigned long)(lds_ptr_t)const_cast<unsigned char*>(sa + 5 * IMG);
        unsigned long long rr[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) asm volatile("ds_read_b64 %0, %1" : "=v"(rr[t]) : "v"(r_addr + (unsigned)out_off(t)) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rr[0]), "+v"(rr[1]), "+v"(rr[2]), "+v"(rr[3]), "+v"(rr[4])::"memory");
#pragma unroll
        for (int t = 0; t < 5; ++t) {
          const unsigned lo = (unsigned)rr[t], hi = (unsigned)(rr[t] >> 32);
          acc[t][0] += T::to_f(lo & 0xffff); acc[t][1] += T::to_f(lo >> 16);
          acc[t][2] += T::to_f(hi & 0xffff); acc[t][3] += T::to_f(hi >> 16);
        }
      }
      [[maybe_unused]] float s1 = 0.f, s2 = 0.f;
      // k-step s + 1's fragment is requested before k-step s's five MFMAs and nothing else moves across the fences: two fragments
      // live, not the six the scheduler would fetch ahead (the weights leave no room for them)
      typename T::v8 fa[2];
      fa[0] = *reinterpret_cast<const typename T::v8*>(sa + lds_off(row_l, fq));
#pragma unroll
      for (int s = 0; s < 10; ++s) {
        if (s + 1 < 10)
          fa[(s + 1) & 1] = *reinterpret_cast<const typename T::v8*>(sa + ((s + 1) >> 1) * IMG + lds_off(row_l, ((s + 1) & 1) * 4 + fq));
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (LNF) { s1 = T::dot_ones(fa[s & 1], s1); s2 = T::dot_self(fa[s & 1], s2); }
#pragma unroll
        for (int t = 0; t < 5; ++t) acc[t] = T::mfma16(wf[t][s], fa[s & 1], acc[t]);
        __builtin_amdgcn_sched_barrier(0);
      }
      [[maybe_unused]] float mu = 0.f, rs = 0.f;
      if constexpr (LNF) {
        // a lane holds the k-chunks fq, fq + 4 of every k-tile of row fr: the other three lane groups hold the rest
        const float invk = 1.0f / 320.0f;
        float a1 = s1, a2 = s2;
        a1 += __shfl_xor(a1, 16, 64); a2 += __shfl_xor(a2, 16, 64);
        a1 += __shfl_xor(a1, 32, 64); a2 += __shfl_xor(a2, 32, 64);
        mu = a1 * invk;
        const float var = fmaxf(a2 * invk - mu * mu, 0.f);
        rs = __builtin_amdgcn_rsqf(var + g.ln_eps);
      }
      if (!RES && gi > 0) {                                  // the first pass's rows have left the staging slab
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      // packed rows: staging slab, or (RES) in place over the residual image.  Written from an asm statement: before a ds_write of
      // its own the compiler waits for vmcnt(0) while LDS-DMA is in flight
      const unsigned char* oimg = RES ? sa + 5 * IMG : smem + STG;
      const unsigned o_addr = (unsigned)(unsigned long)(lds_ptr_t)const_cast<unsigned char*>(oimg);
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        f32x4 v = acc[t];
        if constexpr (LNF) {
          const f32x4 cv = *reinterpret_cast<const f32x4*>(prm + 320 + wn * 80 + t * 16 + fq * 4);
          const f32x4 dv = *reinterpret_cast<const f32x4*>(prm + 640 + wn * 80 + t * 16 + fq * 4);
          v = (acc[t] - mu * cv) * rs + dv;
        }
        uint2 pk; pk.x = T::pack2(v[0], v[1]); pk.y = T::pack2(v[2], v[3]);
        asm volatile("ds_write_b64 %0, %1" ::"v"(o_addr + (unsigned)out_off(t)), "v"((unsigned long long)pk.y << 32 | pk.x) : "memory");
        if constexpr (LNF) __builtin_amdgcn_sched_barrier(0);  // (one tile's c / d vectors live at a time)
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (the stores above are not counted by the compiler)
      __builtin_amdgcn_s_barrier();                          // 32 packed rows complete
      asm volatile("" ::: "memory");
      if (wid >= 4) {                                        // 16 bytes per lane, 128-byte lines: a lane stores the five segments of its row
        const int m = m0 + (RES ? st_r : (st_r >> 4) * 32 + gi * 16 + (st_r & 15));
        if (m < g.M) {
          unsigned short* op = g.out + (long)m * g.ldc + n0 + (tl & 7) * 8;
#pragma unroll
          for (int k = 0; k < 5; ++k) *reinterpret_cast<u32x4*>(op + k * 64) = *reinterpret_cast<const u32x4*>(oimg + st_lds + k * 1024);
        }
      }
    }
    slot = slot == 2 ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the trailing (out-of-range) pieces still target this workgroup's LDS
#endif
}

template <typename T>
int launch_k320(const K320Args& g, int grid, bool ln, bool res, hipStream_t st) {
  if (ln) hipLaunchKernelGGL((k_gemm_k320<T, 1, false>), dim3(grid), dim3(512), 0, st, g);
  else if (res) hipLaunchKernelGGL((k_gemm_k320<T, 0, true>), dim3(grid), dim3(512), 0, st, g);
  else hipLaunchKernelGGL((k_gemm_k320<T, 0, false>), dim3(grid), dim3(512), 0, st, g);
  return sdn_launch_status();
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace sdn_gemm_detail
using namespace sdn_gemm_detail;

extern "C" int32_t sdn_gemm_k320_map(int32_t grid, int32_t col_groups, int32_t wg, int32_t* stream_out, int32_t* group_out) {
  if (grid <= 0 || col_groups <= 0 || wg < 0 || wg >= grid) return SDN_E_INVALID;
  int s = -1, c = 0;
  const int S = sdn_k320_map(grid, col_groups, wg, &s, &c);
  if (stream_out) *stream_out = s;
  if (group_out) *group_out = c;
  return S;
}

// debug (tests): cap on the grid, 0 = one workgroup per CU -- a small grid pushes many panels through one workgroup's ring
extern "C" void sdn_debug_set_k320_max_wgs(int n) { g_k320_max_wgs = n > 0 ? n : 0; }
// diagnostics (tests): what the last sdn_gemm_k320 launch ran -- family (6), dtype, LNF, RES, grid, column groups, row streams, panels
extern "C" void sdn_debug_k320_last_launch(int* out, int n) {
  for (int i = 0; out && i < n; ++i) out[i] = i < 8 ? g_k320_last[i] : 0;
}
extern "C" void sdn_debug_k320_reset_launch(void) { for (int& v : g_k320_last) v = 0; }

extern "C" int sdn_gemm_k320(int32_t dtype, const sdn_gemm_desc* d, const void* a, const void* w, const float* bias, const float* ln_c,
                             const float* ln_d, float ln_eps, const void* residual, void* out, void* stream) {
  if (!d || !a || !w || !out || dtype < 0 || dtype > 1) return SDN_E_INVALID;
  if (d->K != 320 || d->N <= 0 || d->N % 320 != 0 || d->M < 0) return SDN_E_INVALID;
  if (d->a_mode != SDN_A_PLAIN || (d->K1 != 0 && d->K1 != d->K) || d->act != SDN_ACT_NONE || d->out_kind != SDN_OUT_BF16 ||
      (d->n_valid != 0 && d->n_valid != d->N) || d->residual_bcast || d->split_k > 1 || d->x3_out || d->f32_stream || d->upsample)
    return SDN_E_INVALID;
  const bool ln = ln_c || ln_d;
  if (ln && (!ln_c || !ln_d || bias || residual)) return SDN_E_INVALID;
  const int ldc = d->ldc > 0 ? d->ldc : d->N;
  if (ldc < d->N || (ldc & 7)) return SDN_E_INVALID;
  if (!al16(a) || !al16(w) || !al16(out) || (residual && !al16(residual)) || (bias && !al16(bias)) || (ln && (!al16(ln_c) || !al16(ln_d))))
    return SDN_E_INVALID;
  // operands stay below the LDS-DMA out-of-range sentinel
  // (and the offsets of the out-of-range pieces past the last panel -- up to 2 panels x 256 streams -- must not wrap 32 bits)
  if ((long)d->M * 640 >= (1L << 31) || (long)d->M * ldc * 2 >= (1L << 31) || ((long)d->M + 40000) * ldc * 2 >= (1L << 32)) return SDN_E_INVALID;
  if (d->M == 0) return SDN_OK;
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return SDN_E_LAUNCH;
    cus = prop.multiProcessorCount;
  }
  const int ncg = d->N / 320;
  int grid = cus > ncg ? cus : ncg;
  if (g_k320_max_wgs > 0 && g_k320_max_wgs < cus) {
    // capped: the smallest grid that runs max(1, cap / ncg) streams (siblings share an XCD, so N = 960 needs 17 workgroups for one)
    const int want = g_k320_max_wgs / ncg > 0 ? g_k320_max_wgs / ncg : 1;
    int s0, c0;
    for (grid = ncg; grid < cus && sdn_k320_map(grid, ncg, 0, &s0, &c0) < want; ++grid) {}
  }
  {
    int s0, c0;
    if (sdn_k320_map(grid, ncg, 0, &s0, &c0) < 1) return SDN_E_INVALID;   // (a device too small to seat one stream's siblings on an XCD)
  }
  K320Args g{};
  g.a = (const unsigned short*)a; g.w = (const unsigned short*)w; g.bias = bias; g.ln_c = ln_c; g.ln_d = ln_d;
  g.res = (const unsigned short*)residual; g.out = (unsigned short*)out;
  g.M = d->M; g.ldc = ldc; g.ncg = ncg; g.ln_eps = ln_eps;
  {
    int s0, c0;
    const int S = sdn_k320_map(grid, ncg, 0, &s0, &c0);
    const int rows = residual ? 32 : 64;
    const int v[8] = {6, dtype, ln ? 1 : 0, residual ? 1 : 0, grid, ncg, S, (d->M + rows - 1) / rows};
    for (int i = 0; i < 8; ++i) g_k320_last[i] = v[i];
  }
  hipStream_t st = (hipStream_t)stream;
  return dtype == 0 ? launch_k320<SdnBF16>(g, grid, ln, residual != nullptr, st) : launch_k320<SdnF16>(g, grid, ln, residual != nullptr, st);
}
