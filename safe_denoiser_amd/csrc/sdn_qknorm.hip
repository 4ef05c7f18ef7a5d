// q/k RMS norm of the SD-3.5 attentions (diffusers Attention with qk_norm = "rms_norm": norm_q / norm_k = RMSNorm(head_dim) applied
// per head after the projections): in place on the q and k thirds of the rows the stacked QKV GEMM writes.  Pure streaming: no LDS,
// no barrier; one 16-byte load and store per lane, the squares summed in f32 in the lane and across the lanes of a head by shuffles.
#include "sdn_common.h"

namespace {

constexpr int THREADS = 256, HD = 64;

// Sum across the LPH (8 or 16) adjacent lanes that own one head: every lane of the head ends with the total.
template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int off = LPH / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SDN_WAVE);
  return v;
}

// One wave per item = GPW consecutive heads (groups of 64 columns) of one row; EPL elements per lane, LPH = 64 / EPL lanes per head.
// T = SdnBF16 / SdnF16 (EPL 8) or float (EPL 4).  Groups g < heads take wq, the others wk; groups from 2 * heads on (v and whatever
// lies behind it) are never touched.  Items are walked grid-stride as (row, chunk) pairs, advanced without a division; offsets are
// 64-bit (rows * ld 16-bit elements pass 2^31 bytes at the plan's largest batch).
template <typename T, int EPL>
__global__ void __launch_bounds__(THREADS)
k_qk_rmsnorm(void* qkv, long rows, int wpr, int heads, long ld, const float* __restrict__ wq, const float* __restrict__ wk, float eps) {
  constexpr int LPH = HD / EPL, GPW = SDN_WAVE / LPH, ES = 16 / EPL;
  const int lane = threadIdx.x & 63, sub = lane % LPH, gl = lane / LPH;
  float gq[EPL], gk[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) { gq[j] = wq[sub * EPL + j]; gk[j] = wk[sub * EPL + j]; }
  const int nwaves = gridDim.x * (THREADS / 64), wave0 = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  const int dr = nwaves / wpr, dc = nwaves % wpr;
  long row = wave0 / wpr;
  int chunk = wave0 % wpr;
  for (; row < rows; row += dr, chunk += dc) {
    if (chunk >= wpr) { chunk -= wpr; ++row; if (row >= rows) break; }       // (wave-uniform)
    const int g = chunk * GPW + gl;
    const bool on = g < 2 * heads;
    char* p = (char*)qkv + (row * ld + (long)g * HD + sub * EPL) * ES;
    float x[EPL];
    if (on) {
      if constexpr (EPL == 4) {
        const sdn_f32x4 t = *reinterpret_cast<const sdn_f32x4*>(p);
        x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
      } else {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        x[0] = T::to_f(t.x & 0xffff); x[1] = T::to_f(t.x >> 16); x[2] = T::to_f(t.y & 0xffff); x[3] = T::to_f(t.y >> 16);
        x[4] = T::to_f(t.z & 0xffff); x[5] = T::to_f(t.z >> 16); x[6] = T::to_f(t.w & 0xffff); x[7] = T::to_f(t.w >> 16);
      }
    } else {
#pragma unroll
      for (int j = 0; j < EPL; ++j) x[j] = 0.f;
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < EPL; ++j) ss = fmaf(x[j], x[j], ss);
    ss = head_sum<LPH>(ss);
    const float r = rsqrtf(ss * (1.0f / HD) + eps);
    const bool isq = g < heads;
    float y[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) y[j] = x[j] * r * (isq ? gq[j] : gk[j]);
    if (on) {
      if constexpr (EPL == 4) {
        const sdn_f32x4 t = {y[0], y[1], y[2], y[3]};
        *reinterpret_cast<sdn_f32x4*>(p) = t;
      } else {
        uint4 t;
        t.x = T::pack2(y[0], y[1]); t.y = T::pack2(y[2], y[3]); t.z = T::pack2(y[4], y[5]); t.w = T::pack2(y[6], y[7]);
        *reinterpret_cast<uint4*>(p) = t;
      }
    }
  }
}

template <typename T, int EPL>
int launch(void* qkv, int64_t rows, int heads, int ld, const float* wq, const float* wk, float eps, hipStream_t st) {
  constexpr int GPW = SDN_WAVE / (HD / EPL);
  const int wpr = (2 * heads + GPW - 1) / GPW;                               // wave items per row
  const int64_t items = rows * wpr, blocks = (items + THREADS / 64 - 1) / (THREADS / 64);
  hipLaunchKernelGGL((k_qk_rmsnorm<T, EPL>), dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(THREADS), 0, st, qkv, (long)rows, wpr,
                     heads, (long)ld, wq, wk, eps);
  return sdn_launch_status();
}

}  // namespace

extern "C" int sdn_qk_rmsnorm(int32_t dtype, void* qkv, int64_t rows, int32_t heads, int32_t ld, const float* wq, const float* wk,
                              float eps, void* stream) {
  if (!qkv || !wq || !wk || rows < 0 || rows > (1LL << 40) || heads <= 0 || heads > (1 << 20) || dtype < 0 || dtype > 2 || !(eps > 0.f))
    return SDN_E_INVALID;
  if ((int64_t)ld < 3LL * heads * HD || (ld % (dtype == 2 ? 4 : 8)) != 0) return SDN_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(wq) & 3) || (reinterpret_cast<uintptr_t>(wk) & 3))
    return SDN_E_INVALID;
  if (rows == 0) return SDN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) return launch<SdnBF16, 8>(qkv, rows, heads, ld, wq, wk, eps, st);
  if (dtype == 1) return launch<SdnF16, 8>(qkv, rows, heads, ld, wq, wk, eps, st);
  return launch<float, 4>(qkv, rows, heads, ld, wq, wk, eps, st);
}
