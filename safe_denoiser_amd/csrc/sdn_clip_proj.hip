// Building blocks of the projected CLIP text encoders (transformers CLIPTextModelWithProjection, third party; SD-v3's
// text_encoder and text_encoder_2): the pooled row of each sequence -- gathered at the end-token position and passed through
// final_layer_norm, the only rows of the last layer that norm is ever applied to -- and the strided copy that places the tapped
// hidden state into a column slice of the caller's joint buffer.  The encoder layers are the CLIP plan's (sdn_plan_text.hip), the
// exact-erf GELU an epilogue of k_gemm_dma, text_projection an ordinary plan GEMM over the rows written here.
#include <math.h>
#include <type_traits>

#include "sdn_common.h"

namespace {

constexpr int THREADS = 256;

struct StoreF32 {};      // tag: f32 storage (SdnBF16 / SdnF16 are the 16-bit ones)

template <typename T>
__device__ __forceinline__ void load4(const void* row, int c, float (&v)[4]) {
  if constexpr (std::is_same<T, StoreF32>::value) {
    const sdn_f32x4 t = *reinterpret_cast<const sdn_f32x4*>(reinterpret_cast<const float*>(row) + c);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    const uint2 t = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(row) + c);
    v[0] = T::to_f(t.x & 0xffff); v[1] = T::to_f(t.x >> 16); v[2] = T::to_f(t.y & 0xffff); v[3] = T::to_f(t.y >> 16);
  }
}

// One workgroup per sequence.  Pooling position: wave 0 scans the ids (clamped like k_clip_embed's) for the first position of
// the highest id (eos_token_id == 2, transformers' legacy rule) or the first position equal to eos_token_id (0 when absent);
// both are "smallest position among the candidates", i.e. one min-reduction over a (key, position) pair.  Then LayerNorm of
// that row: mean first, variance around the mean second (two passes over a row that sits in L2), all in f32.
template <typename T>
__global__ void __launch_bounds__(THREADS)
k_clip_eos_rows(const int* __restrict__ ids, const void* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                int n, int C, int vocab, int eos, float eps, void* __restrict__ out, int* __restrict__ positions) {
  __shared__ float red[8];
  __shared__ int s_pos;
  const int b = blockIdx.x;
  if (threadIdx.x < 64) {
    // key = -id (legacy) or (id == eos ? 0 : 1); the smallest (key, position) wins, position 0 when no id equals eos
    long long best = 0x7fffffffffffffffLL;
    for (int t = threadIdx.x; t < n; t += 64) {
      int id = ids[(long)b * n + t];
      id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
      const long long key = eos == 2 ? (long long)(vocab - id) : (id == eos ? 0LL : 1LL);
      const long long cand = key * 0x100000000LL + t;
      best = cand < best ? cand : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long long o = __shfl_xor(best, off, SDN_WAVE);
      best = o < best ? o : best;
    }
    if (threadIdx.x == 0) {
      int p = (int)(best & 0xffffffffLL);
      if (eos != 2 && (best >> 32) != 0) p = 0;                  // no end token in the sequence: argmax of an all-zero vector
      s_pos = p;
      if (positions) positions[b] = p;
    }
  }
  __syncthreads();
  const int p = s_pos;                                           // in [0, n) by construction
  const size_t esz = std::is_same<T, StoreF32>::value ? 4 : 2;
  const char* row = reinterpret_cast<const char*>(x) + ((size_t)b * n + p) * C * esz;
  float s = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    load4<T>(row, c, v);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = block_sum<4>(s, red) / (float)C;
  float q = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    load4<T>(row, c, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = v[e] - mean; q = fmaf(d, d, q); }
  }
  const float rstd = 1.0f / sqrtf(block_sum<4>(q, red + 4) / (float)C + eps);
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    load4<T>(row, c, v);
    const sdn_f32x4 g = *reinterpret_cast<const sdn_f32x4*>(gamma + c), bt = *reinterpret_cast<const sdn_f32x4*>(beta + c);
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (v[e] - mean) * rstd * g[e] + bt[e];
    if constexpr (std::is_same<T, StoreF32>::value) {
      const sdn_f32x4 o = {r[0], r[1], r[2], r[3]};
      *reinterpret_cast<sdn_f32x4*>(reinterpret_cast<float*>(out) + (size_t)b * C + c) = o;
    } else {
      uint2 pk; pk.x = T::pack2(r[0], r[1]); pk.y = T::pack2(r[2], r[3]);
      *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out) + (size_t)b * C + c) = pk;
    }
  }
}

// 16 bytes per thread; chunk e of the source's [rows][cpr] grid goes to the strided destination row of the same (b, t)
__global__ void __launch_bounds__(THREADS)
k_copy_rows_strided(const uint4* __restrict__ src, long rows, int rows_per_batch, int cpr, char* __restrict__ dst, long batch_bytes,
                    long row_bytes) {
  const long total = rows * cpr;
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < total; e += (long)gridDim.x * THREADS) {
    const long r = e / cpr; const int c = (int)(e - r * cpr);
    const long b = r / rows_per_batch; const int t = (int)(r - b * rows_per_batch);
    *reinterpret_cast<uint4*>(dst + b * batch_bytes + t * row_bytes + (long)c * 16) = src[e];
  }
}

}  // namespace

extern "C" int sdn_clip_eos_rows(int32_t dtype, const int32_t* input_ids, const void* x, const float* gamma, const float* beta,
                                 int32_t batch, int32_t seq_len, int32_t hidden, int32_t vocab, int32_t eos_token_id, float eps,
                                 void* out, int32_t* positions, void* stream) {
  if (!input_ids || !x || !gamma || !beta || !out || batch < 0 || seq_len <= 0 || seq_len > 4096 || hidden <= 0 || (hidden & 3) ||
      vocab <= 0 || dtype < 0 || dtype > 2 || !(eps >= 0.f))
    return SDN_E_INVALID;
  const uintptr_t am = dtype == 2 ? 15 : 7;
  if ((reinterpret_cast<uintptr_t>(x) & am) || (reinterpret_cast<uintptr_t>(out) & am) || (reinterpret_cast<uintptr_t>(gamma) & 15) ||
      (reinterpret_cast<uintptr_t>(beta) & 15) || (reinterpret_cast<uintptr_t>(input_ids) & 3) || (reinterpret_cast<uintptr_t>(positions) & 3))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const dim3 grid((unsigned)batch), blk(THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 2)
    hipLaunchKernelGGL((k_clip_eos_rows<StoreF32>), grid, blk, 0, st, input_ids, x, gamma, beta, seq_len, hidden, vocab, eos_token_id, eps, out, positions);
  else if (dtype == 1)
    hipLaunchKernelGGL((k_clip_eos_rows<SdnF16>), grid, blk, 0, st, input_ids, x, gamma, beta, seq_len, hidden, vocab, eos_token_id, eps, out, positions);
  else
    hipLaunchKernelGGL((k_clip_eos_rows<SdnBF16>), grid, blk, 0, st, input_ids, x, gamma, beta, seq_len, hidden, vocab, eos_token_id, eps, out, positions);
  return sdn_launch_status();
}

extern "C" int sdn_copy_rows_strided(const void* src, int32_t batch, int32_t rows_per_batch, int32_t cols, int32_t elem_bytes, void* dst,
                                     int64_t dst_batch_stride, int64_t dst_row_stride, void* stream) {
  if (!src || !dst || batch < 0 || rows_per_batch <= 0 || cols <= 0 || (elem_bytes != 2 && elem_bytes != 4)) return SDN_E_INVALID;
  const long row_bytes = (long)cols * elem_bytes;
  if ((row_bytes & 15) || dst_row_stride < cols || dst_batch_stride < (int64_t)rows_per_batch * dst_row_stride ||
      ((dst_row_stride * elem_bytes) & 15) || ((dst_batch_stride * elem_bytes) & 15) || (reinterpret_cast<uintptr_t>(src) & 15) ||
      (reinterpret_cast<uintptr_t>(dst) & 15))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const long rows = (long)batch * rows_per_batch;
  const int cpr = (int)(row_bytes / 16);
  long g = (rows * cpr + THREADS - 1) / THREADS;
  g = g > 8192 ? 8192 : g;
  hipLaunchKernelGGL(k_copy_rows_strided, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, (const uint4*)src, rows,
                     rows_per_batch, cpr, (char*)dst, (long)dst_batch_stride * elem_bytes, (long)dst_row_stride * elem_bytes);
  return sdn_launch_status();
}
