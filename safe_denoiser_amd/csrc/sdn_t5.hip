// T5 encoder building blocks (transformers T5EncoderModel, third party; SD-v3's text_encoder_3): RMS layer norm, token
// embedding into the f32 residual stream, and the relative-position bias vector of the self-attention.  The biased
// attention itself is an instantiation of k_attn (sdn_attn.hip), the gated tanh-GELU an epilogue of k_gemm_dma.
#include <math.h>

#include "sdn_common.h"

namespace {

constexpr int THREADS = 256;

// T5LayerNorm: out = x * rsqrt(mean(x^2) + eps) * w.  No mean subtraction, no bias; statistics in f32.  One workgroup per
// row; the row is read twice (the second read hits L2), so any width fits.
template <typename T, bool XF32>
__global__ void __launch_bounds__(THREADS)
k_rmsnorm(const void* __restrict__ xv, int C, float eps, const float* __restrict__ w, unsigned short* __restrict__ out) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const float* xf = reinterpret_cast<const float*>(xv) + row * C;
  const unsigned short* xh = reinterpret_cast<const unsigned short*>(xv) + row * C;
  float ss = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    if (XF32) {
      const sdn_f32x4 t = *reinterpret_cast<const sdn_f32x4*>(xf + c);
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
      const uint2 t = *reinterpret_cast<const uint2*>(xh + c);
      v[0] = T::to_f(t.x & 0xffff); v[1] = T::to_f(t.x >> 16); v[2] = T::to_f(t.y & 0xffff); v[3] = T::to_f(t.y >> 16);
    }
    ss = fmaf(v[0], v[0], ss); ss = fmaf(v[1], v[1], ss); ss = fmaf(v[2], v[2], ss); ss = fmaf(v[3], v[3], ss);
  }
  ss = block_sum<4>(ss, red);
  const float rs = 1.0f / sqrtf(ss / (float)C + eps);
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    if (XF32) {
      const sdn_f32x4 t = *reinterpret_cast<const sdn_f32x4*>(xf + c);
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
      const uint2 t = *reinterpret_cast<const uint2*>(xh + c);
      v[0] = T::to_f(t.x & 0xffff); v[1] = T::to_f(t.x >> 16); v[2] = T::to_f(t.y & 0xffff); v[3] = T::to_f(t.y >> 16);
    }
    const sdn_f32x4 g = *reinterpret_cast<const sdn_f32x4*>(w + c);
    uint2 pk;
    pk.x = T::pack2(v[0] * rs * g[0], v[1] * rs * g[1]);
    pk.y = T::pack2(v[2] * rs * g[2], v[3] * rs * g[3]);
    *reinterpret_cast<uint2*>(out + row * C + c) = pk;
  }
}

// out[r, :] = f32(table[ids[r], :]): the residual stream starts in f32 (no position table: T5's positions live in the attention bias)
template <typename T>
__global__ void __launch_bounds__(THREADS)
k_embed_tokens(const int* __restrict__ ids, const unsigned short* __restrict__ tok, long rows, int C, int vocab, float* __restrict__ out) {
  const int cch = C / 2;
  const long total = rows * cch;
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < total; e += (long)gridDim.x * THREADS) {
    const long r = e / cch; const int c = (int)(e - r * cch) * 2;
    int id = ids[r]; id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);       // out-of-range ids are clamped, not faulted on
    const unsigned a = *reinterpret_cast<const unsigned*>(tok + (long)id * C + c);
    *reinterpret_cast<float2*>(out + r * C + c) = make_float2(T::to_f(a & 0xffff), T::to_f(a >> 16));
  }
}

// Bucket of a relative position (memory - query) in T5's bidirectional scheme: half the buckets per sign, the first half of
// those exact, the rest logarithmic up to max_distance.  The logarithmic part is float arithmetic in transformers
// (T5Attention._relative_position_bucket: log(rel / max_exact) / log(max_distance / max_exact) * (half - max_exact), truncated);
// it is evaluated HERE, on the host, once per distance, and the kernel only compares against the resulting thresholds.
// Verified equal to transformers at every distance up to 511 for (32 buckets, max distance 128), the pair T5-v1.1 uses
// (tests/test_t5_host.py).  Other pairs are accepted but NOT verified: logf here and torch.log there may differ by an ulp, which
// at a bucket edge would move that edge by one position.
int bucket_of(int rel, int num_buckets, int max_distance) {
  const int half = num_buckets / 2;
  int b = rel > 0 ? half : 0;
  const int a = rel < 0 ? -rel : rel;
  const int max_exact = half / 2;
  if (a < max_exact) return b + a;
  const float v = logf((float)a / (float)max_exact) / (float)log((double)max_distance / (double)max_exact) * (float)(half - max_exact);
  int large = max_exact + (int)v;
  if (large > half - 1) large = half - 1;
  return b + large;
}

struct BucketThresholds { int first[32]; };   // first[b] = smallest distance whose bucket (of one sign) is >= b, b in (max_exact, half)

// out[h, d + n - 1] = table[bucket(d), h], d = key - query in (-n, n)
template <typename T>
__global__ void __launch_bounds__(THREADS)
k_t5_bias(const unsigned short* __restrict__ table, int half, int heads, int n, const BucketThresholds th, float* __restrict__ out) {
  const int L = 2 * n - 1, total = heads * L;
  const int max_exact = half / 2;
  for (int e = blockIdx.x * THREADS + threadIdx.x; e < total; e += gridDim.x * THREADS) {
    const int hd = e / L, d = e - hd * L - (n - 1);
    const int a = d < 0 ? -d : d;
    int b = a;
    if (a >= max_exact) {
      b = max_exact;
      for (int k = max_exact + 1; k < half; ++k) b += a >= th.first[k] ? 1 : 0;
    }
    if (d > 0) b += half;
    out[e] = T::to_f(table[b * heads + hd]);
  }
}

inline unsigned grid_for(long total) {
  long g = (total + THREADS - 1) / THREADS;
  return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int sdn_t5_bucket(int32_t relative_position, int32_t num_buckets, int32_t max_distance) {
  if (num_buckets < 4 || num_buckets > 64 || (num_buckets & 3) || max_distance <= num_buckets / 4) return SDN_E_INVALID;
  return bucket_of(relative_position, num_buckets, max_distance);
}

extern "C" int sdn_rmsnorm(int32_t dtype, const void* x, int32_t x_is_f32, int64_t rows, int32_t c, float eps, const float* weight,
                           void* out, void* stream) {
  if (!x || !weight || !out || rows < 0 || rows > 0x7fffffffL || c <= 0 || (c & 3) || dtype < 0 || dtype > 1 || !(eps >= 0.f)) return SDN_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(x) & (x_is_f32 ? 15 : 7)) || (reinterpret_cast<uintptr_t>(weight) & 15) ||
      (reinterpret_cast<uintptr_t>(out) & 7))
    return SDN_E_INVALID;
  if (rows == 0) return SDN_OK;
  unsigned short* o = (unsigned short*)out;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)rows), blk(THREADS);
  if (dtype == 1) {
    if (x_is_f32) hipLaunchKernelGGL((k_rmsnorm<SdnF16, true>), grid, blk, 0, st, x, c, eps, weight, o);
    else hipLaunchKernelGGL((k_rmsnorm<SdnF16, false>), grid, blk, 0, st, x, c, eps, weight, o);
  } else {
    if (x_is_f32) hipLaunchKernelGGL((k_rmsnorm<SdnBF16, true>), grid, blk, 0, st, x, c, eps, weight, o);
    else hipLaunchKernelGGL((k_rmsnorm<SdnBF16, false>), grid, blk, 0, st, x, c, eps, weight, o);
  }
  return sdn_launch_status();
}

extern "C" int sdn_embed_tokens(int32_t dtype, const int32_t* input_ids, const void* token_embedding, int64_t rows, int32_t hidden,
                                int32_t vocab, float* out, void* stream) {
  if (!input_ids || !token_embedding || !out || rows < 0 || hidden <= 0 || (hidden & 1) || vocab <= 0 || dtype < 0 || dtype > 1 ||
      (reinterpret_cast<uintptr_t>(token_embedding) & 3) || (reinterpret_cast<uintptr_t>(out) & 7))
    return SDN_E_INVALID;
  if (rows == 0) return SDN_OK;
  const dim3 grid(grid_for(rows * (hidden / 2))), blk(THREADS);
  if (dtype == 1)
    hipLaunchKernelGGL((k_embed_tokens<SdnF16>), grid, blk, 0, (hipStream_t)stream, input_ids, (const unsigned short*)token_embedding,
                       (long)rows, hidden, vocab, out);
  else
    hipLaunchKernelGGL((k_embed_tokens<SdnBF16>), grid, blk, 0, (hipStream_t)stream, input_ids, (const unsigned short*)token_embedding,
                       (long)rows, hidden, vocab, out);
  return sdn_launch_status();
}

extern "C" int sdn_t5_relative_bias(int32_t dtype, const void* table, int32_t num_buckets, int32_t max_distance, int32_t heads,
                                    int32_t n, float* out, void* stream) {
  if (!table || !out || heads <= 0 || n < 2 || n > 512 || dtype < 0 || dtype > 1 || num_buckets < 4 || num_buckets > 64 ||
      (num_buckets & 3) || max_distance <= num_buckets / 4 || (reinterpret_cast<uintptr_t>(out) & 3))
    return SDN_E_INVALID;
  const int half = num_buckets / 2, max_exact = half / 2;
  BucketThresholds th;
  for (int k = 0; k < 32; ++k) th.first[k] = 0x7fffffff;
  // buckets are monotone in the distance and saturate by max_distance: scan far enough to have seen the last one
  const int far = max_distance + 1 > n ? max_distance + 1 : n;
  for (int a = far; a >= max_exact; --a) {
    const int b = bucket_of(-a, num_buckets, max_distance);
    for (int k = max_exact + 1; k <= b && k < half; ++k) th.first[k] = a;
  }
  const dim3 grid(grid_for((long)heads * (2 * n - 1))), blk(THREADS);
  if (dtype == 1)
    hipLaunchKernelGGL((k_t5_bias<SdnF16>), grid, blk, 0, (hipStream_t)stream, (const unsigned short*)table, half, heads, n, th, out);
  else
    hipLaunchKernelGGL((k_t5_bias<SdnBF16>), grid, blk, 0, (hipStream_t)stream, (const unsigned short*)table, half, heads, n, th, out);
  return sdn_launch_status();
}
