// Building blocks of the CLIP ViT vision tower (transformers CLIPVisionModelWithProjection, third party; the OpenAI ViT-L/14 image
// encoder behind the reference's Q16 classifier) and of CLIP's image preprocessing: the patch rows the patch convolution reads as
// a GEMM operand, the embedding row kernel (class token / patch projection + position embedding, then pre_layrnorm), post_layernorm
// on the class rows, Pillow's 8-bit resampling (square and rectangular) and the uint8 -> normalised f32 map.  The encoder layers are plan GEMMs,
// row LayerNorms and the d = 64 attention kernel (sdn_plan_vision.hip).
#include <math.h>

#include "sdn_common.h"

namespace {

constexpr int THREADS = 256;

// ---- patch rows ---------------------------------------------------------------------------------------------------------------
// One thread per PAIR of output columns (one 32-bit store).  Column j of row (b, py, px) is pixel (c, py p + ky, px p + kx) with
// j = c p^2 + ky p + kx -- the flattening of the conv weight [hidden, 3, p, p] -- and zero from 3 p^2 on.
template <typename T>
__global__ void __launch_bounds__(THREADS)
k_clip_patch_rows(const float* __restrict__ pix, long pairs, int S, int p, int g, int kpad, unsigned* __restrict__ out) {
  const int kp2 = kpad >> 1, pp = p * p, kreal = 3 * pp;
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < pairs; e += (long)gridDim.x * THREADS) {
    const long row = e / kp2;
    const int j0 = (int)(e - row * kp2) * 2;
    const long b = row / (g * g);
    const int pr = (int)(row - b * (g * g)), py = pr / g, px = pr - py * g;
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = j0 + h;
      if (j < kreal) {
        const int c = j / pp, r = j - c * pp, ky = r / p, kx = r - ky * p;
        v[h] = pix[((b * 3 + c) * S + (py * p + ky)) * (long)S + (px * p + kx)];
      } else {
        v[h] = 0.f;
      }
    }
    out[e] = T::pack2(v[0], v[1]);
  }
}

// ---- row LayerNorms -----------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load4(const unsigned short* row, int c, float (&v)[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(row + c);
  v[0] = T::to_f(t.x & 0xffff); v[1] = T::to_f(t.x >> 16); v[2] = T::to_f(t.y & 0xffff); v[3] = T::to_f(t.y >> 16);
}

// v = a[c .. c + 4) (16-bit row, or the f32 row `af` when a == nullptr) + b[c .. c + 4) (16-bit row, nullable)
template <typename T>
__device__ __forceinline__ void sum4(const unsigned short* a, const float* af, const unsigned short* b, int c, float (&v)[4]) {
  if (a) {
    load4<T>(a, c, v);
  } else {
    const sdn_f32x4 t = *reinterpret_cast<const sdn_f32x4*>(af + c);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  if (b) {
    float w[4];
    load4<T>(b, c, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += w[e];
  }
}

// LayerNorm of one row a (+ b): mean first, variance around the mean second (the row sits in L2), all in f32; the whole workgroup.
template <typename T>
__device__ __forceinline__ void ln_row(const unsigned short* a, const float* af, const unsigned short* b, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, int C, float eps, unsigned short* __restrict__ out, float* red) {
  float s = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    sum4<T>(a, af, b, c, v);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = block_sum<4>(s, red) / (float)C;
  float q = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    sum4<T>(a, af, b, c, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = v[e] - mean; q = fmaf(d, d, q); }
  }
  const float rstd = 1.0f / sqrtf(block_sum<4>(q, red + 4) / (float)C + eps);
  for (int c = threadIdx.x * 4; c < C; c += THREADS * 4) {
    float v[4];
    sum4<T>(a, af, b, c, v);
    const sdn_f32x4 g = *reinterpret_cast<const sdn_f32x4*>(gamma + c), bt = *reinterpret_cast<const sdn_f32x4*>(beta + c);
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (v[e] - mean) * rstd * g[e] + bt[e];
    uint2 pk; pk.x = T::pack2(r[0], r[1]); pk.y = T::pack2(r[2], r[3]);
    *reinterpret_cast<uint2*>(out + c) = pk;
  }
}

// one workgroup per output row (b, t): t == 0 is the class token, t >= 1 patch t - 1 of image b
template <typename T>
__global__ void __launch_bounds__(THREADS)
k_clip_vision_embed(const unsigned short* __restrict__ proj, const float* __restrict__ cls, const unsigned short* __restrict__ pos,
                    const float* __restrict__ gamma, const float* __restrict__ beta, int n, int C, float eps,
                    unsigned short* __restrict__ out) {
  __shared__ float red[8];
  const long row = blockIdx.x;
  const long b = row / n;
  const int t = (int)(row - b * n);
  const unsigned short* a = t == 0 ? nullptr : proj + (b * (n - 1) + (t - 1)) * (long)C;
  ln_row<T>(a, cls, pos + (long)t * C, gamma, beta, C, eps, out + row * C, red);
}

// one workgroup per sequence: LayerNorm of its row 0
template <typename T>
__global__ void __launch_bounds__(THREADS)
k_clip_class_rows(const unsigned short* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, int n, int C,
                  float eps, unsigned short* __restrict__ out) {
  __shared__ float red[8];
  const long b = blockIdx.x;
  ln_row<T>(x + b * n * (long)C, nullptr, nullptr, gamma, beta, C, eps, out + b * C, red);
}

// ---- Pillow's 8-bit resampling --------------------------------------------------------------------------------------------------
// One pass along one axis: out[b, y, x, :] over `len` source positions `step` bytes apart.  Horizontal: lines = S rows of S pixels,
// T outputs per line; vertical: the same with the roles of the axes exchanged.  One thread per output pixel (3 channels).
__global__ void __launch_bounds__(THREADS)
k_resize_pass(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const int* __restrict__ coeffs,
              const int* __restrict__ bounds, int ksize, long total, int T, int in_len, int vertical, int in_h, int in_w, int out_h, int out_w) {
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < total; e += (long)gridDim.x * THREADS) {
    const long b = e / ((long)out_h * out_w);
    const int r = (int)(e - b * ((long)out_h * out_w)), y = r / out_w, x = r - y * out_w;
    const int i = vertical ? y : x;                                   // output index along the resampled axis
    int lo = bounds[2 * i], cnt = bounds[2 * i + 1];
    // a table that names taps outside the input is not followed there
    if (lo < 0) lo = 0;
    if (cnt > ksize) cnt = ksize;
    if (cnt > in_len - lo) cnt = in_len - lo;
    const int* k = coeffs + (long)i * ksize;
    const unsigned char* src = in + ((b * in_h + (vertical ? lo : y)) * (long)in_w + (vertical ? x : lo)) * 3;
    const long step = vertical ? (long)in_w * 3 : 3;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int t = 0; t < cnt; ++t) {
      const int w = k[t];
      s0 += (int)src[0] * w; s1 += (int)src[1] * w; s2 += (int)src[2] * w;
      src += step;
    }
    s0 >>= 22; s1 >>= 22; s2 >>= 22;
    unsigned char* dst = out + e * 3;
    dst[0] = (unsigned char)(s0 < 0 ? 0 : (s0 > 255 ? 255 : s0));
    dst[1] = (unsigned char)(s1 < 0 ? 0 : (s1 > 255 ? 255 : s1));
    dst[2] = (unsigned char)(s2 < 0 ? 0 : (s2 > 255 ? 255 : s2));
  }
}

struct Norm3 { float mean[3], stdv[3]; };

// one thread per pixel: NHWC uint8 -> NCHW f32
__global__ void __launch_bounds__(THREADS)
k_clip_normalize(const unsigned char* __restrict__ in, long pixels, long plane, Norm3 nm, float* __restrict__ out) {
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < pixels; e += (long)gridDim.x * THREADS) {
    const long b = e / plane, r = e - b * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)in[e * 3 + c] / 255.0f;
      out[(b * 3 + c) * plane + r] = (u - nm.mean[c]) / nm.stdv[c];
    }
  }
}

// The LAST pass of a rectangular resize (or, with coeffs == nullptr, the copy Pillow makes when neither axis changes length): the
// arithmetic of k_resize_pass, then the clipped 8-bit value goes from registers to out_u8 [B, out_h, out_w, 3] and / or, through
// k_clip_normalize's f32 operations in their order, to the planes out_f32 [B, 3, out_h, out_w].  One thread per output pixel, x
// fastest: a wave stores 64 consecutive floats of each plane.
__global__ void __launch_bounds__(THREADS)
k_resize_last(const unsigned char* __restrict__ in, unsigned char* __restrict__ out_u8, float* __restrict__ out_f32, Norm3 nm,
              const int* __restrict__ coeffs, const int* __restrict__ bounds, int ksize, long total, int in_len, int vertical, int in_h,
              int in_w, int out_h, int out_w) {
  const long plane = (long)out_h * out_w;
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < total; e += (long)gridDim.x * THREADS) {
    const long b = e / plane;
    const int r = (int)(e - b * plane), y = r / out_w, x = r - y * out_w;
    int v[3];
    if (coeffs) {
      const int i = vertical ? y : x;
      int lo = bounds[2 * i], cnt = bounds[2 * i + 1];
      if (lo < 0) lo = 0;
      if (cnt > ksize) cnt = ksize;
      if (cnt > in_len - lo) cnt = in_len - lo;
      const int* k = coeffs + (long)i * ksize;
      const unsigned char* src = in + ((b * in_h + (vertical ? lo : y)) * (long)in_w + (vertical ? x : lo)) * 3;
      const long step = vertical ? (long)in_w * 3 : 3;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int t = 0; t < cnt; ++t) {
        const int w = k[t];
        s0 += (int)src[0] * w; s1 += (int)src[1] * w; s2 += (int)src[2] * w;
        src += step;
      }
      s0 >>= 22; s1 >>= 22; s2 >>= 22;
      v[0] = s0 < 0 ? 0 : (s0 > 255 ? 255 : s0);
      v[1] = s1 < 0 ? 0 : (s1 > 255 ? 255 : s1);
      v[2] = s2 < 0 ? 0 : (s2 > 255 ? 255 : s2);
    } else {
      const unsigned char* src = in + e * 3;                           // same shape in and out
      v[0] = src[0]; v[1] = src[1]; v[2] = src[2];
    }
    if (out_u8) {
      unsigned char* dst = out_u8 + e * 3;
      dst[0] = (unsigned char)v[0]; dst[1] = (unsigned char)v[1]; dst[2] = (unsigned char)v[2];
    }
    if (out_f32) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = (float)(unsigned char)v[c] / 255.0f;
        out_f32[(b * 3 + c) * plane + r] = (u - nm.mean[c]) / nm.stdv[c];
      }
    }
  }
}

unsigned grid_for(long items) {
  long g = (items + THREADS - 1) / THREADS;
  return (unsigned)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int sdn_clip_patch_rows(int32_t dtype, const float* pixels, int32_t batch, int32_t image_size, int32_t patch_size, int32_t kpad,
                                   void* out, void* stream) {
  if (!pixels || !out || batch < 0 || image_size <= 0 || patch_size <= 0 || image_size > 4096 || image_size % patch_size != 0 ||
      kpad < 3 * patch_size * patch_size || (kpad & 7) || dtype < 0 || dtype > 1 || !aligned(pixels, 4) || !aligned(out, 16))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const int g = image_size / patch_size;
  const long pairs = (long)batch * g * g * (kpad / 2);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    hipLaunchKernelGGL((k_clip_patch_rows<SdnF16>), dim3(grid_for(pairs)), dim3(THREADS), 0, st, pixels, pairs, image_size, patch_size, g, kpad, (unsigned*)out);
  else
    hipLaunchKernelGGL((k_clip_patch_rows<SdnBF16>), dim3(grid_for(pairs)), dim3(THREADS), 0, st, pixels, pairs, image_size, patch_size, g, kpad, (unsigned*)out);
  return sdn_launch_status();
}

extern "C" int sdn_clip_vision_embed(int32_t dtype, const void* patch_proj, const float* class_embedding, const void* position_embedding,
                                     const float* gamma, const float* beta, int32_t batch, int32_t tokens, int32_t hidden, float eps,
                                     void* out, void* stream) {
  if (!patch_proj || !class_embedding || !position_embedding || !gamma || !beta || !out || batch < 0 || tokens < 2 || tokens > 65536 ||
      hidden <= 0 || (hidden & 3) || dtype < 0 || dtype > 1 || !(eps >= 0.f) || (long)batch * tokens > 0x7fffffffL)
    return SDN_E_INVALID;
  if (!aligned(patch_proj, 8) || !aligned(position_embedding, 8) || !aligned(out, 8) || !aligned(class_embedding, 16) || !aligned(gamma, 16) ||
      !aligned(beta, 16))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const dim3 grid((unsigned)(batch * tokens)), blk(THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    hipLaunchKernelGGL((k_clip_vision_embed<SdnF16>), grid, blk, 0, st, (const unsigned short*)patch_proj, class_embedding,
                       (const unsigned short*)position_embedding, gamma, beta, tokens, hidden, eps, (unsigned short*)out);
  else
    hipLaunchKernelGGL((k_clip_vision_embed<SdnBF16>), grid, blk, 0, st, (const unsigned short*)patch_proj, class_embedding,
                       (const unsigned short*)position_embedding, gamma, beta, tokens, hidden, eps, (unsigned short*)out);
  return sdn_launch_status();
}

extern "C" int sdn_clip_class_rows(int32_t dtype, const void* x, const float* gamma, const float* beta, int32_t batch, int32_t seq_len,
                                   int32_t hidden, float eps, void* out, void* stream) {
  if (!x || !gamma || !beta || !out || batch < 0 || seq_len <= 0 || seq_len > 65536 || hidden <= 0 || (hidden & 3) || dtype < 0 ||
      dtype > 1 || !(eps >= 0.f))
    return SDN_E_INVALID;
  if (!aligned(x, 8) || !aligned(out, 8) || !aligned(gamma, 16) || !aligned(beta, 16)) return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const dim3 grid((unsigned)batch), blk(THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    hipLaunchKernelGGL((k_clip_class_rows<SdnF16>), grid, blk, 0, st, (const unsigned short*)x, gamma, beta, seq_len, hidden, eps, (unsigned short*)out);
  else
    hipLaunchKernelGGL((k_clip_class_rows<SdnBF16>), grid, blk, 0, st, (const unsigned short*)x, gamma, beta, seq_len, hidden, eps, (unsigned short*)out);
  return sdn_launch_status();
}

extern "C" int sdn_image_resize_u8(const uint8_t* in, int32_t batch, int32_t in_size, int32_t out_size, const int32_t* coeffs,
                                   const int32_t* bounds, int32_t ksize, uint8_t* tmp, uint8_t* out, void* stream) {
  if (!in || !coeffs || !bounds || !tmp || !out || batch < 0 || in_size <= 0 || in_size > 16384 || out_size <= 0 || out_size > 16384 ||
      ksize <= 0 || ksize > 4096 || !aligned(coeffs, 4) || !aligned(bounds, 4))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = in_size, T = out_size;
  const long n1 = (long)batch * S * T, n2 = (long)batch * T * T;
  hipLaunchKernelGGL(k_resize_pass, dim3(grid_for(n1)), dim3(THREADS), 0, st, in, tmp, coeffs, bounds, ksize, n1, T, S, 0, S, S, S, T);
  hipLaunchKernelGGL(k_resize_pass, dim3(grid_for(n2)), dim3(THREADS), 0, st, (const unsigned char*)tmp, out, coeffs, bounds, ksize, n2, T, S, 1,
                     S, T, T, T);
  return sdn_launch_status();
}

extern "C" int sdn_image_resize_rect_u8(const uint8_t* in, int32_t batch, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                                        const int32_t* coeffs_x, const int32_t* bounds_x, int32_t ksize_x, const int32_t* coeffs_y,
                                        const int32_t* bounds_y, int32_t ksize_y, uint8_t* tmp, uint8_t* out_u8, float* out_f32,
                                        float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, void* stream) {
  auto dim_ok = [](int32_t d) { return d >= 1 && d <= 16384; };
  if (!in || (!out_u8 && !out_f32) || batch < 0 || !dim_ok(in_h) || !dim_ok(in_w) || !dim_ok(out_h) || !dim_ok(out_w) ||
      !(std_r > 0.f) || !(std_g > 0.f) || !(std_b > 0.f) || !aligned(out_f32, 4))
    return SDN_E_INVALID;
  // an axis that keeps its length has no pass and no tables; one that changes needs both tables
  const bool horizontal = in_w != out_w, vertical = in_h != out_h;
  if (horizontal ? (!coeffs_x || !bounds_x || ksize_x <= 0 || ksize_x > 4096 || !aligned(coeffs_x, 4) || !aligned(bounds_x, 4))
                 : (coeffs_x || bounds_x))
    return SDN_E_INVALID;
  if (vertical ? (!coeffs_y || !bounds_y || ksize_y <= 0 || ksize_y > 4096 || !aligned(coeffs_y, 4) || !aligned(bounds_y, 4))
               : (coeffs_y || bounds_y))
    return SDN_E_INVALID;
  if (horizontal && vertical && !tmp) return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  hipStream_t st = (hipStream_t)stream;
  const Norm3 nm{{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
  const long n_out = (long)batch * out_h * out_w;
  const dim3 grid(grid_for(n_out)), blk(THREADS);
  if (horizontal && vertical) {
    const long n1 = (long)batch * in_h * out_w;
    hipLaunchKernelGGL(k_resize_pass, dim3(grid_for(n1)), blk, 0, st, in, tmp, coeffs_x, bounds_x, ksize_x, n1, out_w, in_w, 0, in_h, in_w,
                       in_h, out_w);
    hipLaunchKernelGGL(k_resize_last, grid, blk, 0, st, (const unsigned char*)tmp, out_u8, out_f32, nm, coeffs_y, bounds_y, ksize_y, n_out,
                       in_h, 1, in_h, out_w, out_h, out_w);
  } else if (horizontal) {
    hipLaunchKernelGGL(k_resize_last, grid, blk, 0, st, in, out_u8, out_f32, nm, coeffs_x, bounds_x, ksize_x, n_out, in_w, 0, in_h, in_w,
                       out_h, out_w);
  } else if (vertical) {
    hipLaunchKernelGGL(k_resize_last, grid, blk, 0, st, in, out_u8, out_f32, nm, coeffs_y, bounds_y, ksize_y, n_out, in_h, 1, in_h, in_w,
                       out_h, out_w);
  } else {
    hipLaunchKernelGGL(k_resize_last, grid, blk, 0, st, in, out_u8, out_f32, nm, (const int*)nullptr, (const int*)nullptr, 0, n_out, 0, 0,
                       in_h, in_w, out_h, out_w);
  }
  return sdn_launch_status();
}

extern "C" int sdn_clip_normalize_u8(const uint8_t* in, int32_t batch, int32_t size, float mean_r, float mean_g, float mean_b, float std_r,
                                     float std_g, float std_b, float* out, void* stream) {
  if (!in || !out || batch < 0 || size <= 0 || size > 16384 || !(std_r > 0.f) || !(std_g > 0.f) || !(std_b > 0.f) || !aligned(out, 4))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const long plane = (long)size * size, pixels = plane * batch;
  const Norm3 nm{{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
  hipLaunchKernelGGL(k_clip_normalize, dim3(grid_for(pixels)), dim3(THREADS), 0, (hipStream_t)stream, in, pixels, plane, nm, out);
  return sdn_launch_status();
}
