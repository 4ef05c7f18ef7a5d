// Data-movement kernels of the Inception-v3 pool3 tower (the FID / KID feature extractor; plan: sdn_plan_inception.hip).  Every
// contraction of the tower is sdn_gemm_f32; what is here only moves or reduces NHWC f32 activations:
//   sdn_patch_rows_f32        the patch matrix of one convolution (any kh x kw, stride, zero padding)
//   sdn_pool3_f32             3x3 max pooling and the pad-excluding 3x3 average pooling, into a channel slice of a wider map
//   sdn_resize_bilinear_f32   F.interpolate(bilinear, align_corners=False) of NCHW [0, 1] pixels, then a x + b, into NHWC
//   sdn_spatial_mean_f32      AdaptiveAvgPool2d(1)
// All element offsets are 64-bit; every kernel is a grid-stride loop over independent outputs (no LDS, no inter-thread traffic).
#include <math.h>

#include "sdn_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int THREADS = 256;

struct PatchArgs {
  const float* in; float* out;
  long items;                 // output elements (VEC = 1) or quads (VEC = 4)
  int H, W, C, kh, kw, sh, sw, ph, pw, Ho, Wo, kpad;
};

// out[(b, oy, ox), (ky kw + kx) C + c] = in[b, oy sh - ph + ky, ox sw - pw + kx, c], zero for taps in the padding and for the
// columns kh kw C .. kpad.  VEC = 4 (C % 4 == 0): a quad of columns lies inside one tap, one 16-byte load and store.
template <int VEC>
__global__ void __launch_bounds__(THREADS) k_patch_rows_f32(const PatchArgs g) {
  const int kq = g.kpad / VEC, kvalid = g.kh * g.kw * g.C;
  for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < g.items; i += (long)gridDim.x * THREADS) {
    const long row = i / kq;
    const int k = (int)(i - row * kq) * VEC;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k < kvalid) {
      const int tap = k / g.C, c = k - tap * g.C;
      const int ky = tap / g.kw, kx = tap - ky * g.kw;
      const long b = row / ((long)g.Ho * g.Wo);
      const int p = (int)(row - b * g.Ho * g.Wo);
      const int oy = p / g.Wo, ox = p - oy * g.Wo;
      const int y = oy * g.sh - g.ph + ky, x = ox * g.sw - g.pw + kx;
      if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
        const float* src = g.in + ((b * g.H + y) * g.W + x) * g.C + c;
        if (VEC == 4) v = *reinterpret_cast<const f32x4*>(src);
        else v[0] = *src;
      }
    }
    if (VEC == 4) *reinterpret_cast<f32x4*>(g.out + row * g.kpad + k) = v;
    else g.out[row * g.kpad + k] = v[0];
  }
}

// 3x3 window at stride s, zero-free padding p: mode 0 = max over the taps inside the map (a NaN wins, as in torch), mode 1 = their
// sum in (ky, kx) order divided by their count (count_include_pad=False).  out[(b, oy, ox), c0 + c], row stride ldo.
__global__ void __launch_bounds__(THREADS)
k_pool3_f32(const float* __restrict__ in, float* __restrict__ out, long items, int H, int W, int C, int Ho, int Wo, int stride, int pad,
            int mode, int ldo, int c0) {
  for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < items; i += (long)gridDim.x * THREADS) {
    const long row = i / C;
    const int c = (int)(i - row * C);
    const long b = row / ((long)Ho * Wo);
    const int p = (int)(row - b * Ho * Wo);
    const int oy = p / Wo, ox = p - oy * Wo;
    float m = -INFINITY, sum = 0.f;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
      const int y = oy * stride - pad + ky;
      if (y < 0 || y >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int x = ox * stride - pad + kx;
        if (x < 0 || x >= W) continue;
        const float v = in[((b * H + y) * W + x) * C + c];
        if (v > m || v != v) m = v;
        sum += v;
        ++cnt;
      }
    }
    out[row * ldo + c0 + c] = mode == 0 ? m : sum / (float)cnt;
  }
}

// Bilinear resize without antialiasing, align_corners=False: the source coordinate of output index d on an axis of `in` samples
// resized to `on` is ((2 d + 1) in - on) / (2 on), clamped at 0 -- formed in INTEGERS, so the cell index is exact and the weight
// is the correctly rounded f32 of an exact fraction (torch forms it in f32: off by up to in * 2^-24).  The four taps are combined
// as torch's GPU kernel does: w0y (w0x p00 + w1x p01) + w1y (w0x p10 + w1x p11); then out = a v + b.  identity: copy, a v + b.
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap tap_of(int d, int in, int on) {
  long num = (long)(2 * d + 1) * in - on;
  if (num < 0) num = 0;
  const long den = 2L * on;
  const int i0 = (int)(num / den);
  Tap t;
  t.i0 = i0; t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  t.w1 = (float)(num - (long)i0 * den) / (float)den;      // both exact in f32 (< 2^24): one rounding
  t.w0 = 1.f - t.w1;
  return t;
}

__global__ void __launch_bounds__(THREADS)
k_resize_bilinear_f32(const float* __restrict__ in, float* __restrict__ out, long items, int H, int W, int Ho, int Wo, float a, float b_,
                      int identity) {
  for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < items; i += (long)gridDim.x * THREADS) {
    const int c = (int)(i % 3);
    const long px = i / 3;
    const int ox = (int)(px % Wo);
    const long r = px / Wo;
    const int oy = (int)(r % Ho);
    const long b = r / Ho;
    const float* plane = in + (b * 3 + c) * (long)H * W;
    float v;
    if (identity) {
      v = plane[(long)oy * W + ox];
    } else {
      const Tap ty = tap_of(oy, H, Ho), tx = tap_of(ox, W, Wo);
      const float* r0 = plane + (long)ty.i0 * W;
      const float* r1 = plane + (long)ty.i1 * W;
      v = ty.w0 * (tx.w0 * r0[tx.i0] + tx.w1 * r0[tx.i1]) + ty.w1 * (tx.w0 * r1[tx.i0] + tx.w1 * r1[tx.i1]);
    }
    out[i] = a * v + b_;
  }
}

// out[b, c] = mean over p of in[b, p, c]: the hw terms added in p order in DOUBLE, divided and rounded to f32 once.
__global__ void __launch_bounds__(THREADS)
k_spatial_mean_f32(const float* __restrict__ in, float* __restrict__ out, long items, int hw, int C) {
  for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < items; i += (long)gridDim.x * THREADS) {
    const long b = i / C;
    const int c = (int)(i - b * C);
    const float* src = in + b * (long)hw * C + c;
    double s = 0.0;
    for (int p = 0; p < hw; ++p) s += (double)src[(long)p * C];
    out[i] = (float)(s / (double)hw);
  }
}

unsigned grid_for(long items) {
  long g = (items + THREADS - 1) / THREADS;
  return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr long MAX_ITEMS = 1L << 40;      // element counts stay far inside 64-bit offsets of 4-byte elements

}  // namespace

extern "C" int sdn_patch_rows_f32(const float* in, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                                  int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t kpad, float* out,
                                  void* stream) {
  if (!in || !out || batch < 0 || h <= 0 || w <= 0 || c <= 0 || kh <= 0 || kw <= 0 || kh > 16 || kw > 16 || stride_h <= 0 ||
      stride_w <= 0 || pad_h < 0 || pad_w < 0 || pad_h >= kh || pad_w >= kw || h > 16384 || w > 16384 || c > 65536)
    return SDN_E_INVALID;
  if (h + 2 * pad_h < kh || w + 2 * pad_w < kw) return SDN_E_INVALID;
  const long kvalid = (long)kh * kw * c;
  if (kpad < kvalid || (kpad % 64) != 0 || !aligned(in, 16) || !aligned(out, 16)) return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  PatchArgs g;
  g.in = in; g.out = out; g.H = h; g.W = w; g.C = c; g.kh = kh; g.kw = kw; g.sh = stride_h; g.sw = stride_w; g.ph = pad_h; g.pw = pad_w;
  g.Ho = (h + 2 * pad_h - kh) / stride_h + 1; g.Wo = (w + 2 * pad_w - kw) / stride_w + 1; g.kpad = kpad;
  const long rows = (long)batch * g.Ho * g.Wo;
  if (rows * kpad > MAX_ITEMS) return SDN_E_INVALID;
  if ((c & 3) == 0) {
    g.items = rows * (kpad / 4);
    hipLaunchKernelGGL(k_patch_rows_f32<4>, dim3(grid_for(g.items)), dim3(THREADS), 0, (hipStream_t)stream, g);
  } else {
    g.items = rows * kpad;
    hipLaunchKernelGGL(k_patch_rows_f32<1>, dim3(grid_for(g.items)), dim3(THREADS), 0, (hipStream_t)stream, g);
  }
  return sdn_launch_status();
}

extern "C" int sdn_pool3_f32(int32_t mode, const float* in, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t stride,
                             int32_t pad, float* out, int32_t ldo, int32_t c0, void* stream) {
  if (!in || !out || batch < 0 || h <= 0 || w <= 0 || c <= 0 || (mode != SDN_POOL_MAX && mode != SDN_POOL_AVG_NOPAD) ||
      (stride != 1 && stride != 2) || (pad != 0 && pad != 1) || h + 2 * pad < 3 || w + 2 * pad < 3 || h > 16384 || w > 16384 ||
      c > 65536 || c0 < 0 || ldo < c0 + c || !aligned(in, 4) || !aligned(out, 4))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const int Ho = (h + 2 * pad - 3) / stride + 1, Wo = (w + 2 * pad - 3) / stride + 1;     // floor: ceil_mode=False
  const long items = (long)batch * Ho * Wo * c;
  if ((long)batch * Ho * Wo * ldo > MAX_ITEMS) return SDN_E_INVALID;
  hipLaunchKernelGGL(k_pool3_f32, dim3(grid_for(items)), dim3(THREADS), 0, (hipStream_t)stream, in, out, items, h, w, c, Ho, Wo, stride,
                     pad, mode, ldo, c0);
  return sdn_launch_status();
}

extern "C" int sdn_resize_bilinear_f32(const float* in_nchw, int32_t batch, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                                       float scale, float shift, float* out_nhwc, void* stream) {
  if (!in_nchw || !out_nhwc || batch < 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0 || h > 8192 || w > 8192 || out_h > 8192 ||
      out_w > 8192 || !aligned(in_nchw, 4) || !aligned(out_nhwc, 4))
    return SDN_E_INVALID;                                       // (the fraction's two integers are below 2 * 8192: exact in f32)
  if (batch == 0) return SDN_OK;
  const long items = (long)batch * out_h * out_w * 3;
  hipLaunchKernelGGL(k_resize_bilinear_f32, dim3(grid_for(items)), dim3(THREADS), 0, (hipStream_t)stream, in_nchw, out_nhwc, items, h, w,
                     out_h, out_w, scale, shift, (h == out_h && w == out_w) ? 1 : 0);
  return sdn_launch_status();
}

extern "C" int sdn_spatial_mean_f32(const float* in, int32_t batch, int32_t hw, int32_t c, float* out, void* stream) {
  if (!in || !out || batch < 0 || hw <= 0 || c <= 0 || hw > (1 << 24) || c > 65536 || !aligned(in, 4) || !aligned(out, 4))
    return SDN_E_INVALID;
  if (batch == 0) return SDN_OK;
  const long items = (long)batch * c;
  hipLaunchKernelGGL(k_spatial_mean_f32, dim3(grid_for(items)), dim3(THREADS), 0, (hipStream_t)stream, in, out, items, hw, c);
  return sdn_launch_status();
}
