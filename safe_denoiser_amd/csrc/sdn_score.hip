// The scoring head of the two image metrics the reference's result tables report (evaluations/fid.py): one scaled cosine per row of
// an embedding matrix.
//   CLIP score       torchmetrics' CLIPScore update arithmetic (third party; evaluations/base_image.py:145-157 drives it):
//                    img / img.norm(), txt / txt.norm(), 100 * (img * txt).sum(-1) per (image, caption) pair.
//   aesthetic score  AE.forward, evaluations/utils/aes.py:23-35: emb / emb.norm() through AE_MLP, which holds no activation and is
//                    therefore one affine map w . x + b (composed on the host, safe_denoiser_amd/metrics.py).
// One wave per row, one pass: sum x y, sum x^2 and (when y is normalised too) sum y^2 in f32, wave_sum, one store.
//   COCO CLIP score  Eval.clip_score of run_coco30k.py:217-234: the mean of the WHOLE image-by-prompt cosine matrix, one scalar
//                    (sdn_embed_cross_mean, at the end of this file).
#include <math.h>
#include <type_traits>

#include "sdn_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / SDN_WAVE;

struct StoreF32 {};      // tag: f32 storage (SdnBF16 / SdnF16 are the 16-bit ones)

template <typename T> struct Elem { typedef unsigned short type; };
template <> struct Elem<StoreF32> { typedef float type; };

template <typename T>
__device__ __forceinline__ float load1(const void* row, int c) {
  if constexpr (std::is_same<T, StoreF32>::value) return reinterpret_cast<const float*>(row)[c];
  else return T::to_f(reinterpret_cast<const unsigned short*>(row)[c]);
}

// elements c .. c + 3 of a row whose address at c is 8-byte (16-bit storage) or 16-byte (f32) aligned
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

// vec: every row of x and of y starts on a 16-byte boundary (the host checks pointer and pitch), so groups of four elements are
// fetched with one load each; the dim % 4 tail, and whole rows of an odd pitch, go element by element.  Nothing at or past
// column `dim` is read.
template <typename TX, typename TY>
__global__ void __launch_bounds__(THREADS)
k_embed_row_scores(const void* __restrict__ x, long ldx, const void* __restrict__ y, long ldy, int y_bcast, int rows, int dim, int vec,
                   int normalize_y, float scale, float bias, float* __restrict__ out) {
  const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                                         // wave-uniform
  const void* xr = reinterpret_cast<const typename Elem<TX>::type*>(x) + (size_t)row * ldx;
  const void* yr = reinterpret_cast<const typename Elem<TY>::type*>(y) + (y_bcast ? (size_t)0 : (size_t)row * ldy);
  float sxy = 0.f, sxx = 0.f, syy = 0.f;
  const int nvec = vec ? (dim & ~3) : 0;
  for (int c = lane * 4; c < nvec; c += SDN_WAVE * 4) {
    float a[4], b[4];
    load4<TX>(xr, c, a);
    load4<TY>(yr, c, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) { sxy = fmaf(a[e], b[e], sxy); sxx = fmaf(a[e], a[e], sxx); syy = fmaf(b[e], b[e], syy); }
  }
  for (int c = nvec + lane; c < dim; c += SDN_WAVE) {
    const float a = load1<TX>(xr, c), b = load1<TY>(yr, c);
    sxy = fmaf(a, b, sxy); sxx = fmaf(a, a, sxx); syy = fmaf(b, b, syy);
  }
  sxy = wave_sum(sxy); sxx = wave_sum(sxx);
  float den = sqrtf(sxx);
  if (normalize_y) den *= sqrtf(wave_sum(syy));
  if (lane == 0) out[row] = scale * (sxy / den) + bias;            // a zero row: 0 / 0 = NaN, as x / x.norm() gives
}

template <typename TX>
void launch_y(int dtype_y, dim3 grid, hipStream_t st, const void* x, long ldx, const void* y, long ldy, int y_bcast, int rows, int dim,
              int vec, int normalize_y, float scale, float bias, float* out) {
  if (dtype_y == 2)
    hipLaunchKernelGGL((k_embed_row_scores<TX, StoreF32>), grid, dim3(THREADS), 0, st, x, ldx, y, ldy, y_bcast, rows, dim, vec, normalize_y, scale, bias, out);
  else if (dtype_y == 1)
    hipLaunchKernelGGL((k_embed_row_scores<TX, SdnF16>), grid, dim3(THREADS), 0, st, x, ldx, y, ldy, y_bcast, rows, dim, vec, normalize_y, scale, bias, out);
  else
    hipLaunchKernelGGL((k_embed_row_scores<TX, SdnBF16>), grid, dim3(THREADS), 0, st, x, ldx, y, ldy, y_bcast, rows, dim, vec, normalize_y, scale, bias, out);
}

// ---- the COCO evaluator's head: the mean of the whole cosine matrix ---------------------------------------------------------------
// mean_ij <x^_i, y^_j> = (sum_i x^_i) . (sum_j y^_j) / (rx ry): the rx x ry matrix is never formed.
// k_cross_row_sums: two workgroups, one per matrix, each the only writer of its half of sums [2, dim].  Four rows at a time: wave w
// takes the norm of row r0 + w (one wave per row, as k_embed_row_scores), then every thread adds the four normalised rows, in row
// order, to the columns it owns (c = thread, thread + 256, ...).  The first group writes, so the scratch needs no zeroing; no atomics,
// so the result is the same bits on every run.  k_cross_dot: one workgroup, sum_c sums[0, c] sums[1, c] / (rx ry), one store.
template <typename T>
__device__ __forceinline__ void cross_matrix(const void* base, long ld, int rows, int dim, int vec, float* __restrict__ sums, float* den) {
  const typename Elem<T>::type* m = reinterpret_cast<const typename Elem<T>::type*>(base);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nvec = vec ? (dim & ~3) : 0;
  for (int r0 = 0; r0 < rows; r0 += ROWS_PER_BLOCK) {                // (the host keeps rows + ROWS_PER_BLOCK inside int)
    if (r0 + w < rows) {                                            // wave-uniform
      const void* row = m + (size_t)(r0 + w) * ld;
      float ss = 0.f;
      for (int c = lane * 4; c < nvec; c += SDN_WAVE * 4) {
        float a[4];
        load4<T>(row, c, a);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(a[e], a[e], ss);
      }
      for (int c = nvec + lane; c < dim; c += SDN_WAVE) { const float a = load1<T>(row, c); ss = fmaf(a, a, ss); }
      ss = sqrtf(wave_sum(ss));                                     // a zero row: 0 / 0 = NaN in every column, as x / x.norm() gives
      if (lane == 0) den[w] = ss;
    }
    __syncthreads();
    const int n = rows - r0 < ROWS_PER_BLOCK ? rows - r0 : ROWS_PER_BLOCK;
    for (int c = threadIdx.x; c < dim; c += THREADS) {
      float acc = r0 ? sums[c] : 0.f;
      for (int k = 0; k < n; ++k) acc += load1<T>(m + (size_t)(r0 + k) * ld, c) / den[k];
      sums[c] = acc;
    }
    __syncthreads();
  }
}

template <typename TX, typename TY>
__global__ void __launch_bounds__(THREADS)
k_cross_row_sums(const void* __restrict__ x, long ldx, int vecx, const void* __restrict__ y, long ldy, int vecy, int rx, int ry, int dim,
                 float* __restrict__ sums) {
  __shared__ float den[ROWS_PER_BLOCK];
  if (blockIdx.x == 0) cross_matrix<TX>(x, ldx, rx, dim, vecx, sums, den);
  else cross_matrix<TY>(y, ldy, ry, dim, vecy, sums + dim, den);
}

__global__ void __launch_bounds__(THREADS) k_cross_dot(const float* __restrict__ sums, int dim, float count, float* __restrict__ out) {
  __shared__ float red[ROWS_PER_BLOCK];
  float s = 0.f;
  for (int c = threadIdx.x; c < dim; c += THREADS) s = fmaf(sums[c], sums[dim + c], s);
  s = block_sum<ROWS_PER_BLOCK>(s, red);
  if (threadIdx.x == 0) out[0] = s / count;
}

template <typename TX>
void launch_cross_y(int dtype_y, hipStream_t st, const void* x, long ldx, int vecx, const void* y, long ldy, int vecy, int rx, int ry,
                    int dim, float* sums) {
  const dim3 grid(2);
  if (dtype_y == 2)
    hipLaunchKernelGGL((k_cross_row_sums<TX, StoreF32>), grid, dim3(THREADS), 0, st, x, ldx, vecx, y, ldy, vecy, rx, ry, dim, sums);
  else if (dtype_y == 1)
    hipLaunchKernelGGL((k_cross_row_sums<TX, SdnF16>), grid, dim3(THREADS), 0, st, x, ldx, vecx, y, ldy, vecy, rx, ry, dim, sums);
  else
    hipLaunchKernelGGL((k_cross_row_sums<TX, SdnBF16>), grid, dim3(THREADS), 0, st, x, ldx, vecx, y, ldy, vecy, rx, ry, dim, sums);
}

}  // namespace

extern "C" int sdn_embed_row_scores(const void* x, int32_t dtype_x, int64_t ldx, const void* y, int32_t dtype_y, int64_t ldy,
                                    int32_t y_rows, int32_t rows, int32_t dim, int32_t normalize_y, float scale, float bias, float* out,
                                    void* stream) {
  if (rows < 0 || dim < 1 || dtype_x < 0 || dtype_x > 2 || dtype_y < 0 || dtype_y > 2 || ldx < dim || ldy < dim) return SDN_E_INVALID;
  if (rows == 0) return SDN_OK;
  if (!x || !y || !out || (y_rows != 1 && y_rows != rows)) return SDN_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(out) & 3))
    return SDN_E_INVALID;
  const int64_t ex = dtype_x == 2 ? 4 : 2, ey = dtype_y == 2 ? 4 : 2;
  const int y_bcast = y_rows == 1;                                 // (rows == 1 too: the same row either way)
  // a pitch that is a multiple of 16 bytes puts every row on a 16-byte boundary: the vector path.  A row that is read alone
  // (rows == 1, the broadcast y) starts at the base pointer, whatever its pitch.
  const int vec = (rows == 1 || ((ldx * ex) & 15) == 0) && (y_bcast || ((ldy * ey) & 15) == 0);
  const dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
  hipStream_t st = (hipStream_t)stream;
  if (dtype_x == 2)
    launch_y<StoreF32>(dtype_y, grid, st, x, (long)ldx, y, (long)ldy, y_bcast, rows, dim, vec, normalize_y != 0, scale, bias, out);
  else if (dtype_x == 1)
    launch_y<SdnF16>(dtype_y, grid, st, x, (long)ldx, y, (long)ldy, y_bcast, rows, dim, vec, normalize_y != 0, scale, bias, out);
  else
    launch_y<SdnBF16>(dtype_y, grid, st, x, (long)ldx, y, (long)ldy, y_bcast, rows, dim, vec, normalize_y != 0, scale, bias, out);
  return sdn_launch_status();
}

extern "C" int sdn_embed_cross_mean(const void* x, int32_t dtype_x, int64_t ldx, int32_t rx, const void* y, int32_t dtype_y, int64_t ldy,
                                    int32_t ry, int32_t dim, float* scratch, float* out, void* stream) {
  if (!x || !y || !scratch || !out || dim < 1 || rx < 1 || ry < 1 || dtype_x < 0 || dtype_x > 2 || dtype_y < 0 || dtype_y > 2 ||
      ldx < dim || ldy < dim)
    return SDN_E_INVALID;
  if (dim > (1 << 30) || rx > (1 << 30) || ry > (1 << 30)) return SDN_E_INVALID;        // the kernels' int loop counters (sdn.h)
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(scratch) & 3) ||
      (reinterpret_cast<uintptr_t>(out) & 3))
    return SDN_E_INVALID;
  const int64_t ex = dtype_x == 2 ? 4 : 2, ey = dtype_y == 2 ? 4 : 2;
  // the vector loads need every row on a 16-byte boundary (sdn_embed_row_scores' rule): a pitch of whole 16 bytes, or a single row
  const int vecx = rx == 1 || ((ldx * ex) & 15) == 0, vecy = ry == 1 || ((ldy * ey) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype_x == 2)
    launch_cross_y<StoreF32>(dtype_y, st, x, (long)ldx, vecx, y, (long)ldy, vecy, rx, ry, dim, scratch);
  else if (dtype_x == 1)
    launch_cross_y<SdnF16>(dtype_y, st, x, (long)ldx, vecx, y, (long)ldy, vecy, rx, ry, dim, scratch);
  else
    launch_cross_y<SdnBF16>(dtype_y, st, x, (long)ldx, vecx, y, (long)ldy, vecy, rx, ry, dim, scratch);
  hipLaunchKernelGGL(k_cross_dot, dim3(1), dim3(THREADS), 0, st, (const float*)scratch, dim, (float)rx * (float)ry, out);
  return sdn_launch_status();
}
