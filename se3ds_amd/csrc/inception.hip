// Inception-v3 evaluator kernels (utils/inception_utils.py, utils/eval_metric.py EvalMetric):
// the fused augment + crop + resize + renormalise gather that builds the network input, the Keras
// pooling layers of InceptionV3 (3x3/s2 VALID max, 3x3/s1 SAME average), the global average pool,
// the row softmax of the `predictions` layer, and the binary64 feature moments behind the FID.
// The convolutions run on se3ds_conv2d_fwd (conv.hip) with the batch norm folded into them.
// Compiled with -ffp-contract=off: the preprocess gather must round every fp32 op as
// se3ds_resize does (geom.hip); the moments use explicit fma().
#include "common.h"

namespace se3ds {
namespace {

constexpr int kB = 256;

__device__ __forceinline__ int floormod(int a, int m) {
  const int r = a % m;
  return r < 0 ? r + m : r;
}

// ------------------------------------------------------------------------------ preprocess
// out[b, oy, ox, k] = clip(resize(crop(flip(roll(x))))[oy, ox, k] * 2 - 1, -1, 1).
//   roll / flip: indoor_datasets.augment (reference datasets/indoor_datasets.py:34-61) with the
//     per-image draw rf[b] = (roll, flip): rolled[j] = x[(j - roll) mod W], flipped[j] = v[W-1-j];
//   crop: crop_pano(resize_to_original=False) keeps rows [crop, H - crop);
//   resize: tf.image.resize bilinear, half-pixel centres, no antialias -- the arithmetic of
//     resize_bilinear_kernel (geom.hip) operation for operation, on the cropped grid;
//   renormalise: inception_utils.get_inception, clip(x * 2 - 1, -1, 1).
// The augment only permutes columns, so it applies to the resize's tap columns.
template <typename TO>
__global__ void __launch_bounds__(kB)
preprocess_kernel(const float* __restrict__ x, int n, int h, int w, const int32_t* __restrict__ rf,
                  int crop, int oh, int ow, TO* __restrict__ y) {
  const int ch = h - 2 * crop;
  const float sy = (float)ch / (float)oh, sx = (float)w / (float)ow;
  const int64_t total = (int64_t)n * oh * ow * 3;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kB) {
    const int k = (int)(i % 3);
    const int64_t p = i / 3;
    const int ox = (int)(p % ow);
    const int64_t q = p / ow;
    const int oy = (int)(q % oh), b = (int)(q / oh);
    const float fy = ((float)oy + 0.5f) * sy - 0.5f, fx = ((float)ox + 0.5f) * sx - 0.5f;
    const float ly = floorf(fy), lx = floorf(fx);
    const float ty = fy - ly, tx = fx - lx;
    int y0 = (int)ly, x0 = (int)lx, y1 = y0 + 1, x1 = x0 + 1;
    y0 = y0 < 0 ? 0 : (y0 > ch - 1 ? ch - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > ch - 1 ? ch - 1 : y1);
    x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0);
    x1 = x1 < 0 ? 0 : (x1 > w - 1 ? w - 1 : x1);
    if (rf != nullptr) {
      const int roll = rf[2 * b], flip = rf[2 * b + 1];
      if (flip) { x0 = w - 1 - x0; x1 = w - 1 - x1; }
      x0 = floormod(x0 - roll, w);
      x1 = floormod(x1 - roll, w);
    }
    const float* base = x + ((int64_t)b * h + crop) * w * 3 + k;
    const float v00 = base[((int64_t)y0 * w + x0) * 3], v01 = base[((int64_t)y0 * w + x1) * 3];
    const float v10 = base[((int64_t)y1 * w + x0) * 3], v11 = base[((int64_t)y1 * w + x1) * 3];
    const float top = v00 + (v01 - v00) * tx, bot = v10 + (v11 - v10) * tx;
    float v = top + (bot - top) * ty;
    v = v * 2.f - 1.f;
    v = fminf(fmaxf(v, -1.f), 1.f);
    VT<TO>::st1(y + i, v);
  }
}

// ------------------------------------------------------------------------------ pooling
// Keras MaxPooling2D((3, 3), strides=(2, 2)) 'valid' and AveragePooling2D((3, 3), strides=(1, 1),
// padding='same') (TF: padded taps are not counted in the divisor).  Input dense (n,h,w,c);
// output pixel rows have yc channels and this layer fills [yc0, yc0 + c).
template <typename T>
__global__ void __launch_bounds__(kB)
maxpool3s2_kernel(const T* __restrict__ x, int n, int h, int w, int c, int oh, int ow,
                  T* __restrict__ y, int yc, int yc0) {
  const int64_t total = (int64_t)n * oh * ow * c;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kB) {
    const int k = (int)(i % c);
    const int64_t p = i / c;
    const int ox = (int)(p % ow);
    const int64_t q = p / ow;
    const int oy = (int)(q % oh), b = (int)(q / oh);
    const T* base = x + (((int64_t)b * h + 2 * oy) * w + 2 * ox) * c + k;
    float m = VT<T>::ld1(base);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float v = VT<T>::ld1(base + ((int64_t)dy * w + dx) * c);
        m = v > m ? v : m;
      }
    VT<T>::st1(y + p * yc + yc0 + k, m);
  }
}

template <typename T>
__global__ void __launch_bounds__(kB)
avgpool3s1_kernel(const T* __restrict__ x, int n, int h, int w, int c, T* __restrict__ y, int yc,
                  int yc0) {
  const int64_t total = (int64_t)n * h * w * c;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kB) {
    const int k = (int)(i % c);
    const int64_t p = i / c;
    const int ox = (int)(p % w);
    const int64_t q = p / w;
    const int oy = (int)(q % h), b = (int)(q / h);
    float s = 0.f;
    int cnt = 0;
    for (int yy = oy - 1; yy <= oy + 1; ++yy) {
      if (yy < 0 || yy >= h) continue;
      for (int xx = ox - 1; xx <= ox + 1; ++xx) {
        if (xx < 0 || xx >= w) continue;
        s += VT<T>::ld1(x + (((int64_t)b * h + yy) * w + xx) * c + k);
        ++cnt;
      }
    }
    VT<T>::st1(y + p * yc + yc0 + k, s / (float)cnt);
  }
}

// GlobalAveragePooling2D: y[b, k] = sum_p x[b, p, k] / hw (fp32, pixels in order)
template <typename T>
__global__ void __launch_bounds__(kB)
global_avg_pool_kernel(const T* __restrict__ x, int n, int hw, int c, float* __restrict__ y) {
  const int64_t total = (int64_t)n * c;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kB) {
    const int k = (int)(i % c);
    const int64_t b = i / c;
    const T* base = x + b * hw * c + k;
    float s = 0.f;
    for (int p = 0; p < hw; ++p) s += VT<T>::ld1(base + (int64_t)p * c);
    y[i] = s / (float)hw;
  }
}

// tf.nn.softmax over rows: one wave per row, exp(x - max) / sum
template <typename T>
__global__ void __launch_bounds__(kB)
softmax_rows_kernel(const T* __restrict__ x, int64_t rows, int c, float* __restrict__ y) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = (int64_t)gridDim.x * (kB / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kB / kWave) + threadIdx.x / kWave; r < rows; r += waves) {
    const T* xr = x + r * c;
    float m = -INFINITY;
    for (int j = lane; j < c; j += kWave) {
      const float v = VT<T>::ld1(xr + j);
      m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float t = __shfl_xor(m, o, kWave);
      m = t > m ? t : m;
    }
    float s = 0.f;
    for (int j = lane; j < c; j += kWave) s += expf(VT<T>::ld1(xr + j) - m);
    s = wave_sum(s);
    const float inv = 1.f / s;
    for (int j = lane; j < c; j += kWave) y[r * c + j] = expf(VT<T>::ld1(xr + j) - m) * inv;
  }
}

// ------------------------------------------------------------------------------ feature moments
// sum[j] += sum_b x[b, j], gram[i][j] += sum_b x[b, i] x[b, j], *count += rows, in binary64.
// One 256-thread workgroup per 64 x 64 tile (ti <= tj: the upper-triangle tiles; the strictly
// lower tiles of `gram` are never touched).  Thread (ty, tx) owns the 16 elements
// (ti*64 + ty + 16 r, tj*64 + tx + 16 s) and walks the rows in order with fma(): no atomics and
// a fixed reduction order, so the result is bit-reproducible.  The fp32 products are exact in
// binary64; only the running sums round.
constexpr int kMT = 64, kMRows = 32;

__global__ void __launch_bounds__(kB)
moments_kernel(const float* __restrict__ x, int64_t rows, int c, int ntile,
               int64_t* __restrict__ count, double* __restrict__ sum, double* __restrict__ gram) {
  __shared__ double si[kMRows][kMT];
  __shared__ double sj[kMRows][kMT];
  int ti = 0, t = blockIdx.x;
  while (t >= ntile - ti) { t -= ntile - ti; ++ti; }
  const int tj = ti + t;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const bool diag = ti == tj;
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.0;
  double cs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t b0 = 0; b0 < rows; b0 += kMRows) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kMRows * kMT / kB; ++e) {
      const int idx = e * kB + threadIdx.x;
      const int rr = idx / kMT, cc = idx % kMT;
      const int64_t b = b0 + rr;
      const int ci = ti * kMT + cc, cj = tj * kMT + cc;
      si[rr][cc] = (b < rows && ci < c) ? (double)x[b * c + ci] : 0.0;
      sj[rr][cc] = (b < rows && cj < c) ? (double)x[b * c + cj] : 0.0;
    }
    __syncthreads();
    const int nr = rows - b0 < kMRows ? (int)(rows - b0) : kMRows;
    for (int rr = 0; rr < nr; ++rr) {
      double a[4], v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = si[rr][ty + 16 * r];
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] = sj[rr][tx + 16 * s];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = fma(a[r], v[s], acc[r][s]);
      if (diag && ty == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) cs[s] += v[s];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ti * kMT + ty + 16 * r;
    if (i >= c) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = tj * kMT + tx + 16 * s;
      if (j < c) gram[(int64_t)i * c + j] += acc[r][s];
    }
  }
  if (diag && ty == 0) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = tj * kMT + tx + 16 * s;
      if (j < c) sum[j] += cs[s];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *count += rows;
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" {

int se3ds_inception_preprocess(const float* frames, int n, int h, int w, const int32_t* roll_flip,
                               int crop_rows, int oh, int ow, void* out, int out_dtype,
                               void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || crop_rows < 0 || h - 2 * crop_rows <= 0)
    return SE3DS_E_BADSHAPE;
  hipStream_t s = as_stream(stream);
  const dim3 g((unsigned)grid_for((int64_t)n * oh * ow * 3, kB));
  if (out_dtype == SE3DS_F32)
    hipLaunchKernelGGL(preprocess_kernel<float>, g, dim3(kB), 0, s, frames, n, h, w, roll_flip,
                       crop_rows, oh, ow, (float*)out);
  else if (out_dtype == SE3DS_BF16)
    hipLaunchKernelGGL(preprocess_kernel<uint16_t>, g, dim3(kB), 0, s, frames, n, h, w, roll_flip,
                       crop_rows, oh, ow, (uint16_t*)out);
  else
    return SE3DS_E_BADDTYPE;
  return check_launch("inception_preprocess");
}

int se3ds_inception_maxpool3s2(const void* x, int dtype, int n, int h, int w, int c, void* y,
                               int y_c, int y_c0, void* stream) {
  if (n <= 0 || h < 3 || w < 3 || c <= 0 || y_c0 < 0 || y_c0 + c > y_c) return SE3DS_E_BADSHAPE;
  const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
  hipStream_t s = as_stream(stream);
  const dim3 g((unsigned)grid_for((int64_t)n * oh * ow * c, kB));
  if (dtype == SE3DS_F32)
    hipLaunchKernelGGL(maxpool3s2_kernel<float>, g, dim3(kB), 0, s, (const float*)x, n, h, w, c,
                       oh, ow, (float*)y, y_c, y_c0);
  else if (dtype == SE3DS_BF16)
    hipLaunchKernelGGL(maxpool3s2_kernel<uint16_t>, g, dim3(kB), 0, s, (const uint16_t*)x, n, h,
                       w, c, oh, ow, (uint16_t*)y, y_c, y_c0);
  else
    return SE3DS_E_BADDTYPE;
  return check_launch("inception_maxpool3s2");
}

int se3ds_inception_avgpool3s1(const void* x, int dtype, int n, int h, int w, int c, void* y,
                               int y_c, int y_c0, void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || y_c0 < 0 || y_c0 + c > y_c) return SE3DS_E_BADSHAPE;
  hipStream_t s = as_stream(stream);
  const dim3 g((unsigned)grid_for((int64_t)n * h * w * c, kB));
  if (dtype == SE3DS_F32)
    hipLaunchKernelGGL(avgpool3s1_kernel<float>, g, dim3(kB), 0, s, (const float*)x, n, h, w, c,
                       (float*)y, y_c, y_c0);
  else if (dtype == SE3DS_BF16)
    hipLaunchKernelGGL(avgpool3s1_kernel<uint16_t>, g, dim3(kB), 0, s, (const uint16_t*)x, n, h,
                       w, c, (uint16_t*)y, y_c, y_c0);
  else
    return SE3DS_E_BADDTYPE;
  return check_launch("inception_avgpool3s1");
}

int se3ds_global_avg_pool(const void* x, int dtype, int n, int hw, int c, float* y, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0) return SE3DS_E_BADSHAPE;
  hipStream_t s = as_stream(stream);
  const dim3 g((unsigned)grid_for((int64_t)n * c, kB));
  if (dtype == SE3DS_F32)
    hipLaunchKernelGGL(global_avg_pool_kernel<float>, g, dim3(kB), 0, s, (const float*)x, n, hw, c,
                       y);
  else if (dtype == SE3DS_BF16)
    hipLaunchKernelGGL(global_avg_pool_kernel<uint16_t>, g, dim3(kB), 0, s, (const uint16_t*)x, n,
                       hw, c, y);
  else
    return SE3DS_E_BADDTYPE;
  return check_launch("global_avg_pool");
}

int se3ds_softmax_rows(const void* x, int dtype, int64_t rows, int c, float* y, void* stream) {
  if (rows <= 0 || c <= 0) return SE3DS_E_BADSHAPE;
  hipStream_t s = as_stream(stream);
  const dim3 g((unsigned)grid_for(rows * kWave, kB));
  if (dtype == SE3DS_F32)
    hipLaunchKernelGGL(softmax_rows_kernel<float>, g, dim3(kB), 0, s, (const float*)x, rows, c, y);
  else if (dtype == SE3DS_BF16)
    hipLaunchKernelGGL(softmax_rows_kernel<uint16_t>, g, dim3(kB), 0, s, (const uint16_t*)x, rows,
                       c, y);
  else
    return SE3DS_E_BADDTYPE;
  return check_launch("softmax_rows");
}

int se3ds_feature_moments_accumulate(const float* x, int64_t rows, int c, int64_t* count,
                                     double* sum, double* gram, void* stream) {
  if (rows < 0 || c <= 0) return SE3DS_E_BADSHAPE;
  if (rows == 0) return SE3DS_OK;
  const int ntile = (int)ceil_div(c, kMT);
  const int64_t tiles = (int64_t)ntile * (ntile + 1) / 2;
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)tiles), dim3(kB), 0, as_stream(stream), x, rows,
                     c, ntile, count, sum, gram);
  return check_launch("feature_moments_accumulate");
}

}  // extern "C"
