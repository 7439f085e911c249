// Paired image metrics (utils/image_metrics.py): SSIM / MS-SSIM as tf.image.ssim defines them, the
// squared-difference sum behind PSNR, and the 2 x 2 mean between MS-SSIM scales.  Everything after a
// load is binary64; the file is built with -ffp-contract=off, so every product and every sum below
// rounds as written.
//
// SSIM.  ssim_tile_kernel: a workgroup of 256 threads owns a kTileRows x kTileCols tile of the
// (h - fs + 1) x (w - fs + 1) map, all channels.
//   * stage: the (kTileRows + fs - 1) x (kTileCols + fs - 1) x c pixels of a and b under the tile go
//     to LDS once, as fp32 (uint8 widens exactly), one plane per image and channel; what lies outside
//     the image is 0 and only feeds map positions that do not exist.
//   Then, one channel at a time (so that the row sums of one channel are all the LDS they take):
//   * horizontal pass: thread (ty, tx) takes column tx of rows ty, ty + 16, ... and forms the four
//     window sums G_h(a), G_h(b), G_h(a b), G_h(a a + b b) -- taps ascending, the first tap a
//     product, every later one a product and an add -- into four binary64 planes in LDS.
//   * vertical pass: thread (ty, tx) is map position (ty, tx) of the tile: the four sums over rows
//     ty .. ty + fs - 1 of its column, then lum, cs, lum * cs.
//   * lum * cs and cs of the 256 positions: butterfly per wave, one pair per wave and channel in LDS.
//   At the end the four waves' values are added in index order into one 8-slot record per workgroup
//   (ssim sums of channels 0..3, cs sums of channels 0..3) in the workspace.
// No filtered plane reaches HBM.  ssim_reduce_kernel adds an image's records in a fixed order and
// divides by the map size.  No atomics: the same input gives the same bits on every run.
//
// LDS per workgroup: 8 c (15 + fs)^2 bytes of staged pixels + 512 (15 + fs) bytes of row sums
// (c = 3, fs = 11: 16 224 + 13 312 = 29 536 bytes, five workgroups in the 160 KB of a CU; c = 4,
// fs = 15: 28 800 + 15 360 = 44 160 bytes, three).
//
// All device stores are plain C++ vector stores.
#include "common.h"

namespace se3ds {
namespace {

constexpr int kTileRows = 16;
constexpr int kTileCols = 16;
constexpr int kSsimThreads = kTileRows * kTileCols;
constexpr int kSsimWaves = kSsimThreads / kWave;
constexpr int kMaxTaps = 15;
constexpr int kMaxChannels = 4;
constexpr int kSlots = 2 * kMaxChannels;   // a workgroup's record: ssim sums [4], cs sums [4]
constexpr int kMaxSide = 32768;
constexpr int kMaxImages = 65535;

struct Taps {
  float w[kMaxTaps];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

template <class T>
__global__ void __launch_bounds__(kSsimThreads)
ssim_tile_kernel(const T* __restrict__ a, const T* __restrict__ b, int h, int w, int c, int fs, Taps taps,
                 double c1, double c2, double* __restrict__ partial, double* __restrict__ map) {
  extern __shared__ double lds[];
  __shared__ double wl[kMaxTaps + 1];
  __shared__ double part[kSlots][kSsimWaves];
  const int in_rows = kTileRows + fs - 1, in_cols = kTileCols + fs - 1;
  const int plane_in = in_rows * in_cols, plane_h = in_rows * kTileCols;
  double* hsum = lds;                                                    // [4][in_rows][kTileCols]: one channel
  float* in = reinterpret_cast<float*>(lds + 4 * plane_h);               // [2][c][in_rows][in_cols]
  const int tid = (int)threadIdx.x;
  const int y0 = (int)blockIdx.y * kTileRows, x0 = (int)blockIdx.x * kTileCols;
  const int img = (int)blockIdx.z;
  const int oh = h - fs + 1, ow = w - fs + 1;
  if (tid < fs) wl[tid] = (double)taps.w[tid];
  if (tid < kSlots * kSsimWaves) part[tid / kSsimWaves][tid % kSsimWaves] = 0.0;   // channels >= c stay 0

  // stage: a tile row is in_cols * c adjacent elements of the image row; a wave takes rows wave,
  // wave + 4, ...  k / c for k < 2^15 and c <= 4 is (k * (2^16 / c + 1)) >> 16.
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int row_elems = in_cols * c;
  const uint32_t recip = 65536u / (uint32_t)c + 1u;
  const int64_t img_base = (int64_t)img * h * w * c;
  for (int row = wave; row < in_rows; row += kSsimWaves) {
    const int gy = y0 + row;
    const int64_t row_base = img_base + ((int64_t)gy * w + x0) * c;
    for (int k = lane; k < row_elems; k += kWave) {
      const int x = (int)(((uint32_t)k * recip) >> 16), ch = k - x * c;
      float va = 0.0f, vb = 0.0f;
      if (gy < h && x0 + x < w) {
        va = (float)a[row_base + k];
        vb = (float)b[row_base + k];
      }
      const int o = (ch * in_rows + row) * in_cols + x;
      in[o] = va;
      in[c * plane_in + o] = vb;
    }
  }
  __syncthreads();

  const int tx = tid & (kTileCols - 1), ty = tid / kTileCols;
  const int oy = y0 + ty, ox = x0 + tx;
  const bool valid = oy < oh && ox < ow;
  for (int ch = 0; ch < c; ++ch) {
    for (int row = ty; row < in_rows; row += kTileRows) {
      const float* pa = in + (ch * in_rows + row) * in_cols + tx;
      const float* pb = pa + c * plane_in;
      double av = (double)pa[0], bv = (double)pb[0], wt = wl[0];
      double m0 = wt * av, m1 = wt * bv, sab = wt * (av * bv), ssq = wt * (av * av + bv * bv);
      for (int t = 1; t < fs; ++t) {
        av = (double)pa[t];
        bv = (double)pb[t];
        wt = wl[t];
        m0 = m0 + wt * av;
        m1 = m1 + wt * bv;
        sab = sab + wt * (av * bv);
        ssq = ssq + wt * (av * av + bv * bv);
      }
      const int o = row * kTileCols + tx;
      hsum[o] = m0;
      hsum[plane_h + o] = m1;
      hsum[2 * plane_h + o] = sab;
      hsum[3 * plane_h + o] = ssq;
    }
    __syncthreads();
    const double* p = hsum + ty * kTileCols + tx;
    double wt = wl[0];
    double m0 = wt * p[0], m1 = wt * p[plane_h], sab = wt * p[2 * plane_h], ssq = wt * p[3 * plane_h];
    for (int t = 1; t < fs; ++t) {
      const double* q = p + t * kTileCols;
      wt = wl[t];
      m0 = m0 + wt * q[0];
      m1 = m1 + wt * q[plane_h];
      sab = sab + wt * q[2 * plane_h];
      ssq = ssq + wt * q[3 * plane_h];
    }
    const double n0 = 2.0 * m0 * m1, d0 = m0 * m0 + m1 * m1;
    const double lum = (n0 + c1) / (d0 + c1);
    const double n1 = 2.0 * sab;
    const double cs = (n1 - n0 + c2) / (ssq - d0 + c2);
    const double index = lum * cs;
    if (valid && map) map[(((int64_t)img * oh + oy) * ow + ox) * c + ch] = index;
    const double s = wave_sum_f64(valid ? index : 0.0), q = wave_sum_f64(valid ? cs : 0.0);
    if (lane == 0) {
      part[ch][wave] = s;
      part[kMaxChannels + ch][wave] = q;
    }
    __syncthreads();   // the next channel's row sums overwrite hsum
  }
  if (tid < kSlots) {
    double s = part[tid][0];
#pragma unroll
    for (int k = 1; k < kSsimWaves; ++k) s += part[tid][k];
    const int64_t block = ((int64_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[block * kSlots + tid] = s;
  }
}

constexpr int kReduceThreads = 256;
constexpr int kReduceGroups = kReduceThreads / kSlots;

// thread (group g, slot s) adds slot s of records g, g + 32, ... in order; thread s then adds the 32
// groups in order and divides by the map size
__global__ void __launch_bounds__(kReduceThreads)
ssim_reduce_kernel(const double* __restrict__ partial, int tiles, int c, double count,
                   double* __restrict__ ssim_mean, double* __restrict__ cs_mean) {
  __shared__ double red[kReduceGroups][kSlots];
  const int tid = (int)threadIdx.x, slot = tid & (kSlots - 1), group = tid / kSlots;
  const double* p = partial + (int64_t)blockIdx.x * tiles * kSlots;
  double s = 0.0;
  for (int t = group; t < tiles; t += kReduceGroups) s += p[(int64_t)t * kSlots + slot];
  red[group][slot] = s;
  __syncthreads();
  if (tid < kSlots) {
    double total = red[0][tid];
    for (int g = 1; g < kReduceGroups; ++g) total += red[g][tid];
    const int ch = tid & (kMaxChannels - 1);
    if (ch < c) (tid < kMaxChannels ? ssim_mean : cs_mean)[(int64_t)blockIdx.x * c + ch] = total / count;
  }
}

// ---------------------------------------------------------------------------------------------
// squared differences

constexpr int kSumThreads = 256;
constexpr int kSumWaves = kSumThreads / kWave;
constexpr int kSumChunk = 8192;   // elements of one image per workgroup

__device__ __forceinline__ void block_sum(double v, double* out) {
  __shared__ double part[kSumWaves];
  v = wave_sum_f64(v);
  if (((int)threadIdx.x & (kWave - 1)) == 0) part[(int)threadIdx.x / kWave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = part[0];
#pragma unroll
    for (int k = 1; k < kSumWaves; ++k) s += part[k];
    *out = s;
  }
}

__device__ __forceinline__ bool aligned16(const void* p, const void* q) {
  return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15u) == 0;
}

// uint8: a thread sees 32 elements of a chunk, at most 32 * 255^2 < 2^32: an exact integer
__global__ void __launch_bounds__(kSumThreads)
sqdiff_partial_u8_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t elems, int parts,
                         double* __restrict__ partial) {
  const int64_t image = (int64_t)blockIdx.x / parts;
  const int64_t e0 = ((int64_t)blockIdx.x - image * parts) * kSumChunk;
  const int len = (int)(elems - e0 < kSumChunk ? elems - e0 : kSumChunk);
  const uint8_t* p = a + image * elems + e0;
  const uint8_t* q = b + image * elems + e0;
  const int tid = (int)threadIdx.x;
  uint32_t sum = 0;
  const int nvec = aligned16(p, q) ? len / 16 : 0;
  const uint4* pv = reinterpret_cast<const uint4*>(p);
  const uint4* qv = reinterpret_cast<const uint4*>(q);
  for (int v = tid; v < nvec; v += kSumThreads) {
    const uint4 x = pv[v], y = qv[v];
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int d = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu) - (int)((yw[j >> 2] >> (8 * (j & 3))) & 0xffu);
      sum += (uint32_t)(d * d);
    }
  }
  for (int i = 16 * nvec + tid; i < len; i += kSumThreads) {
    const int d = (int)p[i] - (int)q[i];
    sum += (uint32_t)(d * d);
  }
  block_sum((double)sum, partial + blockIdx.x);
}

__global__ void __launch_bounds__(kSumThreads)
sqdiff_partial_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t elems, int parts,
                          double* __restrict__ partial) {
  const int64_t image = (int64_t)blockIdx.x / parts;
  const int64_t e0 = ((int64_t)blockIdx.x - image * parts) * kSumChunk;
  const int len = (int)(elems - e0 < kSumChunk ? elems - e0 : kSumChunk);
  const float* p = a + image * elems + e0;
  const float* q = b + image * elems + e0;
  const int tid = (int)threadIdx.x;
  double sum = 0.0;
  const int nvec = aligned16(p, q) ? len / 4 : 0;
  const float4* pv = reinterpret_cast<const float4*>(p);
  const float4* qv = reinterpret_cast<const float4*>(q);
  for (int v = tid; v < nvec; v += kSumThreads) {
    const float4 x = pv[v], y = qv[v];
    const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y;
    const double d2 = (double)x.z - (double)y.z, d3 = (double)x.w - (double)y.w;
    sum += d0 * d0;
    sum += d1 * d1;
    sum += d2 * d2;
    sum += d3 * d3;
  }
  for (int i = 4 * nvec + tid; i < len; i += kSumThreads) {
    const double d = (double)p[i] - (double)q[i];
    sum += d * d;
  }
  block_sum(sum, partial + blockIdx.x);
}

// out[image] = the image's partial sums: thread k takes parts k, k + 256, ... in order, then the block sum
__global__ void __launch_bounds__(kSumThreads)
sqdiff_reduce_kernel(const double* __restrict__ partial, int parts, double* __restrict__ out) {
  const double* p = partial + (int64_t)blockIdx.x * parts;
  double s = 0.0;
  for (int k = (int)threadIdx.x; k < parts; k += kSumThreads) s += p[k];
  block_sum(s, out + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// 2 x 2 mean

constexpr int kDownThreads = 256;

template <class T>
__global__ void __launch_bounds__(kDownThreads)
downsample2_kernel(const T* __restrict__ x, int h, int w, int c, int oh, int ow, int64_t total,
                   float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kDownThreads;
  for (int64_t i = (int64_t)blockIdx.x * kDownThreads + threadIdx.x; i < total; i += stride) {
    const int64_t px = i / c;
    const int ch = (int)(i - px * c);
    const int64_t row = px / ow;
    const int ox = (int)(px - row * ow);
    const int64_t image = row / oh;
    const int oy = (int)(row - image * oh);
    const int ya = 2 * oy, yb = 2 * oy + 1 < h ? 2 * oy + 1 : h - 1;   // an odd side repeats its last line
    const int xa = 2 * ox, xb = 2 * ox + 1 < w ? 2 * ox + 1 : w - 1;
    const T* base = x + image * h * w * c + ch;
    const double x00 = (double)base[((int64_t)ya * w + xa) * c], x01 = (double)base[((int64_t)ya * w + xb) * c];
    const double x10 = (double)base[((int64_t)yb * w + xa) * c], x11 = (double)base[((int64_t)yb * w + xb) * c];
    out[i] = (float)((((x00 + x01) + x10) + x11) * 0.25);
  }
}

// ---------------------------------------------------------------------------------------------
// host side

bool ssim_shape_ok(int n, int h, int w, int c, int fs) {
  return n >= 1 && n <= kMaxImages && c >= 1 && c <= kMaxChannels && fs >= 1 && fs <= kMaxTaps && h >= fs &&
         w >= fs && h <= kMaxSide && w <= kMaxSide;
}

int64_t ssim_tiles(int h, int w, int fs) {
  return ceil_div(h - fs + 1, kTileRows) * ceil_div(w - fs + 1, kTileCols);
}

size_t ssim_workspace_bytes(int n, int h, int w, int fs) {
  return (size_t)n * (size_t)ssim_tiles(h, w, fs) * kSlots * sizeof(double);
}

constexpr size_t ssim_lds_bytes(int c, int fs) {
  const size_t in_rows = kTileRows + fs - 1, in_cols = kTileCols + fs - 1;
  return 4 * in_rows * kTileCols * sizeof(double) + 2 * c * in_rows * in_cols * sizeof(float);
}

template <class T>
int launch_ssim(const void* a, const void* b, int n, int h, int w, int c, int fs, const Taps& taps, double c1,
                double c2, double* partial, double* map, hipStream_t st) {
  static_assert(ssim_lds_bytes(kMaxChannels, kMaxTaps) <= 48 * 1024, "within the default dynamic LDS limit");
  const size_t lds = ssim_lds_bytes(c, fs);
  const dim3 grid((unsigned)ceil_div(w - fs + 1, kTileCols), (unsigned)ceil_div(h - fs + 1, kTileRows), (unsigned)n);
  hipLaunchKernelGGL(ssim_tile_kernel<T>, grid, dim3(kSsimThreads), lds, st, static_cast<const T*>(a),
                     static_cast<const T*>(b), h, w, c, fs, taps, c1, c2, partial, map);
  return check_launch("ssim tiles");
}

bool sums_shape_ok(int n, int64_t elems) {
  return n >= 1 && n <= kMaxImages && elems >= 1 && elems <= ((int64_t)1 << 40) &&
         (int64_t)n * ceil_div(elems, kSumChunk) <= INT32_MAX;
}

unsigned elem_mask(int dtype) { return dtype == SE3DS_F32 ? 3u : 0u; }

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_ssim_tile_rows(void) { return kTileRows; }
extern "C" int se3ds_ssim_tile_cols(void) { return kTileCols; }

extern "C" size_t se3ds_ssim_workspace_bytes(int n, int h, int w, int c, int filter_size) {
  return ssim_shape_ok(n, h, w, c, filter_size) ? ssim_workspace_bytes(n, h, w, filter_size) : 0;
}

extern "C" int se3ds_ssim(const void* a, const void* b, int dtype, int n, int h, int w, int c, const float* weights,
                          int filter_size, double max_val, double k1, double k2, double* ssim_mean,
                          double* cs_mean, double* map, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ssim_shape_ok(n, h, w, c, filter_size) || !(max_val > 0.0)) return SE3DS_E_BADSHAPE;
  if (dtype != SE3DS_F32 && dtype != SE3DS_U8) return SE3DS_E_BADDTYPE;
  if (!a || !b || !weights || !ssim_mean || !cs_mean || !workspace) return SE3DS_E_BADSHAPE;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & elem_mask(dtype)) != 0 ||
      ((reinterpret_cast<uintptr_t>(ssim_mean) | reinterpret_cast<uintptr_t>(cs_mean) |
        reinterpret_cast<uintptr_t>(map) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
    return SE3DS_E_BADSHAPE;
  if (workspace_bytes < ssim_workspace_bytes(n, h, w, filter_size)) return SE3DS_E_WORKSPACE;
  Taps taps = {};
  for (int t = 0; t < filter_size; ++t) taps.w[t] = weights[t];
  const double l1 = k1 * max_val, l2 = k2 * max_val;
  const double c1 = l1 * l1, c2 = l2 * l2;
  double* partial = static_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  const int rc = dtype == SE3DS_F32
                     ? launch_ssim<float>(a, b, n, h, w, c, filter_size, taps, c1, c2, partial, map, st)
                     : launch_ssim<uint8_t>(a, b, n, h, w, c, filter_size, taps, c1, c2, partial, map, st);
  if (rc != SE3DS_OK) return rc;
  const double count = (double)((int64_t)(h - filter_size + 1) * (w - filter_size + 1));
  hipLaunchKernelGGL(ssim_reduce_kernel, dim3((unsigned)n), dim3(kReduceThreads), 0, st, partial,
                     (int)ssim_tiles(h, w, filter_size), c, count, ssim_mean, cs_mean);
  return check_launch("ssim reduce");
}

extern "C" int se3ds_sqdiff_chunk(void) { return kSumChunk; }

extern "C" size_t se3ds_sqdiff_workspace_bytes(int n, int64_t elems_per_image) {
  return sums_shape_ok(n, elems_per_image) ? (size_t)n * (size_t)ceil_div(elems_per_image, kSumChunk) * sizeof(double)
                                           : 0;
}

extern "C" int se3ds_sqdiff_sum(const void* a, const void* b, int dtype, int n, int64_t elems_per_image,
                                double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sums_shape_ok(n, elems_per_image)) return SE3DS_E_BADSHAPE;
  if (dtype != SE3DS_F32 && dtype != SE3DS_U8) return SE3DS_E_BADDTYPE;
  if (!a || !b || !out || !workspace) return SE3DS_E_BADSHAPE;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & elem_mask(dtype)) != 0 ||
      ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
    return SE3DS_E_BADSHAPE;
  const int parts = (int)ceil_div(elems_per_image, kSumChunk);
  if (workspace_bytes < (size_t)n * (size_t)parts * sizeof(double)) return SE3DS_E_WORKSPACE;
  double* partial = static_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(n * parts)), block(kSumThreads);
  if (dtype == SE3DS_F32)
    hipLaunchKernelGGL(sqdiff_partial_f32_kernel, grid, block, 0, st, static_cast<const float*>(a),
                       static_cast<const float*>(b), elems_per_image, parts, partial);
  else
    hipLaunchKernelGGL(sqdiff_partial_u8_kernel, grid, block, 0, st, static_cast<const uint8_t*>(a),
                       static_cast<const uint8_t*>(b), elems_per_image, parts, partial);
  const int rc = check_launch("sqdiff_sum");
  if (rc != SE3DS_OK) return rc;
  hipLaunchKernelGGL(sqdiff_reduce_kernel, dim3((unsigned)n), block, 0, st, partial, parts, out);
  return check_launch("sqdiff_sum reduce");
}

extern "C" int se3ds_downsample2_sym(const void* x, int dtype, int n, int h, int w, int c, float* out,
                                     void* stream) {
  if (n < 1 || n > kMaxImages || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide || c < 1 || c > kMaxChannels)
    return SE3DS_E_BADSHAPE;
  if (dtype != SE3DS_F32 && dtype != SE3DS_U8) return SE3DS_E_BADDTYPE;
  if (!x || !out || (reinterpret_cast<uintptr_t>(x) & elem_mask(dtype)) != 0 ||
      (reinterpret_cast<uintptr_t>(out) & 3u) != 0)
    return SE3DS_E_BADSHAPE;
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  const int64_t total = (int64_t)n * oh * ow * c;
  const dim3 grid((unsigned)grid_for(total, kDownThreads)), block(kDownThreads);
  if (dtype == SE3DS_F32)
    hipLaunchKernelGGL(downsample2_kernel<float>, grid, block, 0, as_stream(stream), static_cast<const float*>(x), h,
                       w, c, oh, ow, total, out);
  else
    hipLaunchKernelGGL(downsample2_kernel<uint8_t>, grid, block, 0, as_stream(stream),
                       static_cast<const uint8_t*>(x), h, w, c, oh, ow, total, out);
  return check_launch("downsample2_sym");
}
