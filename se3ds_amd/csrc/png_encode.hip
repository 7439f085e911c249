// PNG encoding on the device: image sheets for the TensorBoard summaries (utils/image_grid.py,
// utils/logger.py of the reference; trainers/gan_manager.py:404-420,571-617) and the roll-out PNGs of
// GANManager.test.  Two entry points: se3ds_grid_quantize composes a batch of float images into one
// uint8 sheet (tf.cast(x * 255.0, tf.uint8) + images_to_grid, utils/image_grid.py:24-51), and
// se3ds_png_encode turns many uint8 images into zlib streams -- filtering and deflate.  The encoder
// is deflate_core.h; this file is its 64-lane policy, the two kernels and the entry points.
// se3ds_png_encode_planes is the same pair of launches for the planes of a training record
// (datasets/record_writer.py), whose table may also name 16-bit grey planes (field 3 = 2).
//
// Schedule: an image is cut into strips of max(1, 65535 / (1 + row_bytes)) rows; one wavefront (one
// 64-thread workgroup) per strip, grid = the strips of all images.  A strip reads the row above its
// first row from the source image, so strips do not depend on each other, and writes its blocks
// into a slot of its own in the workspace (at most 10 bytes more than its filtered bytes: the
// stored-block fallback bounds it).  A second launch, one workgroup per strip again, sums the
// lengths of the strips in front of its own within the image, copies the slot to its place in the
// compact output and -- the image's last strip -- folds the strips' Adler-32 sums into the image's
// and writes the size.  Both launches go to the caller's stream; nothing synchronises.
//
// LDS: the strip's filtered bytes (64 KiB) + the code construction's tables (7 KiB) = 72 736 B
// static, two workgroups per CU, as the inflater.  No scratch.  No atomics anywhere: every output
// byte has one writer and the sums are folded in a fixed order, so the output is the same bytes on
// every run.
#include "common.h"
#include "deflate_core.h"

namespace se3ds {
namespace {

constexpr int kEncodeFields = 8;        // int64 per descriptor row
constexpr int kEncodeMaxRowBytes = 32768;
constexpr int kMetaWords = 4;           // uint32 per strip: length, Adler s1, s2, filtered bytes
constexpr int kCompactThreads = 256;

struct WavePolicy {
  static constexpr int kLanes = kWave;
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ void sync() const { __syncthreads(); }
  __device__ uint32_t sum(uint32_t v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, kWave);
    return v;
  }
  __device__ uint32_t min(uint32_t v) const { return wave_min_u32(v); }
};

// What both kernels and the host-side check derive from a descriptor row.
struct Geometry {
  int64_t strips, rows_per_strip, slot_bytes, out_bytes;
};

__host__ __device__ inline Geometry geometry(int64_t height, int64_t row_bytes) {
  Geometry g;
  g.rows_per_strip = (int64_t)deflate::strip_rows((uint32_t)row_bytes);
  g.strips = (height + g.rows_per_strip - 1) / g.rows_per_strip;
  const int64_t slot_rows = height < g.rows_per_strip ? height : g.rows_per_strip;
  g.slot_bytes = ((int64_t)deflate::kStripOverhead + slot_rows * (1 + row_bytes) + 7) & ~(int64_t)7;
  g.out_bytes = g.strips * (int64_t)deflate::kStripOverhead + height * (1 + row_bytes);
  return g;
}

__host__ __device__ inline int64_t meta_bytes(int64_t total_strips) {
  return (total_strips * kMetaWords * (int64_t)sizeof(uint32_t) + 15) & ~(int64_t)15;
}

// the image whose strips include `strip`: the last row with first_strip (field 5) <= strip
__device__ inline int image_of(const int64_t* __restrict__ table, int n, int64_t strip) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(int64_t)mid * kEncodeFields + 5] <= strip) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kWave)
png_encode_kernel(const int64_t* __restrict__ table, int n, int64_t total_strips,
                  uint8_t* __restrict__ workspace) {
  __shared__ deflate::Shared shared;
  const int64_t strip = (int64_t)blockIdx.x;
  const int64_t* d = table + (int64_t)image_of(table, n, strip) * kEncodeFields;
  const uint8_t* image = reinterpret_cast<const uint8_t*>(d[0]);
  const int64_t height = d[1], row_bytes = d[2];
  const Geometry g = geometry(height, row_bytes);
  const int64_t k = strip - d[5];
  const int64_t row0 = k * g.rows_per_strip;
  const int64_t rows = height - row0 < g.rows_per_strip ? height - row0 : g.rows_per_strip;
  uint8_t* slot = workspace + meta_bytes(total_strips) + d[7] + k * g.slot_bytes;
  const WavePolicy policy;
  deflate::Encoder<WavePolicy> encoder(policy, shared, slot);
  // field 3 = 2 (se3ds_png_encode_planes only): 16-bit samples in host order
  const uint32_t bytes = encoder.filter(image, (uint32_t)row_bytes, (uint32_t)d[3], (uint32_t)d[4],
                                        (uint32_t)row0, (uint32_t)rows, d[3] == 2);
  const uint32_t length = encoder.compress(bytes, k == g.strips - 1);
  if (threadIdx.x == 0) {
    uint32_t* meta = reinterpret_cast<uint32_t*>(workspace) + strip * kMetaWords;
    meta[0] = length;
    meta[1] = encoder.s1();
    meta[2] = encoder.s2();
    meta[3] = bytes;
  }
}

__global__ void __launch_bounds__(kCompactThreads)
png_compact_kernel(const int64_t* __restrict__ table, int n, int64_t total_strips,
                   const uint8_t* __restrict__ workspace, uint8_t* __restrict__ out,
                   uint32_t* __restrict__ sizes) {
  __shared__ uint32_t partial[kCompactThreads / kWave];
  const int64_t strip = (int64_t)blockIdx.x;
  const int img = image_of(table, n, strip);
  const int64_t* d = table + (int64_t)img * kEncodeFields;
  const Geometry g = geometry(d[1], d[2]);
  const int64_t k = strip - d[5];
  const uint32_t* meta = reinterpret_cast<const uint32_t*>(workspace) + d[5] * kMetaWords;
  // bytes of the image's strips in front of this one (< 2^32: an image's bound is checked on the host)
  uint32_t before = 0;
  for (int64_t j = threadIdx.x; j < k; j += kCompactThreads) before += meta[j * kMetaWords];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += (uint32_t)__shfl_xor((int)before, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) partial[threadIdx.x / kWave] = before;
  __syncthreads();
  before = 0;
  for (int w = 0; w < kCompactThreads / kWave; ++w) before += partial[w];
  const uint32_t length = meta[k * kMetaWords];
  const uint8_t* slot = workspace + meta_bytes(total_strips) + d[7] + k * g.slot_bytes;
  uint8_t* dst = out + d[6] + before;
  for (uint32_t i = threadIdx.x; i < length; i += kCompactThreads) dst[i] = slot[i];
  if (k == g.strips - 1 && threadIdx.x == 0) {
    uint32_t s1 = 1, s2 = 0;
    for (int64_t j = 0; j < g.strips; ++j)
      deflate::adler_combine(s1, s2, meta[j * kMetaWords + 1], meta[j * kMetaWords + 2],
                             meta[j * kMetaWords + 3], &s1, &s2);
    sizes[2 * img] = before + length;
    sizes[2 * img + 1] = (s2 << 16) | s1;
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
grid_quantize_kernel(const T* __restrict__ src, int h, int w, int c, int nx, int out_c,
                     int64_t total, uint8_t* __restrict__ out) {
  const int64_t sheet_w = (int64_t)nx * w;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % out_c);
    const int64_t px = i / out_c;
    const int64_t X = px % sheet_w, Y = px / sheet_w;
    const int64_t tile = (Y / h) * nx + X / w;
    const int64_t at = ((tile * h + Y % h) * w + X % w) * c + (c == 1 ? 0 : ch);
    // tf.cast(x * 255.0, tf.uint8): one fp32 product, truncated toward zero; out of range saturates,
    // NaN -> 0
    const float v = VT<T>::ld1(src + at) * 255.0f;
    out[i] = !(v > 0.0f) ? (uint8_t)0 : v >= 255.0f ? (uint8_t)255 : (uint8_t)(int)v;
  }
}

// The host copy of the table: every row's own fields, and the cumulative ones against what this
// file derives.  Fills the totals.  planes: the table of se3ds_png_encode_planes, whose field 3 may
// also be 2.
int check_table(const int64_t* host_table, int n, bool planes, int64_t* total_strips,
                int64_t* slots_bytes, int64_t* out_bytes) {
  if (n < 1 || n > 65535 || !host_table) return SE3DS_E_BADSHAPE;
  int64_t strips = 0, slots = 0, outs = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = host_table + (int64_t)i * kEncodeFields;
    const int64_t height = d[1], row_bytes = d[2], bpp = d[3], mode = d[4];
    if (d[0] == 0 || height < 1 || height > INT32_MAX / 2 || row_bytes < 1) return SE3DS_E_BADSHAPE;
    if ((bpp != 1 && bpp != 3 && !(planes && bpp == 2)) || row_bytes % bpp != 0) return SE3DS_E_BADSHAPE;
    if (row_bytes > kEncodeMaxRowBytes) return SE3DS_E_UNSUPPORTED;
    if (mode < 0 || mode > (int64_t)deflate::kFilterAdaptive) return SE3DS_E_BADSHAPE;
    const Geometry g = geometry(height, row_bytes);
    if (g.out_bytes > 0x7fffffff) return SE3DS_E_UNSUPPORTED;   // sizes are uint32
    if (d[5] != strips || d[6] != outs || d[7] != slots) return SE3DS_E_BADSHAPE;
    strips += g.strips;
    outs += g.out_bytes;
    slots += g.strips * g.slot_bytes;
  }
  if (strips > 0x7fffffff) return SE3DS_E_UNSUPPORTED;
  *total_strips = strips;
  *slots_bytes = slots;
  *out_bytes = outs;
  return SE3DS_OK;
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_png_encode_fields(void) { return kEncodeFields; }
extern "C" int se3ds_png_encode_max_row_bytes(void) { return kEncodeMaxRowBytes; }

extern "C" uint32_t se3ds_adler32_combine(uint32_t a, uint32_t b, int64_t len_b) {
  uint32_t s1 = 0, s2 = 0;
  deflate::adler_combine(a & 0xffffu, a >> 16, b & 0xffffu, b >> 16, (uint64_t)(len_b < 0 ? 0 : len_b),
                         &s1, &s2);
  return (s2 << 16) | s1;
}

extern "C" size_t se3ds_png_encode_workspace_bytes(const int64_t* host_table, int n) {
  int64_t strips = 0, slots = 0, outs = 0;
  if (check_table(host_table, n, false, &strips, &slots, &outs) != SE3DS_OK) return 0;
  return (size_t)(meta_bytes(strips) + slots);
}

extern "C" int64_t se3ds_png_encode_out_bytes(const int64_t* host_table, int n) {
  int64_t strips = 0, slots = 0, outs = 0;
  if (check_table(host_table, n, false, &strips, &slots, &outs) != SE3DS_OK) return 0;
  return outs;
}

static int encode(const int64_t* table, const int64_t* host_table, int n, bool planes,
                  uint8_t* workspace, int64_t workspace_bytes, uint8_t* out, int64_t out_bytes,
                  uint32_t* sizes_dev, int phases, void* stream) {
  if (!table || !workspace || !out || !sizes_dev || phases < 1 || phases > 3) return SE3DS_E_BADSHAPE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return SE3DS_E_BADSHAPE;
  int64_t strips = 0, slots = 0, outs = 0;
  const int rc = check_table(host_table, n, planes, &strips, &slots, &outs);
  if (rc != SE3DS_OK) return rc;
  if (workspace_bytes < meta_bytes(strips) + slots) return SE3DS_E_WORKSPACE;
  if (out_bytes < outs) return SE3DS_E_BADSHAPE;
  if (phases & 1) {
    hipLaunchKernelGGL(png_encode_kernel, dim3((unsigned)strips), dim3(kWave), 0, as_stream(stream),
                       table, n, strips, workspace);
    const int launched = check_launch("png_encode");
    if (launched != SE3DS_OK) return launched;
  }
  if (!(phases & 2)) return SE3DS_OK;
  hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)strips), dim3(kCompactThreads), 0,
                     as_stream(stream), table, n, strips, workspace, out, sizes_dev);
  return check_launch("png_compact");
}

extern "C" int se3ds_png_encode(const int64_t* table, const int64_t* host_table, int n,
                                uint8_t* workspace, int64_t workspace_bytes, uint8_t* out,
                                int64_t out_bytes, uint32_t* sizes_dev, int phases, void* stream) {
  return encode(table, host_table, n, false, workspace, workspace_bytes, out, out_bytes, sizes_dev,
                phases, stream);
}

extern "C" size_t se3ds_png_encode_planes_workspace_bytes(const int64_t* host_table, int n) {
  int64_t strips = 0, slots = 0, outs = 0;
  if (check_table(host_table, n, true, &strips, &slots, &outs) != SE3DS_OK) return 0;
  return (size_t)(meta_bytes(strips) + slots);
}

extern "C" int64_t se3ds_png_encode_planes_out_bytes(const int64_t* host_table, int n) {
  int64_t strips = 0, slots = 0, outs = 0;
  if (check_table(host_table, n, true, &strips, &slots, &outs) != SE3DS_OK) return 0;
  return outs;
}

extern "C" int se3ds_png_encode_planes(const int64_t* table, const int64_t* host_table, int n,
                                       uint8_t* workspace, int64_t workspace_bytes, uint8_t* out,
                                       int64_t out_bytes, uint32_t* sizes_dev, int phases,
                                       void* stream) {
  return encode(table, host_table, n, true, workspace, workspace_bytes, out, out_bytes, sizes_dev,
                phases, stream);
}

extern "C" int se3ds_grid_quantize(const void* src, int dtype, int n, int h, int w, int c, int ny,
                                   int nx, int out_c, uint8_t* out, void* stream) {
  if (!src || !out || n < 1 || h < 1 || w < 1 || ny < 1 || nx < 1) return SE3DS_E_BADSHAPE;
  if ((c != 1 && c != 3) || (out_c != 1 && out_c != 3) || (c == 3 && out_c == 1)) return SE3DS_E_BADSHAPE;
  if ((int64_t)ny * nx > n) return SE3DS_E_BADSHAPE;
  const int64_t total = (int64_t)ny * h * nx * w * out_c;
  if (dtype == SE3DS_F32) {
    hipLaunchKernelGGL(grid_quantize_kernel<float>, dim3(grid_for(total, 256)), dim3(256), 0,
                       as_stream(stream), static_cast<const float*>(src), h, w, c, nx, out_c, total, out);
  } else if (dtype == SE3DS_BF16) {
    hipLaunchKernelGGL(grid_quantize_kernel<uint16_t>, dim3(grid_for(total, 256)), dim3(256), 0,
                       as_stream(stream), static_cast<const uint16_t*>(src), h, w, c, nx, out_c, total,
                       out);
  } else {
    return SE3DS_E_BADDTYPE;
  }
  return check_launch("grid_quantize");
}
