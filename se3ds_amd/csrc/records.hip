// Writing R2R training records on the device (datasets/record_writer.py): the inverse of the input
// path of datasets/indoor_datasets.py:125-247.  Three entry points besides the PNG encoder's
// se3ds_png_encode_planes (png_encode.hip):
//
//   se3ds_record_planes      the warp's fp32 results (models/models.py:273-293: proj_rgb with its void
//                            class, proj_depth in [0, 1], proj_mask) -> the stored uint8 / uint16 /
//                            uint8 planes, one elementwise pass
//   se3ds_assemble_segments  n byte ranges from a few source buffers (the literals the host made,
//                            the encoder's compact streams) to their places in one file buffer
//   se3ds_patch_crc          device-resident CRC words into that buffer: PNG chunk CRCs (big-endian)
//                            and TFRecord's masked CRC-32C (little-endian)
//
// The CRCs themselves are se3ds_crc32z_multi / se3ds_crc32c_multi (crc32c.hip) over the assembled
// buffer.  No LDS, no atomics; every output byte has one writer, so a file is the same bytes on
// every run.  Every table is validated on its host copy before anything is launched, and the
// kernels skip a row of the device copy that leaves a buffer.
#include "common.h"

namespace se3ds {
namespace {

constexpr int kPlaneThreads = 256;
constexpr int kAssembleFields = 4;         // int64 per segment: source, source offset, destination, length
constexpr int kAssembleMaxSources = 8;
constexpr int64_t kAssembleMaxSegment = 1 << 16;   // one workgroup's share
constexpr int kAssembleThreads = 256;
constexpr int kPatchFields = 3;            // int64 per patch: CRC index, byte offset, form
constexpr int kPatchThreads = 64;

// ------------------------------------------------------------------------------- the planes
// tf.cast-like: truncated toward zero, saturated; the void class (-1), negatives and NaN are 0
__device__ __forceinline__ uint32_t rgb_code(float v) {
  return !(v > 0.0f) ? 0u : v >= 255.0f ? 255u : (uint32_t)(int)v;
}
// floor(d * 65535 + 0.5) in binary64 (the product is exact: 24 x 16 bits), saturated, NaN -> 0:
// the inverse of the decoder's u16 / 65535 for every code
__device__ __forceinline__ uint32_t depth_code(float d) {
  const double q = floor((double)d * 65535.0 + 0.5);
  return !(q > 0.0) ? 0u : q >= 65535.0 ? 65535u : (uint32_t)q;
}
__device__ __forceinline__ uint32_t mask_code(float m) { return m == 1.0f ? 255u : 0u; }

__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return a | (b << 8) | (c << 16) | (d << 24);
}

// VEC: every pointer is 16-byte aligned; a thread takes four pixels at a time (three 16-byte loads
// and three 4-byte stores of RGB, one 16-byte load and one 8-byte store of depth, one 16-byte load
// and one 4-byte store of the mask), the pixels % 4 behind them one by one.
template <bool VEC>
__global__ void __launch_bounds__(kPlaneThreads)
record_planes_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                     const float* __restrict__ mask, int64_t pixels, uint8_t* __restrict__ rgb_out,
                     uint16_t* __restrict__ depth_out, uint8_t* __restrict__ mask_out) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t quads = VEC ? pixels / 4 : 0;
  for (int64_t u = tid; u < quads; u += step) {
    if (rgb) {
      const float4* p = reinterpret_cast<const float4*>(rgb) + 3 * u;
      const float4 a = p[0], b = p[1], c = p[2];
      uint32_t* o = reinterpret_cast<uint32_t*>(rgb_out) + 3 * u;
      o[0] = pack4(rgb_code(a.x), rgb_code(a.y), rgb_code(a.z), rgb_code(a.w));
      o[1] = pack4(rgb_code(b.x), rgb_code(b.y), rgb_code(b.z), rgb_code(b.w));
      o[2] = pack4(rgb_code(c.x), rgb_code(c.y), rgb_code(c.z), rgb_code(c.w));
    }
    if (depth) {
      const float4 v = reinterpret_cast<const float4*>(depth)[u];
      reinterpret_cast<uint2*>(depth_out)[u] = make_uint2(depth_code(v.x) | (depth_code(v.y) << 16),
                                                          depth_code(v.z) | (depth_code(v.w) << 16));
    }
    if (mask) {
      const float4 v = reinterpret_cast<const float4*>(mask)[u];
      reinterpret_cast<uint32_t*>(mask_out)[u] =
          pack4(mask_code(v.x), mask_code(v.y), mask_code(v.z), mask_code(v.w));
    }
  }
  for (int64_t i = 4 * quads + tid; i < pixels; i += step) {
    if (rgb)
      for (int c = 0; c < 3; ++c) rgb_out[3 * i + c] = (uint8_t)rgb_code(rgb[3 * i + c]);
    if (depth) depth_out[i] = (uint16_t)depth_code(depth[i]);
    if (mask) mask_out[i] = (uint8_t)mask_code(mask[i]);
  }
}

// ------------------------------------------------------------------------------ the segments
struct Sources {
  const uint8_t* base[kAssembleMaxSources];
  int64_t bytes[kAssembleMaxSources];
};

// One workgroup per segment.  Stores: single bytes up to the first 16-byte boundary of the
// destination, 16 bytes at a time from there, single bytes behind the last whole 16.  Loads for a
// 16-byte store: one 16-byte load where the source address is a multiple of 16 too, four aligned
// words where it is a multiple of 4, otherwise the five aligned words that cover the 16 bytes,
// shifted together -- unless the first or the last of the five reaches outside the segment's source
// range (its first and last store only), where the 16 bytes are loaded one by one.
__global__ void __launch_bounds__(kAssembleThreads)
assemble_kernel(Sources src, int m, const int64_t* __restrict__ table, int n,
                uint8_t* __restrict__ out, int64_t out_bytes) {
  if ((int)blockIdx.x >= n) return;
  const int64_t* d = table + (int64_t)blockIdx.x * kAssembleFields;
  const int64_t which = d[0], from = d[1], to = d[2], len = d[3];
  // the device copy of a validated table; a row that would leave a buffer is skipped all the same
  if (which < 0 || which >= m || len < 1 || len > kAssembleMaxSegment) return;
  if (from < 0 || from > src.bytes[which] - len || to < 0 || to > out_bytes - len) return;
  const uint8_t* s = src.base[which] + from;
  uint8_t* dst = out + to;
  const int t = (int)threadIdx.x;
  int64_t head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
  if (head > len) head = len;
  if (t < head) dst[t] = s[t];
  const uint8_t* sb = s + head;
  uint8_t* db = dst + head;
  const int64_t vectors = (len - head) >> 4;
  const uintptr_t first = reinterpret_cast<uintptr_t>(s), end = first + (uintptr_t)len;
  const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(sb) & 3u);
  const bool aligned16 = (reinterpret_cast<uintptr_t>(sb) & 15u) == 0;
  for (int64_t v = t; v < vectors; v += kAssembleThreads) {
    const uint8_t* p = sb + 16 * v;
    uint32_t w[4];
    if (aligned16) {
      const uint4 q = *reinterpret_cast<const uint4*>(p);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else if (shift == 0) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = q[i];
    } else {
      const uintptr_t word0 = reinterpret_cast<uintptr_t>(p) - shift;
      if (word0 >= first && word0 + 20 <= end) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(word0);
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = q[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (x[i] >> (8 * shift)) | (x[i + 1] << (32 - 8 * shift));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          w[i] = pack4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
      }
    }
    *reinterpret_cast<uint4*>(db + 16 * v) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  const int64_t done = 16 * vectors;
  const int64_t tail = len - head - done;   // < 16
  if (t < tail) db[done + t] = sb[done + t];
}

// form 0: big-endian raw (a PNG chunk's CRC); form 1: TFRecord's masked CRC, little-endian
__global__ void __launch_bounds__(kPatchThreads)
patch_crc_kernel(const uint32_t* __restrict__ crc, int crc_count, const int64_t* __restrict__ table,
                 int n, uint8_t* __restrict__ out, int64_t out_bytes) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int64_t* d = table + (int64_t)i * kPatchFields;
  const int64_t which = d[0], at = d[1], form = d[2];
  if (which < 0 || which >= crc_count || at < 0 || at > out_bytes - 4) return;
  const uint32_t c = crc[which];
  uint8_t* p = out + at;
  if (form == 0) {
    p[0] = (uint8_t)(c >> 24);
    p[1] = (uint8_t)(c >> 16);
    p[2] = (uint8_t)(c >> 8);
    p[3] = (uint8_t)c;
  } else {
    const uint32_t masked = ((c >> 15) | (c << 17)) + 0xa282ead8u;
    p[0] = (uint8_t)masked;
    p[1] = (uint8_t)(masked >> 8);
    p[2] = (uint8_t)(masked >> 16);
    p[3] = (uint8_t)(masked >> 24);
  }
}

int check_segments(const int64_t* sources_host, int m, const int64_t* host_table, int n,
                   int64_t out_bytes) {
  if (!sources_host || !host_table || m < 1 || m > kAssembleMaxSources || n < 1 || n > (1 << 24) ||
      out_bytes < 0)
    return SE3DS_E_BADSHAPE;
  for (int j = 0; j < m; ++j)
    if (sources_host[2 * j] == 0 || sources_host[2 * j + 1] < 0) return SE3DS_E_BADSHAPE;
  int64_t filled = 0;   // the end of the destination in front
  for (int i = 0; i < n; ++i) {
    const int64_t* d = host_table + (int64_t)i * kAssembleFields;
    const int64_t which = d[0], from = d[1], to = d[2], len = d[3];
    if (which < 0 || which >= m || len < 0 || len > kAssembleMaxSegment) return SE3DS_E_BADSHAPE;
    if (from < 0 || from > sources_host[2 * which + 1] - len) return SE3DS_E_BADSHAPE;
    if (to < filled || to > out_bytes - len) return SE3DS_E_BADSHAPE;   // ascending, disjoint, inside
    filled = to + len;
  }
  return SE3DS_OK;
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_record_planes(const float* proj_rgb, const float* proj_depth,
                                   const float* proj_mask, int64_t pixels, uint8_t* rgb_out,
                                   uint16_t* depth_out, uint8_t* mask_out, void* stream) {
  if (pixels < 1 || pixels > (int64_t)1 << 40) return SE3DS_E_BADSHAPE;
  if (!proj_rgb != !rgb_out || !proj_depth != !depth_out || !proj_mask != !mask_out)
    return SE3DS_E_BADSHAPE;
  if (!proj_rgb && !proj_depth && !proj_mask) return SE3DS_E_BADSHAPE;
  if ((reinterpret_cast<uintptr_t>(proj_rgb) | reinterpret_cast<uintptr_t>(proj_depth) |
       reinterpret_cast<uintptr_t>(proj_mask)) & 3u)
    return SE3DS_E_BADSHAPE;
  if (reinterpret_cast<uintptr_t>(depth_out) & 1u) return SE3DS_E_BADSHAPE;
  const uintptr_t all = reinterpret_cast<uintptr_t>(proj_rgb) | reinterpret_cast<uintptr_t>(proj_depth) |
                        reinterpret_cast<uintptr_t>(proj_mask) | reinterpret_cast<uintptr_t>(rgb_out) |
                        reinterpret_cast<uintptr_t>(depth_out) | reinterpret_cast<uintptr_t>(mask_out);
  const dim3 grid(grid_for((pixels + 3) / 4, kPlaneThreads));
  if ((all & 15u) == 0)
    hipLaunchKernelGGL(record_planes_kernel<true>, grid, dim3(kPlaneThreads), 0, as_stream(stream),
                       proj_rgb, proj_depth, proj_mask, pixels, rgb_out, depth_out, mask_out);
  else
    hipLaunchKernelGGL(record_planes_kernel<false>, grid, dim3(kPlaneThreads), 0, as_stream(stream),
                       proj_rgb, proj_depth, proj_mask, pixels, rgb_out, depth_out, mask_out);
  return check_launch("record_planes");
}

extern "C" int se3ds_assemble_fields(void) { return kAssembleFields; }
extern "C" int64_t se3ds_assemble_max_segment_bytes(void) { return kAssembleMaxSegment; }
extern "C" int se3ds_patch_crc_fields(void) { return kPatchFields; }

extern "C" int se3ds_assemble_segments(const int64_t* sources_host, int m, const int64_t* table_dev,
                                       const int64_t* host_table, int n, uint8_t* out,
                                       int64_t out_bytes, void* stream) {
  if (!table_dev || !out) return SE3DS_E_BADSHAPE;
  const int rc = check_segments(sources_host, m, host_table, n, out_bytes);
  if (rc != SE3DS_OK) return rc;
  Sources src = {};
  for (int j = 0; j < m; ++j) {
    src.base[j] = reinterpret_cast<const uint8_t*>(sources_host[2 * j]);
    src.bytes[j] = sources_host[2 * j + 1];
  }
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)n), dim3(kAssembleThreads), 0, as_stream(stream),
                     src, m, table_dev, n, out, out_bytes);
  return check_launch("assemble_segments");
}

extern "C" int se3ds_patch_crc(const uint32_t* crc_dev, int crc_count, const int64_t* table_dev,
                               const int64_t* host_table, int n, uint8_t* out, int64_t out_bytes,
                               void* stream) {
  if (!crc_dev || !table_dev || !host_table || !out || crc_count < 1 || n < 1 || n > (1 << 24) ||
      out_bytes < 4)
    return SE3DS_E_BADSHAPE;
  if (reinterpret_cast<uintptr_t>(crc_dev) & 3u) return SE3DS_E_BADSHAPE;
  int64_t filled = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = host_table + (int64_t)i * kPatchFields;
    if (d[0] < 0 || d[0] >= crc_count || (d[2] != 0 && d[2] != 1)) return SE3DS_E_BADSHAPE;
    if (d[1] < filled || d[1] > out_bytes - 4) return SE3DS_E_BADSHAPE;   // ascending, disjoint, inside
    filled = d[1] + 4;
  }
  hipLaunchKernelGGL(patch_crc_kernel, dim3((unsigned)((n + kPatchThreads - 1) / kPatchThreads)),
                     dim3(kPatchThreads), 0, as_stream(stream), crc_dev, crc_count, table_dev, n, out,
                     out_bytes);
  return check_launch("patch_crc");
}
