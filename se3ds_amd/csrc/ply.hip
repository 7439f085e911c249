// Point-cloud bodies of a .ply file on the device (utils/ply.py): the ASCII lines `x y z r g b \n` of
// SE3DSModel.write_memory_as_pointcloud, byte for byte what the host loop prints, and the 15-byte
// binary_little_endian records.  The characters, the digit generation and the length bound are
// ply_format_core.h; this file is the placement: three kernels for the text, one for the records.
//
// Text.  Line lengths vary (19 to kMaxLineBytes = 109 bytes), so a line's place is a prefix sum.
//   A  ply_records_kernel: a workgroup takes kChunkPoints = 256 consecutive points, one per lane.  A
//      lane turns its three coordinates into records (decimal digits, exponent, class, length: 16
//      bytes each, one vector store), adds the lengths of its colours and the workgroup writes the
//      bytes of its chunk.  The powers-of-5 tables (1360 bytes) are copied to LDS first: a lookup is
//      a data-dependent pair of ds_read_b64.
//   S  ply_scan_kernel: one workgroup turns the chunk totals (at most 2^24 / 256 = 65536) into 64-bit
//      offsets and the byte count.
//   B  ply_emit_kernel: the same chunking.  The lanes scan their line lengths in LDS, write their
//      characters into an LDS staging buffer and the workgroup stores it with 16-byte vector stores.
//      The staging buffer starts at (destination address mod 16), so LDS and global memory agree on
//      the 16-byte grid; only the head and tail of a chunk (< 16 bytes each) go out as bytes.
// The order is the input order and there is no atomic anywhere: the same input gives the same bytes.
// Nothing is written outside [out, out + m * kMaxLineBytes): the entry point refuses a smaller
// buffer, and a chunk's offset plus its total is a sum of line lengths.
//
// Records.  ply_binary_kernel: a chunk of 256 points is 3840 bytes = 240 vectors; interleaved in LDS,
// stored as vectors.  A colour outside [0, 255] sets the flag word (a plain store of 1; every writer
// writes the same value) and its low byte is written.
#include "common.h"
#include "ply_format_core.h"

namespace se3ds {
namespace {

namespace pf = ply;

constexpr int kThreads = pf::kChunkPoints;
constexpr int kScanThreads = 256;
constexpr int kStageBytes = ((pf::kChunkPoints * pf::kMaxLineBytes + 15) & ~15) + 16;
constexpr int kBinaryChunkBytes = pf::kChunkPoints * pf::kBinaryRecordBytes;
static_assert(kThreads % kWave == 0 && kBinaryChunkBytes % 16 == 0, "whole waves, whole vectors");

__constant__ pf::Tables kTables = pf::make_tables();

__device__ __forceinline__ int32_t colour(const void* rgb, int dtype, int64_t at) {
  return dtype == SE3DS_U8 ? (int32_t) static_cast<const uint8_t*>(rgb)[at] : static_cast<const int32_t*>(rgb)[at];
}

// inclusive scan of one value per lane over the workgroup; `scratch` holds kThreads words
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* scratch) {
  const int tid = (int)threadIdx.x;
  scratch[tid] = v;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const uint32_t add = tid >= o ? scratch[tid - o] : 0u;
    __syncthreads();
    scratch[tid] += add;
    __syncthreads();
  }
  return scratch[tid];
}

__global__ void __launch_bounds__(kThreads)
ply_records_kernel(const float* __restrict__ coords, int64_t row_stride, const void* __restrict__ rgb, int dtype,
                   int64_t m, pf::Record* __restrict__ records, uint32_t* __restrict__ totals) {
  __shared__ uint64_t tables[pf::kTableWords];
  __shared__ uint32_t scratch[kThreads];
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < pf::kTableWords; i += kThreads) tables[i] = kTables.w[i];
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * kThreads + tid;
  uint32_t bytes = 0;
  if (p < m) {
    bytes = 1u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const pf::Record r = pf::to_decimal(__float_as_uint(coords[k * row_stride + p]), tables);
      records[p * 3 + k] = r;
      bytes += r.length + 1u + pf::int_length(colour(rgb, dtype, p * 3 + k)) + 1u;
    }
  }
  const uint32_t sum = block_scan(bytes, scratch);
  if (tid == kThreads - 1) totals[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(kScanThreads)
ply_scan_kernel(const uint32_t* __restrict__ totals, int chunks, int64_t* __restrict__ offsets,
                int64_t* __restrict__ out_bytes) {
  __shared__ int64_t sums[kScanThreads];
  const int tid = (int)threadIdx.x;
  const int per = (chunks + kScanThreads - 1) / kScanThreads;
  const int lo = tid * per < chunks ? tid * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
  int64_t sum = 0;
  for (int c = lo; c < hi; ++c) sum += totals[c];
  sums[tid] = sum;
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {
    const int64_t add = tid >= o ? sums[tid - o] : 0;
    __syncthreads();
    sums[tid] += add;
    __syncthreads();
  }
  int64_t run = sums[tid] - sum;
  for (int c = lo; c < hi; ++c) {
    offsets[c] = run;
    run += totals[c];
  }
  if (tid == kScanThreads - 1) *out_bytes = sums[tid];
}

__global__ void __launch_bounds__(kThreads)
ply_emit_kernel(const pf::Record* __restrict__ records, const void* __restrict__ rgb, int dtype, int64_t m,
                const int64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char stage[kStageBytes];
  __shared__ uint32_t scratch[kThreads];
  const int tid = (int)threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kThreads + tid;
  uint8_t* dst = out + offsets[blockIdx.x];
  const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  pf::Record xyz[3];
  int32_t c[3] = {0, 0, 0};
  uint32_t bytes = 0;
  if (p < m) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xyz[k] = records[p * 3 + k];
      c[k] = colour(rgb, dtype, p * 3 + k);
    }
    bytes = pf::line_length(xyz, c);
  }
  const uint32_t end = block_scan(bytes, scratch);
  if (p < m) pf::write_line(xyz, c, stage + skew + (end - bytes));
  const uint32_t total = scratch[kThreads - 1];   // <= kChunkPoints * kMaxLineBytes
  __syncthreads();
  // stage[skew + i] -> dst[i]: bytes up to the 16-byte grid, vectors, the rest as bytes
  uint32_t head = (16u - skew) & 15u;
  if (head > total) head = total;
  const uint32_t vectors = (total - head) / 16u, tail = head + vectors * 16u;
  if ((uint32_t)tid < head) dst[tid] = (uint8_t)stage[skew + tid];
  for (uint32_t v = (uint32_t)tid; v < vectors; v += kThreads)
    *reinterpret_cast<uint4*>(dst + head + 16u * v) = *reinterpret_cast<const uint4*>(stage + skew + head + 16u * v);
  if (tail + (uint32_t)tid < total) dst[tail + tid] = (uint8_t)stage[skew + tail + tid];
}

__global__ void __launch_bounds__(kThreads)
ply_binary_kernel(const float* __restrict__ coords, int64_t row_stride, const void* __restrict__ rgb, int dtype,
                  int64_t m, uint8_t* __restrict__ out, int32_t* __restrict__ flag) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kBinaryChunkBytes];
  const int tid = (int)threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * kThreads, p = first + tid;
  if (p < m) {
    uint8_t* at = stage + tid * pf::kBinaryRecordBytes;
    bool outside = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t bits = __float_as_uint(coords[k * row_stride + p]);
      at[4 * k] = (uint8_t)bits;
      at[4 * k + 1] = (uint8_t)(bits >> 8);
      at[4 * k + 2] = (uint8_t)(bits >> 16);
      at[4 * k + 3] = (uint8_t)(bits >> 24);
      const int32_t v = colour(rgb, dtype, p * 3 + k);
      outside = outside || v < 0 || v > 255;
      at[12 + k] = (uint8_t)v;
    }
    if (outside) *flag = 1;
  }
  __syncthreads();
  const int64_t left = m - first;
  const uint32_t total = (uint32_t)(left < kThreads ? left : kThreads) * pf::kBinaryRecordBytes;
  uint8_t* dst = out + first * pf::kBinaryRecordBytes;   // 16-byte aligned: out is, a chunk is 240 vectors
  const uint32_t vectors = total / 16u, tail = vectors * 16u;
  for (uint32_t v = (uint32_t)tid; v < vectors; v += kThreads)
    *reinterpret_cast<uint4*>(dst + 16u * v) = *reinterpret_cast<const uint4*>(stage + 16u * v);
  if (tail + (uint32_t)tid < total) dst[tail + tid] = stage[tail + tid];
}

struct Workspace {
  size_t records, totals, offsets, bytes;
};
Workspace layout(int64_t m) {
  const size_t chunks = (size_t)ceil_div(m, pf::kChunkPoints);
  Workspace w;
  w.records = 0;
  w.totals = (size_t)m * 3 * sizeof(pf::Record);
  w.offsets = w.totals + ((chunks * sizeof(uint32_t) + 15) & ~(size_t)15);
  w.bytes = w.offsets + ((chunks * sizeof(int64_t) + 15) & ~(size_t)15) + 16;
  return w;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int check_inputs(const float* coords, int64_t row_stride, const void* rgb, int dtype, int64_t m) {
  if (dtype != SE3DS_I32 && dtype != SE3DS_U8) return SE3DS_E_BADDTYPE;
  if (!pf::points_ok(m) || !coords || !rgb || row_stride < m || row_stride > ((int64_t)1 << 40)) return SE3DS_E_BADSHAPE;
  if (!aligned(coords, 4) || (dtype == SE3DS_I32 && !aligned(rgb, 4))) return SE3DS_E_BADSHAPE;
  return SE3DS_OK;
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_ply_chunk_points(void) { return pf::kChunkPoints; }
extern "C" int se3ds_ply_max_line_bytes(void) { return pf::kMaxLineBytes; }
extern "C" int64_t se3ds_ply_max_points(void) { return pf::kMaxPoints; }

extern "C" size_t se3ds_ply_ascii_workspace_bytes(int64_t m) { return pf::points_ok(m) ? layout(m).bytes : 0; }

extern "C" int se3ds_ply_ascii(const float* coords, int64_t row_stride, const void* rgb, int rgb_dtype, int64_t m,
                               uint8_t* out, int64_t out_capacity, int64_t* out_bytes, void* workspace,
                               size_t workspace_bytes, int phases, void* stream) {
  const int rc = check_inputs(coords, row_stride, rgb, rgb_dtype, m);
  if (rc != SE3DS_OK) return rc;
  if (!out || !out_bytes || !workspace || !aligned(out_bytes, 8) || !aligned(workspace, 16) || phases < 1 || phases > 7 ||
      out_capacity < m * pf::kMaxLineBytes)
    return SE3DS_E_BADSHAPE;
  const Workspace w = layout(m);
  if (workspace_bytes < w.bytes) return SE3DS_E_WORKSPACE;
  if (m == 0) return SE3DS_OK;
  char* base = static_cast<char*>(workspace);
  pf::Record* records = reinterpret_cast<pf::Record*>(base + w.records);
  uint32_t* totals = reinterpret_cast<uint32_t*>(base + w.totals);
  int64_t* offsets = reinterpret_cast<int64_t*>(base + w.offsets);
  const int chunks = (int)ceil_div(m, pf::kChunkPoints);
  if (phases & 1) {
    hipLaunchKernelGGL(ply_records_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, as_stream(stream), coords,
                       row_stride, rgb, rgb_dtype, m, records, totals);
    const int e = check_launch("ply_records");
    if (e != SE3DS_OK) return e;
  }
  if (phases & 2) {
    hipLaunchKernelGGL(ply_scan_kernel, dim3(1), dim3(kScanThreads), 0, as_stream(stream), totals, chunks, offsets,
                       out_bytes);
    const int e = check_launch("ply_scan");
    if (e != SE3DS_OK) return e;
  }
  if (phases & 4) {
    hipLaunchKernelGGL(ply_emit_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, as_stream(stream), records, rgb,
                       rgb_dtype, m, offsets, out);
    return check_launch("ply_emit");
  }
  return SE3DS_OK;
}

extern "C" int se3ds_ply_binary(const float* coords, int64_t row_stride, const void* rgb, int rgb_dtype, int64_t m,
                                uint8_t* out, int64_t out_capacity, int32_t* flag, void* stream) {
  const int rc = check_inputs(coords, row_stride, rgb, rgb_dtype, m);
  if (rc != SE3DS_OK) return rc;
  if (!out || !flag || !aligned(out, 16) || !aligned(flag, 4) || out_capacity < m * pf::kBinaryRecordBytes)
    return SE3DS_E_BADSHAPE;
  if (m == 0) return SE3DS_OK;
  const int chunks = (int)ceil_div(m, pf::kChunkPoints);
  hipLaunchKernelGGL(ply_binary_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, as_stream(stream), coords, row_stride,
                     rgb, rgb_dtype, m, out, flag);
  return check_launch("ply_binary");
}
