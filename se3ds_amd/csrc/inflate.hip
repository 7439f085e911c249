// zlib inflate of the IDAT streams of a batch of PNGs on the device: the first half of
// tf.image.decode_png (datasets/indoor_datasets.py:185-228), in front of png.hip's reconstruction.
// The decoder is inflate_core.h; this file is its 64-lane policy, the kernel and the entry point.
//
// Schedule: one wavefront (one 64-thread workgroup) per stream, grid = n, as png_unfilter_kernel.
// Deflate is serial in its symbols, so every lane decodes the same symbol from the same bits
// (wave-uniform control flow) and the lanes share what has width: the fetch of the next 1 KiB of
// compressed bytes into LDS, the construction of the decode tables of a dynamic block, the match
// copy (byte i of a match is byte i mod distance of the bytes before it -- all older than the
// match, so overlapping matches need no order between the lanes), and the flush.
//
// The 32 KiB window is an LDS ring of 64 KiB: a match reads what the same wave wrote through LDS,
// whose operations complete in order within a wave; nothing is read back from global memory.
// Granules of 16 KiB leave the ring as 16-byte stores (byte stores when the destination is not
// 16-byte aligned); the flush also sums the granule into the Adler-32 (per-lane partial sums of the
// bytes and of the bytes weighted by their distance to the granule's end, both below 2^32, reduced
// over the wave) and checks the filter-type byte of every scan line that starts in the granule.
// With one wave per workgroup the barriers cost a wait for the LDS counter, no more.
//
// LDS: ring 64 KiB + input chunk 1 KiB + five decode tables (code lengths, dynamic and fixed
// literal/length and distance) of 2784 B + 320 code lengths = 80 832 B static, two workgroups per
// CU.  No scratch, no atomics; plain loads and vector stores only.
#include "common.h"
#include "inflate_core.h"

namespace se3ds {
namespace {

constexpr int kInflateFields = 5;   // int64 per descriptor row

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

__global__ void __launch_bounds__(kWave)
png_inflate_kernel(const uint8_t* __restrict__ buf, uint8_t* __restrict__ workspace,
                   int32_t* __restrict__ status) {
  __shared__ inflate::Shared shared;
  const int64_t* d = reinterpret_cast<const int64_t*>(buf) + (int64_t)blockIdx.x * kInflateFields;
  const WavePolicy policy;
  inflate::Inflater<WavePolicy> inflater(policy, shared, buf + d[0], (uint32_t)d[1], workspace + d[2],
                                         (uint32_t)d[3], (uint32_t)d[4]);
  const int32_t word = inflater.run();
  if (threadIdx.x == 0) status[blockIdx.x] = word;
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_png_inflate_fields(void) { return kInflateFields; }
extern "C" int se3ds_png_inflate_ring_bytes(void) { return (int)inflate::kRingBytes; }

extern "C" int se3ds_png_inflate(const uint8_t* buf, int64_t buf_bytes, uint8_t* workspace,
                                 int64_t workspace_bytes, const int64_t* host_table, int n,
                                 int32_t* status_dev, void* stream) {
  if (n <= 0 || n > 65535 || !buf || !workspace || !host_table || !status_dev) return SE3DS_E_BADSHAPE;
  if ((reinterpret_cast<uintptr_t>(buf) & 7u) != 0 || workspace_bytes < 0) return SE3DS_E_BADSHAPE;
  const int64_t table_bytes = (int64_t)n * kInflateFields * (int64_t)sizeof(int64_t);
  if (buf_bytes < table_bytes) return SE3DS_E_BADSHAPE;
  const int64_t limit = (int64_t)inflate::kMaxStreamBytes;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = host_table + (int64_t)i * kInflateFields;
    const int64_t off = d[0], len = d[1], ws_off = d[2], expected = d[3], pitch = d[4];
    if (off < table_bytes || off > buf_bytes || len < 0 || len > limit || len > buf_bytes - off)
      return SE3DS_E_BADSHAPE;
    if (ws_off < 0 || ws_off > workspace_bytes || expected < 0 || expected > limit ||
        expected > workspace_bytes - ws_off)
      return SE3DS_E_BADSHAPE;
    if (pitch < 2 || pitch > limit || expected % pitch != 0) return SE3DS_E_BADSHAPE;
  }
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(kWave), 0, as_stream(stream), buf,
                     workspace, status_dev);
  return check_launch("png_inflate");
}
