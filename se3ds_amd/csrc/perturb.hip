// Collision screen of the VLN perturbation augmentation (inference/perturbation_utils.py:63-70 of
// the reference): for K candidate offsets at once, the number of pixels of a window of a depth
// panorama with depth * DEPTH_SCALE < distance + padding.  The windows and thresholds are made on
// the host (se3ds_amd/inference/perturbation_utils.py: collision_windows); the reference slices and
// averages once per candidate on the host, here all K candidates are one launch.
//
// Layout of the work:
//   * grid = (blocks of kRows rows, candidates): blockIdx.y is the candidate, so its window, image
//     and threshold are uniform over the workgroup (scalar registers); a workgroup whose rows lie
//     below the window leaves at once;
//   * one wave per row, lanes along the row: a row segment is read as <= 3 single floats up to the
//     first 16-byte boundary, 16-byte loads of four pixels (64 lanes = 1 KiB contiguous), and <= 3
//     single floats at the end -- for any width, any col0 and any base address;
//   * a lane counts in a register over all its rows; one shuffle (DPP) sum per wave, one LDS
//     exchange per workgroup, one integer atomicAdd per workgroup that counted anything.  Integer
//     sums do not depend on the order: the result is deterministic.
//   * count is zeroed by a memset node on the same stream in front of the kernel.
// The windows are clamped to the image in the kernel as well: whatever the table holds, no lane
// reads outside its panorama (the host-side se3ds_collision_check_windows is what reports a bad
// table; the device never reads it back).
#include "common.h"

namespace se3ds {
namespace {

constexpr int kB = 256;                     // 4 waves
constexpr int kWaves = kB / kWave;
constexpr int kRows = 16;                   // rows per workgroup: 4 per wave

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kB)
collision_count_kernel(const float* __restrict__ depth, int n, int height, int width,
                       const int32_t* __restrict__ windows, const int32_t* __restrict__ image_index,
                       const float* __restrict__ threshold, float depth_scale,
                       int32_t* __restrict__ count) {
  const int c = (int)blockIdx.y;
  const int32_t* win = windows + 4 * (int64_t)c;
  const int row0 = max(win[0], 0), row1 = min(win[1], height);
  const int col0 = max(win[2], 0), col1 = min(win[3], width);
  const int img = image_index ? image_index[c] : 0;
  const int first = row0 + (int)blockIdx.x * kRows;
  if (first >= row1 || col0 >= col1 || img < 0 || img >= n) return;   // uniform over the workgroup
  const int last = min(first + kRows, row1);
  const float thr = threshold[c];
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int len = col1 - col0;
  int cnt = 0;
  for (int r = first + wave; r < last; r += kWaves) {
    const float* p = depth + ((int64_t)img * height + r) * width + col0;
    // floats up to the next 16-byte boundary (a float pointer is 4-byte aligned)
    const int head = min(len, (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u));
    const int nvec = (len - head) >> 2;
    const int tail = len - head - 4 * nvec;
    if (lane < head) cnt += (p[lane] * depth_scale < thr) ? 1 : 0;
    const float4* q = reinterpret_cast<const float4*>(p + head);
    for (int v = lane; v < nvec; v += kWave) {
      const float4 d = q[v];
      cnt += (d.x * depth_scale < thr) ? 1 : 0;
      cnt += (d.y * depth_scale < thr) ? 1 : 0;
      cnt += (d.z * depth_scale < thr) ? 1 : 0;
      cnt += (d.w * depth_scale < thr) ? 1 : 0;
    }
    if (lane < tail) cnt += (p[head + 4 * nvec + lane] * depth_scale < thr) ? 1 : 0;
  }
  __shared__ int part[kWaves];
  cnt = wave_sum_i32(cnt);
  if (lane == 0) part[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += part[w];
    if (total) atomicAdd(count + c, total);
  }
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_collision_check_windows(const int32_t* windows, const int32_t* image_index,
                                             int n, int height, int width, int k) {
  if (n <= 0 || height <= 0 || width <= 0 || k < 0 || (k > 0 && !windows)) return SE3DS_E_BADSHAPE;
  for (int c = 0; c < k; ++c) {
    const int32_t* w = windows + 4 * (int64_t)c;
    if (w[0] < 0 || w[0] > w[1] || w[1] > height) return SE3DS_E_BADSHAPE;
    if (w[2] < 0 || w[2] > w[3] || w[3] > width) return SE3DS_E_BADSHAPE;
    if (image_index && (image_index[c] < 0 || image_index[c] >= n)) return SE3DS_E_BADSHAPE;
  }
  return SE3DS_OK;
}

extern "C" int se3ds_collision_count(const float* depth, int n, int height, int width,
                                     const int32_t* windows, const int32_t* image_index,
                                     const float* threshold, float depth_scale, int k,
                                     int32_t* count, void* stream) {
  if (n <= 0 || height <= 0 || width <= 0 || k <= 0) return SE3DS_E_BADSHAPE;
  if (!depth || !windows || !threshold || !count) return SE3DS_E_BADSHAPE;
  if (k > 65535) return SE3DS_E_BADSHAPE;   // gridDim.y
  // a window holds fewer than 2^31 pixels: the int32 count cannot overflow
  if ((int64_t)height * width > INT32_MAX) return SE3DS_E_BADSHAPE;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)k, as_stream(stream));
  if (e != hipSuccess) {
    set_last_error(e, "collision_count memset");
    return SE3DS_E_LAUNCH;
  }
  const dim3 grid((unsigned)ceil_div(height, kRows), (unsigned)k);
  hipLaunchKernelGGL(collision_count_kernel, grid, dim3(kB), 0, as_stream(stream), depth, n, height,
                     width, windows, image_index, threshold, depth_scale, count);
  return check_launch("collision_count");
}
