// What a user does with a label panorama (utils/utils.py of the reference): fill its holes with the
// nearest label, score label maps against ground truth, turn labels into colours and back.
//
// Inpaint (nearest_neighbor_inpaint, utils/utils.py:179-198).  The reference forms every (site, void)
// pixel pair; here an exact separable nearest-site transform in two launches, integers throughout,
// no atomics, no floating point.  The arithmetic and the proof sketch are nn_inpaint_core.h.
//   * row pass: one workgroup per image row, kRowSegment columns at a time.  "Last site at or left
//     of x" is a running maximum: a 6-step wave scan (__shfl_up), the four wave totals through LDS,
//     and a carry in a uniform register from segment to segment, left to right.  The result is
//     parked in the table.  "First site at or right of x" is the mirrored minimum, segments right to
//     left; every thread reads back the entry it wrote itself (same thread, same address, program
//     order) and replaces it by the nearer of the two.  Table: int16 column per pixel, -1 = the row
//     has no site.
//   * column pass: one wavefront per row y and a run of adjacent x, so y, dy and the loop bound are
//     wave-uniform and the table reads of the wave fall into one contiguous run of the table's row.
//     Each lane runs nn_inpaint::nearest_site per pixel and leaves the loop when dy^2 exceeds its best
//     distance.
//     Non-void pixels copy through.  A lane owns one int32 / fp32 pixel or four adjacent uint8 pixels:
//     its load and store are a dword (the index plane: 16 bytes) wherever the row's address allows and
//     single elements otherwise, contiguous over the wave for any W and base address.
//
// Sequence metrics (compute_sequence_iou / compute_sequence_accuracy, utils/utils.py:98-176).
//   * seq_iou_partial_kernel / seq_label_partial_kernel: a workgroup reduces one chunk of kSumChunk
//     elements of one frame to (I, S) in binary64 -- each thread its own elements in a fixed order,
//     a shuffle butterfly per wave, the four waves through LDS in order -- and writes the pair to the
//     workspace.  seq_sums_reduce_kernel adds a frame's partials in a fixed order.  No atomics: the
//     same input at the same addresses gives the same bits on every run.  Built with
//     -ffp-contract=off: a term is rounded as written, never fused into the accumulation.
//     Loads are 16 bytes per lane (4 floats, 16 uint8 labels, 4 int32 labels) between a scalar head
//     up to the first 16-byte boundary and a scalar tail; two operands whose addresses differ mod 16
//     take the scalar path for the whole chunk.  The spatial mask is indexed per pixel.
//   * seq_finalize_kernel: the (N, T)-sized tail in fp32, sums in index order.
//
// Colours (cmap_to_label, create_label_colormap's inverse): the K <= 256 colours packed into one LDS
// word each, one pixel per lane, three single-element loads / byte stores per pixel, so nothing is
// read or written past the last pixel.
//
// All device stores are plain C++ vector stores.
#include <type_traits>

#include "common.h"
#include "nn_inpaint_core.h"

namespace se3ds {
namespace {

namespace nn = nn_inpaint;

constexpr int kRowWaves = nn::kRowSegment / kWave;
constexpr int kColThreads = nn::kColTileRows * kWave;
static_assert(nn::kRowSegment % kWave == 0 && nn::kColTileCols == kWave, "a wavefront per tile row");

template <int kKind>
__device__ __forceinline__ uint32_t load_bits(const void* p, int64_t i) {
  if (kKind == nn::kKindU8) return static_cast<const uint8_t*>(p)[i];
  return static_cast<const uint32_t*>(p)[i];
}
template <int kKind>
__device__ __forceinline__ void store_bits(void* p, int64_t i, uint32_t bits) {
  if (kKind == nn::kKindU8) static_cast<uint8_t*>(p)[i] = (uint8_t)bits;
  else static_cast<uint32_t*>(p)[i] = bits;
}

template <int kKind>
__global__ void __launch_bounds__(nn::kRowSegment)
nn_row_kernel(const void* __restrict__ image, uint32_t void_bits, int w, nn::Entry* __restrict__ table) {
  __shared__ int totals[kRowWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * w;
  const int segments = (w + nn::kRowSegment - 1) / nn::kRowSegment;
  int carry = nn::kNoSite;
  for (int seg = 0; seg < segments; ++seg) {
    const int x = seg * nn::kRowSegment + tid;
    const bool in = x < w;
    const bool site = in && !nn::is_void(load_bits<kKind>(image, base + (in ? x : 0)), void_bits, kKind);
    int v = nn::left_seed(site, x);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int t = __shfl_up(v, o, kWave);
      if (lane >= o) v = nn::left_join(v, t);
    }
    if (lane == kWave - 1) totals[wave] = v;
    __syncthreads();
    int before = carry, all = carry;
#pragma unroll
    for (int k = 0; k < kRowWaves; ++k) {
      if (k < wave) before = nn::left_join(before, totals[k]);
      all = nn::left_join(all, totals[k]);
    }
    if (in) table[base + x] = (nn::Entry)nn::left_join(v, before);
    carry = all;
    __syncthreads();
  }
  carry = nn::kFarRight;
  for (int seg = segments - 1; seg >= 0; --seg) {
    const int x = seg * nn::kRowSegment + tid;
    const bool in = x < w;
    const bool site = in && !nn::is_void(load_bits<kKind>(image, base + (in ? x : 0)), void_bits, kKind);
    int v = nn::right_seed(site, x);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int t = __shfl_down(v, o, kWave);
      if (lane + o < kWave) v = nn::right_join(v, t);
    }
    if (lane == 0) totals[wave] = v;
    __syncthreads();
    int after = carry, all = carry;
#pragma unroll
    for (int k = 0; k < kRowWaves; ++k) {
      if (k > wave) after = nn::right_join(after, totals[k]);
      all = nn::right_join(all, totals[k]);
    }
    if (in) table[base + x] = (nn::Entry)nn::pick_in_row(x, table[base + x], nn::right_join(v, after));
    carry = all;
    __syncthreads();
  }
}

// kPix adjacent pixels per lane: 4 for uint8 images, so that a lane's load and store are a dword
// wherever the row's address allows (any W and base address: bytes otherwise), 1 for int32 / fp32.
// The index plane goes out as one 16-byte store per lane under the same condition.
template <int kKind, int kPix>
__global__ void __launch_bounds__(kColThreads)
nn_col_kernel(const void* __restrict__ image, uint32_t void_bits, int h, int w,
              const nn::Entry* __restrict__ table, void* __restrict__ out, int32_t* __restrict__ indices) {
  static_assert(kPix == 1 || (kPix == 4 && kKind == nn::kKindU8), "four uint8 pixels make a dword");
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int y = (int)blockIdx.y * nn::kColTileRows + wave;
  const int x0 = ((int)blockIdx.x * nn::kColTileCols + lane) * kPix;
  if (y >= h || x0 >= w) return;
  const int64_t off = (int64_t)blockIdx.z * h * w;
  const int64_t at = off + (int64_t)y * w + x0;            // element index of the lane's first pixel
  const int count = w - x0 < kPix ? w - x0 : kPix;
  uint32_t bits[kPix];
  int32_t src[kPix];
  const uint8_t* in8 = static_cast<const uint8_t*>(image) + at;
  if (kPix == 4 && count == 4 && (reinterpret_cast<uintptr_t>(in8) & 3u) == 0) {
    const uint32_t word = *reinterpret_cast<const uint32_t*>(in8);
#pragma unroll
    for (int j = 0; j < kPix; ++j) bits[j] = (word >> (8 * j)) & 0xffu;
  } else {
#pragma unroll
    for (int j = 0; j < kPix; ++j) bits[j] = j < count ? load_bits<kKind>(image, at + j) : 0u;
  }
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    src[j] = y * w + x0 + j;
    if (j < count && nn::is_void(bits[j], void_bits, kKind)) {
      src[j] = nn::nearest_site(table + off, h, w, y, x0 + j);
      if (src[j] != nn::kNoSite) bits[j] = load_bits<kKind>(image, off + src[j]);
    }
  }
  uint8_t* out8 = static_cast<uint8_t*>(out) + at;
  if (kPix == 4 && count == 4 && (reinterpret_cast<uintptr_t>(out8) & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(out8) = bits[0] | (bits[1] << 8) | (bits[kPix > 2 ? 2 : 0] << 16) |
                                         (bits[kPix > 3 ? 3 : 0] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < kPix; ++j)
      if (j < count) store_bits<kKind>(out, at + j, bits[j]);
  }
  if (!indices) return;
  int32_t* ip = indices + at;
  if (kPix == 4 && count == 4 && (reinterpret_cast<uintptr_t>(ip) & 15u) == 0) {
    *reinterpret_cast<int4*>(ip) = make_int4(src[0], src[1], src[kPix > 2 ? 2 : 0], src[kPix > 3 ? 3 : 0]);
  } else {
#pragma unroll
    for (int j = 0; j < kPix; ++j)
      if (j < count) ip[j] = src[j];
  }
}

// ---------------------------------------------------------------------------------------------
// sums

constexpr int kSumThreads = 256;
constexpr int kSumWaves = kSumThreads / kWave;
constexpr int kSumChunk = 8192;   // elements of one frame per workgroup

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// (a, b) of every thread -> out[0], out[1]: butterfly per wave, waves in index order
__device__ __forceinline__ void block_sum_pair(double a, double b, double* out) {
  __shared__ double part[2][kSumWaves];
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  if (lane == 0) {
    part[0][wave] = a;
    part[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = part[0][0], sb = part[1][0];
#pragma unroll
    for (int k = 1; k < kSumWaves; ++k) {
      sa += part[0][k];
      sb += part[1][k];
    }
    out[0] = sa;
    out[1] = sb;
  }
}

// elements in front of the first 16-byte boundary of p (`size` bytes each), at most len; the whole
// chunk when q is not aligned like p
__device__ __forceinline__ int head_of(const void* p, const void* q, int size, int len) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  if (((a ^ b) & 15u) != 0) return len;
  const int head = (int)(((16u - (unsigned)(a & 15u)) & 15u) / (unsigned)size);
  return head < len ? head : len;
}

__global__ void __launch_bounds__(kSumThreads)
seq_iou_partial_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                       const float* __restrict__ spatial, int64_t elems, int64_t pixels, int channels,
                       int parts, double* __restrict__ partial) {
  const int64_t frame = (int64_t)blockIdx.x / parts;
  const int part = (int)((int64_t)blockIdx.x - frame * parts);
  const uint32_t e0 = (uint32_t)part * (uint32_t)kSumChunk;
  const int len = (int)(elems - e0 < kSumChunk ? elems - e0 : kSumChunk);
  const float* p = pred + frame * elems + e0;
  const float* t = truth + frame * elems + e0;
  const float* s = spatial ? spatial + frame * pixels : nullptr;
  const uint32_t c = (uint32_t)channels;
  const int tid = (int)threadIdx.x;
  double sum_i = 0.0, sum_s = 0.0;
  auto term = [&](float a, float b, uint32_t pixel) {
    const double da = (double)a, db = (double)b;
    if (s) {
      const double ds = (double)s[pixel];
      sum_i += da * db * ds;
      sum_s += (da + db) * ds;
    } else {
      sum_i += da * db;
      sum_s += da + db;
    }
  };
  const int head = head_of(p, t, 4, len);
  const int nvec = (len - head) >> 2;
  const int tail0 = head + 4 * nvec;
  for (int i = tid; i < head; i += kSumThreads) term(p[i], t[i], (e0 + (uint32_t)i) / c);
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  const float4* tv = reinterpret_cast<const float4*>(t + head);
  for (int v = tid; v < nvec; v += kSumThreads) {
    const float4 a = pv[v], b = tv[v];
    const uint32_t e = e0 + (uint32_t)head + 4u * (uint32_t)v;
    uint32_t q = e / c, r = e - q * c;
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      term(av[j], bv[j], q);
      if (++r == c) {
        r = 0;
        ++q;
      }
    }
  }
  for (int i = tail0 + tid; i < len; i += kSumThreads) term(p[i], t[i], (e0 + (uint32_t)i) / c);
  block_sum_pair(sum_i, sum_s, partial + 2 * (int64_t)blockIdx.x);
}

struct NoMask {};
template <class M> struct AccOf { typedef uint32_t type; };
template <> struct AccOf<int32_t> { typedef int64_t type; };
template <> struct AccOf<float> { typedef double type; };

// labels L = uint8_t / int32_t; spatial mask M = NoMask / uint8_t (also bool) / int32_t / float.
// A thread sees kSumChunk / kSumThreads = 32 elements of a chunk (a few more around a head), so a
// uint32 accumulator of uint8 weights cannot overflow; int32 weights accumulate in int64, fp32 in
// binary64.  The workgroup's totals continue in binary64, where integers below 2^53 are exact.
template <class L, class M>
__global__ void __launch_bounds__(kSumThreads)
seq_label_partial_kernel(const L* __restrict__ pred, const L* __restrict__ gt, const M* __restrict__ spatial,
                         int64_t pixels, int parts, double* __restrict__ partial) {
  typedef typename AccOf<M>::type Acc;
  constexpr bool kMasked = !std::is_same<M, NoMask>::value;
  constexpr int kVec = 16 / (int)sizeof(L);
  const int64_t frame = (int64_t)blockIdx.x / parts;
  const int part = (int)((int64_t)blockIdx.x - frame * parts);
  const int64_t e0 = (int64_t)part * kSumChunk;
  const int len = (int)(pixels - e0 < kSumChunk ? pixels - e0 : kSumChunk);
  const L* p = pred + frame * pixels + e0;
  const L* g = gt + frame * pixels + e0;
  const M* s = kMasked ? spatial + frame * pixels + e0 : nullptr;
  const int tid = (int)threadIdx.x;
  Acc sum_i = 0, sum_s = 0;
  auto term = [&](L a, L b, int i) {
    const Acc m = (Acc)(a == b ? 1 : 0);
    if constexpr (kMasked) {
      const Acc w = (Acc)s[i];
      sum_i += m * w;
      sum_s += w;
    } else {
      sum_i += m;
      sum_s += (Acc)1;
    }
  };
  const int head = head_of(p, g, (int)sizeof(L), len);
  const int nvec = (len - head) / kVec;
  const int tail0 = head + kVec * nvec;
  for (int i = tid; i < head; i += kSumThreads) term(p[i], g[i], i);
  const uint4* pv = reinterpret_cast<const uint4*>(p + head);
  const uint4* gv = reinterpret_cast<const uint4*>(g + head);
  for (int v = tid; v < nvec; v += kSumThreads) {
    const uint4 a = pv[v], b = gv[v];
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    const int i0 = head + kVec * v;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      if (sizeof(L) == 1)
        term((L)((aw[j >> 2] >> (8 * (j & 3))) & 0xffu), (L)((bw[j >> 2] >> (8 * (j & 3))) & 0xffu), i0 + j);
      else
        term((L)aw[j & 3], (L)bw[j & 3], i0 + j);
    }
  }
  for (int i = tail0 + tid; i < len; i += kSumThreads) term(p[i], g[i], i);
  block_sum_pair((double)sum_i, (double)sum_s, partial + 2 * (int64_t)blockIdx.x);
}

// sums[frame] = the frame's partial pairs added in a fixed order: thread k takes parts k, k + 256,
// ... in order, then the block sum
__global__ void __launch_bounds__(kSumThreads)
seq_sums_reduce_kernel(const double* __restrict__ partial, int parts, double* __restrict__ sums) {
  const double* p = partial + 2 * (int64_t)blockIdx.x * parts;
  double a = 0.0, b = 0.0;
  for (int k = (int)threadIdx.x; k < parts; k += kSumThreads) {
    a += p[2 * k];
    b += p[2 * k + 1];
  }
  block_sum_pair(a, b, sums + 2 * (int64_t)blockIdx.x);
}

__device__ __forceinline__ float divide_no_nan(float x, float y) { return y == 0.0f ? 0.0f : x / y; }

constexpr int kFinalThreads = 256;

__global__ void __launch_bounds__(kFinalThreads)
seq_finalize_kernel(const double* __restrict__ sums, const float* __restrict__ mask, int n, int t, int mode,
                    float* __restrict__ seq, float* __restrict__ mean) {
  __shared__ float example[kFinalThreads];
  const int tid = (int)threadIdx.x;
  float total = 0.0f;   // thread 0 only
  for (int n0 = 0; n0 < n; n0 += kFinalThreads) {
    const int b = n0 + tid;
    if (b < n) {
      float sum = 0.0f, length = 0.0f;
      for (int k = 0; k < t; ++k) {
        const int64_t f = (int64_t)b * t + k;
        const float m = mask[f];
        const float i32 = (float)sums[2 * f];
        const double s64 = mode == SE3DS_SEQ_IOU_LABELS ? 2.0 * sums[2 * f + 1] : sums[2 * f + 1];
        const float s32 = (float)s64;
        float v;
        if (mode == SE3DS_SEQ_ACCURACY) {
          v = divide_no_nan(i32, s32);
        } else {
          const float u = s32 - i32;
          v = divide_no_nan(i32 * m, u * m);
        }
        seq[f] = v;
        sum += v;
        length += m;
      }
      example[tid] = divide_no_nan(sum, length);
    }
    __syncthreads();
    if (tid == 0) {
      const int cnt = n - n0 < kFinalThreads ? n - n0 : kFinalThreads;
      for (int k = 0; k < cnt; ++k) total += example[k];
    }
    __syncthreads();
  }
  if (tid == 0) *mean = total / (float)n;
}

// ---------------------------------------------------------------------------------------------
// colours

constexpr int kColourThreads = 256;
constexpr int kMaxColours = 256;
constexpr uint32_t kNoColour = 0xffffffffu;   // a packed pixel has a zero top byte

__device__ __forceinline__ uint32_t pack_colour(int32_t r, int32_t g, int32_t b) {
  if (((r | g | b) & ~255) != 0) return kNoColour;
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

template <class T>
__global__ void __launch_bounds__(kColourThreads)
cmap_to_label_kernel(const T* __restrict__ image, int64_t pixels, const int32_t* __restrict__ cmap, int k,
                     int32_t* __restrict__ labels) {
  __shared__ uint32_t keys[kMaxColours];
  for (int i = (int)threadIdx.x; i < k; i += kColourThreads)
    keys[i] = pack_colour(cmap[3 * i], cmap[3 * i + 1], cmap[3 * i + 2]);
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kColourThreads;
  for (int64_t px = (int64_t)blockIdx.x * kColourThreads + threadIdx.x; px < pixels; px += stride) {
    const T* q = image + 3 * px;
    const uint32_t key = pack_colour((int32_t)q[0], (int32_t)q[1], (int32_t)q[2]);
    int32_t label = 0;
    if (key != kNoColour) {
      for (int i = 0; i < k; ++i) {
        if (keys[i] == key) {
          label = i;
          break;
        }
      }
    }
    labels[px] = label;
  }
}

template <class T>
__global__ void __launch_bounds__(kColourThreads)
label_to_color_kernel(const T* __restrict__ labels, int64_t pixels, const int32_t* __restrict__ cmap, int k,
                      uint8_t* __restrict__ out) {
  __shared__ uint32_t colours[kMaxColours];
  for (int i = (int)threadIdx.x; i < k; i += kColourThreads)
    colours[i] = ((uint32_t)cmap[3 * i] & 255u) | (((uint32_t)cmap[3 * i + 1] & 255u) << 8) |
                 (((uint32_t)cmap[3 * i + 2] & 255u) << 16);
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kColourThreads;
  for (int64_t px = (int64_t)blockIdx.x * kColourThreads + threadIdx.x; px < pixels; px += stride) {
    const int64_t label = (int64_t)labels[px];
    const uint32_t colour = label >= 0 && label < k ? colours[label] : 0u;
    uint8_t* q = out + 3 * px;
    q[0] = (uint8_t)(colour & 255u);
    q[1] = (uint8_t)((colour >> 8) & 255u);
    q[2] = (uint8_t)(colour >> 16);
  }
}

int kind_of(int dtype) {
  return dtype == SE3DS_U8 ? nn::kKindU8 : dtype == SE3DS_I32 ? nn::kKindI32 : dtype == SE3DS_F32 ? nn::kKindF32 : -1;
}

int64_t parts_of(int64_t elems) { return ceil_div(elems, kSumChunk); }

size_t sums_workspace_bytes(int64_t frames, int64_t elems) {
  return (((size_t)frames * (size_t)parts_of(elems) * 2 * sizeof(double)) + 15) & ~(size_t)15;
}

bool sums_shape_ok(int64_t frames, int64_t elems) {
  return frames >= 1 && elems >= 1 && elems <= INT32_MAX && frames <= INT32_MAX &&
         frames * parts_of(elems) <= INT32_MAX;
}

int reduce_partials(int64_t frames, int parts, const double* partial, double* sums, void* stream) {
  hipLaunchKernelGGL(seq_sums_reduce_kernel, dim3((unsigned)frames), dim3(kSumThreads), 0, as_stream(stream),
                     partial, parts, sums);
  return check_launch("seq_sums_reduce");
}

template <class L>
int launch_label_match(const void* pred, const void* gt, const void* spatial, int spatial_dtype, int64_t frames,
                       int64_t pixels, int parts, double* partial, void* stream) {
  const dim3 grid((unsigned)(frames * parts)), block(kSumThreads);
  const L* p = static_cast<const L*>(pred);
  const L* g = static_cast<const L*>(gt);
  hipStream_t st = as_stream(stream);
  if (!spatial)
    hipLaunchKernelGGL((seq_label_partial_kernel<L, NoMask>), grid, block, 0, st, p, g,
                       static_cast<const NoMask*>(nullptr), pixels, parts, partial);
  else if (spatial_dtype == SE3DS_U8)
    hipLaunchKernelGGL((seq_label_partial_kernel<L, uint8_t>), grid, block, 0, st, p, g,
                       static_cast<const uint8_t*>(spatial), pixels, parts, partial);
  else if (spatial_dtype == SE3DS_I32)
    hipLaunchKernelGGL((seq_label_partial_kernel<L, int32_t>), grid, block, 0, st, p, g,
                       static_cast<const int32_t*>(spatial), pixels, parts, partial);
  else
    hipLaunchKernelGGL((seq_label_partial_kernel<L, float>), grid, block, 0, st, p, g,
                       static_cast<const float*>(spatial), pixels, parts, partial);
  return check_launch("seq_label_match");
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_nn_inpaint_row_segment(void) { return nn::kRowSegment; }
extern "C" int se3ds_nn_inpaint_col_tile_rows(void) { return nn::kColTileRows; }

extern "C" size_t se3ds_nn_inpaint_workspace_bytes(int n, int h, int w) {
  return nn::shape_ok(n, h, w) ? (size_t)nn::table_bytes(n, h, w) : 0;
}

extern "C" int se3ds_nn_inpaint(const void* image, int dtype, uint32_t void_bits, int n, int h, int w, void* out,
                                int32_t* indices, void* workspace, size_t workspace_bytes, int phases,
                                void* stream) {
  if (!nn::shape_ok(n, h, w) || n > 65535 || (int64_t)n * h > INT32_MAX) return SE3DS_E_BADSHAPE;
  const int kind = kind_of(dtype);
  if (kind < 0) return SE3DS_E_BADDTYPE;
  if (!image || !out || !workspace || phases < 1 || phases > 3) return SE3DS_E_BADSHAPE;
  const unsigned elem = kind == nn::kKindU8 ? 0u : 3u;
  if ((reinterpret_cast<uintptr_t>(image) & elem) != 0 || (reinterpret_cast<uintptr_t>(out) & elem) != 0 ||
      (reinterpret_cast<uintptr_t>(indices) & 3u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
    return SE3DS_E_BADSHAPE;
  if (workspace_bytes < nn::table_bytes(n, h, w)) return SE3DS_E_WORKSPACE;
  nn::Entry* table = static_cast<nn::Entry*>(workspace);
  hipStream_t st = as_stream(stream);
  if (phases & 1) {
    const dim3 grid((unsigned)((int64_t)n * h)), block(nn::kRowSegment);
    if (kind == nn::kKindU8)
      hipLaunchKernelGGL(nn_row_kernel<nn::kKindU8>, grid, block, 0, st, image, void_bits, w, table);
    else if (kind == nn::kKindI32)
      hipLaunchKernelGGL(nn_row_kernel<nn::kKindI32>, grid, block, 0, st, image, void_bits, w, table);
    else
      hipLaunchKernelGGL(nn_row_kernel<nn::kKindF32>, grid, block, 0, st, image, void_bits, w, table);
    const int rc = check_launch("nn_inpaint rows");
    if (rc != SE3DS_OK) return rc;
  }
  if (phases & 2) {
    const int pix = kind == nn::kKindU8 ? 4 : 1;
    const dim3 grid((unsigned)ceil_div(w, nn::kColTileCols * pix), (unsigned)ceil_div(h, nn::kColTileRows), (unsigned)n);
    const dim3 block(kColThreads);
    if (kind == nn::kKindU8)
      hipLaunchKernelGGL((nn_col_kernel<nn::kKindU8, 4>), grid, block, 0, st, image, void_bits, h, w, table, out, indices);
    else if (kind == nn::kKindI32)
      hipLaunchKernelGGL((nn_col_kernel<nn::kKindI32, 1>), grid, block, 0, st, image, void_bits, h, w, table, out, indices);
    else
      hipLaunchKernelGGL((nn_col_kernel<nn::kKindF32, 1>), grid, block, 0, st, image, void_bits, h, w, table, out, indices);
    return check_launch("nn_inpaint columns");
  }
  return SE3DS_OK;
}

extern "C" int se3ds_seq_sums_chunk(void) { return kSumChunk; }

extern "C" size_t se3ds_seq_sums_workspace_bytes(int64_t frames, int64_t elems_per_frame) {
  return sums_shape_ok(frames, elems_per_frame) ? sums_workspace_bytes(frames, elems_per_frame) : 0;
}

extern "C" int se3ds_seq_iou_sums(const float* pred, const float* truth, const float* spatial, int64_t frames,
                                  int64_t pixels, int channels, double* sums, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (frames < 1 || pixels < 1 || channels < 1 || pixels > INT32_MAX / channels) return SE3DS_E_BADSHAPE;
  const int64_t elems = pixels * channels;
  if (!sums_shape_ok(frames, elems) || !pred || !truth || !sums || !workspace) return SE3DS_E_BADSHAPE;
  if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth) |
        reinterpret_cast<uintptr_t>(spatial)) & 3u) != 0 ||
      ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
    return SE3DS_E_BADSHAPE;
  if (workspace_bytes < sums_workspace_bytes(frames, elems)) return SE3DS_E_WORKSPACE;
  const int parts = (int)parts_of(elems);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(seq_iou_partial_kernel, dim3((unsigned)(frames * parts)), dim3(kSumThreads), 0,
                     as_stream(stream), pred, truth, spatial, elems, pixels, channels, parts, partial);
  const int rc = check_launch("seq_iou_sums");
  return rc != SE3DS_OK ? rc : reduce_partials(frames, parts, partial, sums, stream);
}

extern "C" int se3ds_seq_label_match(const void* pred, const void* gt, int label_dtype, const void* spatial,
                                     int spatial_dtype, int64_t frames, int64_t pixels, double* sums,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!sums_shape_ok(frames, pixels) || !pred || !gt || !sums || !workspace) return SE3DS_E_BADSHAPE;
  if (label_dtype != SE3DS_U8 && label_dtype != SE3DS_I32) return SE3DS_E_BADDTYPE;
  if (spatial && spatial_dtype != SE3DS_U8 && spatial_dtype != SE3DS_I32 && spatial_dtype != SE3DS_F32)
    return SE3DS_E_BADDTYPE;
  const unsigned lab = label_dtype == SE3DS_U8 ? 0u : 3u;
  const unsigned sp = spatial && spatial_dtype != SE3DS_U8 ? 3u : 0u;
  if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & lab) != 0 ||
      (reinterpret_cast<uintptr_t>(spatial) & sp) != 0 ||
      ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
    return SE3DS_E_BADSHAPE;
  if (workspace_bytes < sums_workspace_bytes(frames, pixels)) return SE3DS_E_WORKSPACE;
  const int parts = (int)parts_of(pixels);
  double* partial = static_cast<double*>(workspace);
  const int rc = label_dtype == SE3DS_U8
                     ? launch_label_match<uint8_t>(pred, gt, spatial, spatial_dtype, frames, pixels, parts, partial, stream)
                     : launch_label_match<int32_t>(pred, gt, spatial, spatial_dtype, frames, pixels, parts, partial, stream);
  return rc != SE3DS_OK ? rc : reduce_partials(frames, parts, partial, sums, stream);
}

extern "C" int se3ds_seq_finalize(const double* sums, const float* mask, int n, int t, int mode, float* seq,
                                  float* mean, void* stream) {
  if (n < 1 || t < 1 || !sums || !mask || !seq || !mean) return SE3DS_E_BADSHAPE;
  if (mode != SE3DS_SEQ_IOU && mode != SE3DS_SEQ_ACCURACY && mode != SE3DS_SEQ_IOU_LABELS) return SE3DS_E_BADSHAPE;
  hipLaunchKernelGGL(seq_finalize_kernel, dim3(1), dim3(kFinalThreads), 0, as_stream(stream), sums, mask, n, t,
                     mode, seq, mean);
  return check_launch("seq_finalize");
}

extern "C" int se3ds_cmap_to_label(const void* image, int dtype, int64_t pixels, const int32_t* cmap, int k,
                                   int32_t* labels, void* stream) {
  if (pixels < 1 || k < 1 || k > kMaxColours || !image || !cmap || !labels) return SE3DS_E_BADSHAPE;
  if (dtype != SE3DS_U8 && dtype != SE3DS_I32) return SE3DS_E_BADDTYPE;
  const dim3 grid((unsigned)grid_for(pixels, kColourThreads)), block(kColourThreads);
  if (dtype == SE3DS_U8)
    hipLaunchKernelGGL(cmap_to_label_kernel<uint8_t>, grid, block, 0, as_stream(stream),
                       static_cast<const uint8_t*>(image), pixels, cmap, k, labels);
  else
    hipLaunchKernelGGL(cmap_to_label_kernel<int32_t>, grid, block, 0, as_stream(stream),
                       static_cast<const int32_t*>(image), pixels, cmap, k, labels);
  return check_launch("cmap_to_label");
}

extern "C" int se3ds_label_to_color(const void* labels, int dtype, int64_t pixels, const int32_t* cmap, int k,
                                    uint8_t* out, void* stream) {
  if (pixels < 1 || k < 1 || k > kMaxColours || !labels || !cmap || !out) return SE3DS_E_BADSHAPE;
  if (dtype != SE3DS_U8 && dtype != SE3DS_I32) return SE3DS_E_BADDTYPE;
  const dim3 grid((unsigned)grid_for(pixels, kColourThreads)), block(kColourThreads);
  if (dtype == SE3DS_U8)
    hipLaunchKernelGGL(label_to_color_kernel<uint8_t>, grid, block, 0, as_stream(stream),
                       static_cast<const uint8_t*>(labels), pixels, cmap, k, out);
  else
    hipLaunchKernelGGL(label_to_color_kernel<int32_t>, grid, block, 0, as_stream(stream),
                       static_cast<const int32_t*>(labels), pixels, cmap, k, out);
  return check_launch("label_to_color");
}
