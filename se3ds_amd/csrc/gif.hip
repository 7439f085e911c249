// Animated GIF encode of a batch of videos on the device: roll-outs as files that play, and as the
// encoded_image_string of a TensorBoard image summary.  The format is DESIGN.md 3.18; the LZW step,
// the bit writer and the slot bound are gif_lzw_core.h; the median cut between the histogram and the
// look-up table, and the container, are the caller's (utils/gif.py).
//
//   histogram  gif_histogram_kernel  colour videos: a workgroup keeps all 32 768 bins of its video
//              in LDS (128 KiB, 32-bit counters, LDS atomic add), walks its share of the pixels four
//              at a time (three dwords) and adds its non-empty bins to the video's histogram with
//              global atomic adds.  Integer sums: the same counts whatever the order.
//   lut        gif_lut_kernel        one lane per bin centre, the palette in LDS: the used entry at
//              the least squared distance, the lowest index on a tie.
//   index      gif_index_kernel      the video's look-up table in LDS (32 KiB); four pixels a lane:
//              ordered dither, clamp, bin, look-up -> one dword of indices.  Grey videos are their
//              own index plane and are skipped.
//   lzw        gif_lzw_kernel        one wave per strip, the hash table in LDS (32 KiB): the walk of
//              gif_lzw_core.h -> the strip's bits in its slot and its bit count.
//   pack       gif_scan_kernel       one lane per frame: the exclusive scan of its strips' bit counts.
//              gif_pack_kernel       one lane per output byte: the strip that holds its first bit by
//              bisection, at most one more strip for the rest, shifted into place and stored behind
//              its sub-block's length byte; lane 0 of a frame writes the terminator and the size.
//
// Everything is queued on the caller's stream; nothing here synchronises with the host.
#include "common.h"
#include "gif_lzw_core.h"

namespace se3ds {
namespace {

constexpr int kBins = 32768;
constexpr int kHistLanes = 1024, kHistBlocks = 64;   // blocks per video at most
constexpr int kFields = 12;

// One row of the table, int64 each.  The caller fills the first six; se3ds_gif_plan the rest.
struct Video {
  int64_t src, frames, height, width, channels, dither;
  int64_t first_frame, first_strip, index_at, slot_at, out_at, frame_bytes;
};
static_assert(sizeof(Video) == kFields * 8, "the table row");

struct Layout {
  int64_t frames, strips, max_frame_data, max_pixels;
  int64_t hist_at, lut_at, index_at, slot_at, bits_at, start_at, bytes;
  int64_t sizes_bytes, out_bytes;
};

int64_t aligned16(int64_t n) { return (n + 15) & ~(int64_t)15; }

__host__ __device__ inline int64_t strips_per_frame(const Video& v) {
  return ceil_div(v.height, gif::strip_rows(v.width));
}
__host__ __device__ inline int64_t strip_slot(const Video& v) {
  return gif::strip_slot_bytes(gif::strip_rows(v.width) * v.width);
}

// The most data bytes a frame packs to, and what it takes with length bytes and terminator.
int64_t frame_data_bound(const Video& v) {
  const int64_t rows = gif::strip_rows(v.width), whole = v.height / rows, rest = v.height % rows;
  int64_t bits = whole * gif::strip_bits_bound(rows * v.width);
  if (rest) bits += gif::strip_bits_bound(rest * v.width);
  return (bits + 7) / 8;
}

int check_shapes(const int64_t* host_table, int n) {
  if (n < 1 || n > 65535 || !host_table) return SE3DS_E_BADSHAPE;
  const Video* videos = reinterpret_cast<const Video*>(host_table);
  for (int i = 0; i < n; ++i) {
    const Video& v = videos[i];
    if (v.src == 0 || v.frames < 1 || v.height < 1 || v.width < 1) return SE3DS_E_BADSHAPE;
    if (v.height > 65535 || v.width > 65535) return SE3DS_E_BADSHAPE;
    if (v.channels != 1 && v.channels != 3) return SE3DS_E_BADSHAPE;
    if (v.dither < 0 || v.dither > 255) return SE3DS_E_BADSHAPE;
  }
  return SE3DS_OK;
}

// Fills the derived fields (plan) or verifies them (!plan), and carves the workspace.
int walk_table(int64_t* host_table, int n, bool plan, Layout* l) {
  const int rc = check_shapes(host_table, n);
  if (rc != SE3DS_OK) return rc;
  Video* videos = reinterpret_cast<Video*>(host_table);
  int64_t frames = 0, strips = 0, index = 0, slot = 0, out = 0, max_data = 0, max_pixels = 0;
  for (int i = 0; i < n; ++i) {
    Video& v = videos[i];
    const int64_t data = frame_data_bound(v);
    const int64_t frame_bytes = aligned16(data + ceil_div(data, 255) + 1);
    if (plan) {
      v.first_frame = frames; v.first_strip = strips; v.index_at = index; v.slot_at = slot; v.out_at = out;
      v.frame_bytes = frame_bytes;
    } else if (v.first_frame != frames || v.first_strip != strips || v.index_at != index || v.slot_at != slot ||
               v.out_at != out || v.frame_bytes != frame_bytes) {
      return SE3DS_E_BADSHAPE;
    }
    const int64_t pixels = v.frames * v.height * v.width;
    frames += v.frames;
    strips += v.frames * strips_per_frame(v);
    if (v.channels == 3) index += aligned16(pixels);
    slot += v.frames * strips_per_frame(v) * strip_slot(v);
    out += v.frames * frame_bytes;
    if (data > max_data) max_data = data;
    if (pixels > max_pixels) max_pixels = pixels;
    if (frames > 0x7fffffff || strips > 0x7fffffff) return SE3DS_E_UNSUPPORTED;
  }
  l->frames = frames; l->strips = strips; l->max_frame_data = max_data; l->max_pixels = max_pixels;
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at = aligned16(at + bytes);
    return here;
  };
  l->hist_at = take((int64_t)n * kBins * 4);
  l->lut_at = take((int64_t)n * kBins);
  l->index_at = take(index);
  l->slot_at = take(slot);
  l->bits_at = take(strips * 4);
  l->start_at = take(strips * 8);
  l->bytes = at;
  l->sizes_bytes = aligned16(frames * 8);
  l->out_bytes = l->sizes_bytes + out;
  return SE3DS_OK;
}

int check_call(const int64_t* table, const int64_t* host_table, int n, const uint8_t* workspace,
               int64_t workspace_bytes, Layout* l) {
  if (!table || !workspace) return SE3DS_E_BADSHAPE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(table) & 7u) != 0)
    return SE3DS_E_BADSHAPE;
  const int rc = walk_table(const_cast<int64_t*>(host_table), n, false, l);
  if (rc != SE3DS_OK) return rc;
  if (workspace_bytes < l->bytes) return SE3DS_E_WORKSPACE;
  return SE3DS_OK;
}

__device__ __forceinline__ uint32_t bin_of(uint32_t r, uint32_t g, uint32_t b) {
  return (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3);
}

// grid (kHistBlocks, n), kHistLanes lanes, kBins * 4 bytes of dynamic LDS
__global__ void __launch_bounds__(kHistLanes)
gif_histogram_kernel(const Video* __restrict__ table, uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t s_bins[];   // [kBins]
  const Video v = table[blockIdx.y];
  if (v.channels != 3) return;
  const int64_t pixels = v.frames * v.height * v.width, quads = pixels / 4;
  if ((int64_t)blockIdx.x * kHistLanes >= quads && blockIdx.x != 0) return;   // nothing for this block
  for (int i = threadIdx.x; i < kBins; i += kHistLanes) s_bins[i] = 0;
  __syncthreads();
  const uint8_t* src = reinterpret_cast<const uint8_t*>(v.src);
  const bool dwords = (v.src & 3) == 0;
  for (int64_t q = (int64_t)blockIdx.x * kHistLanes + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kHistLanes) {
    if (dwords) {   // four pixels are three dwords: r g b r | g b r g | b r g b
      const uint32_t* p = reinterpret_cast<const uint32_t*>(src + q * 12);
      const uint32_t a = p[0], b = p[1], c = p[2];
      atomicAdd(&s_bins[bin_of(a & 255, a >> 8 & 255, a >> 16 & 255)], 1u);
      atomicAdd(&s_bins[bin_of(a >> 24, b & 255, b >> 8 & 255)], 1u);
      atomicAdd(&s_bins[bin_of(b >> 16 & 255, b >> 24, c & 255)], 1u);
      atomicAdd(&s_bins[bin_of(c >> 8 & 255, c >> 16 & 255, c >> 24)], 1u);
    } else {
      for (int k = 0; k < 4; ++k) {
        const uint8_t* p = src + q * 12 + k * 3;
        atomicAdd(&s_bins[bin_of(p[0], p[1], p[2])], 1u);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < pixels - quads * 4) {   // the last one to three pixels
    const uint8_t* p = src + (quads * 4 + threadIdx.x) * 3;
    atomicAdd(&s_bins[bin_of(p[0], p[1], p[2])], 1u);
  }
  __syncthreads();
  uint32_t* mine = hist + (int64_t)blockIdx.y * kBins;
  for (int i = threadIdx.x; i < kBins; i += kHistLanes) {
    const uint32_t count = s_bins[i];
    if (count) atomicAdd(&mine[i], count);
  }
}

// grid (kBins / 256, n), 256 lanes.  palettes: [n][256][3]; used: [n], 0 = no table for this video
__global__ void __launch_bounds__(256)
gif_lut_kernel(const uint8_t* __restrict__ palettes, const int32_t* __restrict__ used, uint8_t* __restrict__ lut) {
  __shared__ int32_t s_pal[256][3];
  const int video = blockIdx.y, count = used[video];
  if (count < 1) return;
  for (int k = 0; k < 3; ++k) s_pal[threadIdx.x][k] = palettes[((int64_t)video * 256 + threadIdx.x) * 3 + k];
  __syncthreads();
  const int bin = blockIdx.x * 256 + threadIdx.x;
  const int r = 8 * (bin >> 10) + 4, g = 8 * (bin >> 5 & 31) + 4, b = 8 * (bin & 31) + 4;
  int best = 0, best_d = 0x7fffffff;
  for (int i = 0; i < count && i < 256; ++i) {
    const int dr = r - s_pal[i][0], dg = g - s_pal[i][1], db = b - s_pal[i][2];
    const int d = dr * dr + dg * dg + db * db;
    if (d < best_d) {
      best_d = d;
      best = i;
    }
  }
  lut[(int64_t)video * kBins + bin] = (uint8_t)best;
}

__device__ __forceinline__ uint32_t bayer8(uint32_t x, uint32_t y) {
  // the recursive 8 x 8 matrix: bit-reversed interleave of (x ^ y, y), 0..63
  const uint32_t a = (x ^ y) & 7, b = y & 7;
  return (a & 1) << 5 | (b & 1) << 4 | (a & 2) << 2 | (b & 2) << 1 | (a & 4) >> 1 | (b & 4) >> 2;
}

__device__ __forceinline__ uint32_t dithered(uint32_t v, int off) {
  const int d = (int)v + off;
  return (uint32_t)(d < 0 ? 0 : d > 255 ? 255 : d);
}

// grid (blocks, n), 256 lanes
__global__ void __launch_bounds__(256)
gif_index_kernel(const Video* __restrict__ table, const uint8_t* __restrict__ lut, uint8_t* __restrict__ index) {
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[kBins];
  const Video v = table[blockIdx.y];
  if (v.channels != 3) return;
  const int64_t pixels = v.frames * v.height * v.width, quads = ceil_div(pixels, 4);
  if ((int64_t)blockIdx.x * 256 >= quads) return;
  const uint4* from = reinterpret_cast<const uint4*>(lut + (int64_t)blockIdx.y * kBins);
  for (int i = threadIdx.x; i < kBins / 16; i += 256) reinterpret_cast<uint4*>(s_lut)[i] = from[i];
  __syncthreads();
  const uint8_t* src = reinterpret_cast<const uint8_t*>(v.src);
  uint8_t* dst = index + v.index_at;   // 16-byte aligned, the video's pixels rounded up to 16
  const int amplitude = (int)v.dither;
  const uint32_t width = (uint32_t)v.width, height = (uint32_t)v.height;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t p = q * 4, row = p / width;
    uint32_t x = (uint32_t)(p - row * width), y = (uint32_t)(row % height);
    uint32_t word = 0;
    for (int k = 0; k < 4 && p + k < pixels; ++k) {
      const uint8_t* px = src + (p + k) * 3;
      const int off = (int)((bayer8(x, y) * amplitude) >> 6) - (amplitude >> 1);
      word |= (uint32_t)s_lut[bin_of(dithered(px[0], off), dithered(px[1], off), dithered(px[2], off))] << (8 * k);
      if (++x == width) {
        x = 0;
        if (++y == height) y = 0;
      }
    }
    *reinterpret_cast<uint32_t*>(dst + p) = word;
  }
}

struct DeviceWave {
  static constexpr int kLanes = kWave;
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ bool leader() const { return threadIdx.x == 0; }
  __device__ uint32_t pick(uint32_t mine, int j) const { return (uint32_t)__builtin_amdgcn_readlane((int)mine, j); }
  __device__ uint32_t uniform(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  __device__ void sync() const { __syncthreads(); }
};

// The video that holds item `id` of a running count (first_frame or first_strip).
template <int64_t Video::*kFirst>
__device__ __forceinline__ int video_of(const Video* table, int n, int64_t id) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (table[mid].*kFirst <= id) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one wave per strip
__global__ void __launch_bounds__(kWave)
gif_lzw_kernel(const Video* __restrict__ table, int n, const uint8_t* __restrict__ index, uint8_t* __restrict__ slots,
               uint32_t* __restrict__ bits) {
  __shared__ uint32_t s_table[gif::kTableSlots];
  const int64_t strip = blockIdx.x;
  const Video v = table[video_of<&Video::first_strip>(table, n, strip)];
  const int64_t per_frame = strips_per_frame(v), local = strip - v.first_strip;
  const int64_t frame = local / per_frame, k = local % per_frame, rows = gif::strip_rows(v.width);
  const int64_t row0 = k * rows, row1 = row0 + rows < v.height ? row0 + rows : v.height;
  const uint8_t* plane = v.channels == 1 ? reinterpret_cast<const uint8_t*>(v.src) : index + v.index_at;
  const uint8_t* px = plane + (frame * v.height + row0) * v.width;
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + v.slot_at + local * strip_slot(v));
  const DeviceWave w;
  const uint64_t total = gif::lzw_strip(w, px, (row1 - row0) * v.width, k == 0, k == per_frame - 1, s_table, out);
  if (threadIdx.x == 0) bits[strip] = (uint32_t)total;
}

// one lane per frame: where every strip's bits begin in the frame's stream
__global__ void __launch_bounds__(256)
gif_scan_kernel(const Video* __restrict__ table, int n, int64_t frames, const uint32_t* __restrict__ bits,
                uint64_t* __restrict__ start) {
  const int64_t frame = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (frame >= frames) return;
  const Video v = table[video_of<&Video::first_frame>(table, n, frame)];
  const int64_t per_frame = strips_per_frame(v);
  const int64_t first = v.first_strip + (frame - v.first_frame) * per_frame;
  uint64_t at = 0;
  for (int64_t s = 0; s < per_frame; ++s) {
    start[first + s] = at;
    at += bits[first + s];
  }
}

// grid (frames, blocks), 256 lanes: lane per data byte of the frame
__global__ void __launch_bounds__(256)
gif_pack_kernel(const Video* __restrict__ table, int n, const uint8_t* __restrict__ slots,
                const uint32_t* __restrict__ bits, const uint64_t* __restrict__ start, int64_t* __restrict__ sizes,
                uint8_t* __restrict__ out) {
  const int64_t frame = blockIdx.x;
  const Video v = table[video_of<&Video::first_frame>(table, n, frame)];
  const int64_t per_frame = strips_per_frame(v), slot_bytes = strip_slot(v);
  const int64_t first = v.first_strip + (frame - v.first_frame) * per_frame;
  const uint64_t total_bits = start[first + per_frame - 1] + bits[first + per_frame - 1];
  const int64_t data = (int64_t)((total_bits + 7) / 8);
  uint8_t* area = out + v.out_at + (frame - v.first_frame) * v.frame_bytes;
  const uint8_t* slot0 = slots + v.slot_at + (first - v.first_strip) * slot_bytes;
  for (int64_t p = (int64_t)blockIdx.y * 256 + threadIdx.x; p < data; p += (int64_t)gridDim.y * 256) {
    const uint64_t bit = (uint64_t)p * 8;
    int64_t lo = 0, hi = per_frame - 1;   // the last strip that begins at or before this bit
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (start[first + mid] <= bit) lo = mid; else hi = mid - 1;
    }
    const uint64_t local = bit - start[first + lo];
    const uint32_t have = bits[first + lo] - (uint32_t)local;   // >= 1 bits of this strip from here
    const uint8_t* s = slot0 + lo * slot_bytes + (local >> 3);
    uint32_t value = ((uint32_t)s[0] | (uint32_t)s[1] << 8) >> (local & 7);
    if (have < 8) {
      value &= (1u << have) - 1;
      // a strip is at least 18 bits: the next one fills the byte; behind the last strip it is padding
      if (lo + 1 < per_frame) value |= (uint32_t)slot0[(lo + 1) * slot_bytes] << have;
    }
    area[p + p / 255 + 1] = (uint8_t)value;
    if (p % 255 == 0) {
      const int64_t left = data - p;
      area[p + p / 255] = (uint8_t)(left < 255 ? left : 255);
    }
    if (p == 0) {
      const int64_t blocks = ceil_div(data, 255);
      area[data + blocks] = 0;
      sizes[frame] = data + blocks + 1;
    }
  }
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_gif_fields(void) { return kFields; }
extern "C" int se3ds_gif_strip_pixels(void) { return gif::kStripPixels; }
extern "C" int64_t se3ds_gif_strip_slot_bytes(int64_t pixels) { return pixels < 1 ? 0 : gif::strip_slot_bytes(pixels); }

extern "C" int se3ds_gif_plan(int64_t* host_table, int n) {
  Layout l;
  return walk_table(host_table, n, true, &l);
}

extern "C" size_t se3ds_gif_workspace_bytes(const int64_t* host_table, int n) {
  Layout l;
  return walk_table(const_cast<int64_t*>(host_table), n, false, &l) == SE3DS_OK ? (size_t)l.bytes : 0;
}

extern "C" int64_t se3ds_gif_out_bytes(const int64_t* host_table, int n) {
  Layout l;
  return walk_table(const_cast<int64_t*>(host_table), n, false, &l) == SE3DS_OK ? l.out_bytes : 0;
}

extern "C" int64_t se3ds_gif_workspace_offset(const int64_t* host_table, int n, int region) {
  Layout l;
  if (walk_table(const_cast<int64_t*>(host_table), n, false, &l) != SE3DS_OK) return -1;
  const int64_t at[7] = {l.hist_at, l.lut_at, l.index_at, l.slot_at, l.bits_at, l.start_at, l.bytes};
  return region >= 0 && region < 7 ? at[region] : -1;
}

extern "C" int se3ds_gif_histogram(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                                   int64_t workspace_bytes, void* stream) {
  Layout l;
  const int rc = check_call(table, host_table, n, workspace, workspace_bytes, &l);
  if (rc != SE3DS_OK) return rc;
  hipStream_t s = as_stream(stream);
  const size_t lds = (size_t)kBins * 4;
  if (!ensure_dynamic_lds((const void*)gif_histogram_kernel, lds)) return SE3DS_E_LAUNCH;
  const hipError_t e = hipMemsetAsync(workspace + l.hist_at, 0, (size_t)n * kBins * 4, s);
  if (e != hipSuccess) {
    set_last_error(e, "gif_histogram clear");
    return SE3DS_E_LAUNCH;
  }
  const int64_t blocks = ceil_div(ceil_div(l.max_pixels, 4), kHistLanes * 16);   // 64 pixels a lane and more
  const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > kHistBlocks ? kHistBlocks : blocks);
  hipLaunchKernelGGL(gif_histogram_kernel, dim3(gx, (unsigned)n), dim3(kHistLanes), lds, s,
                     reinterpret_cast<const Video*>(table), reinterpret_cast<uint32_t*>(workspace + l.hist_at));
  return check_launch("gif_histogram");
}

extern "C" int se3ds_gif_lut(const int64_t* table, const int64_t* host_table, int n, const uint8_t* palettes,
                             const int32_t* used, uint8_t* workspace, int64_t workspace_bytes, void* stream) {
  Layout l;
  const int rc = check_call(table, host_table, n, workspace, workspace_bytes, &l);
  if (rc != SE3DS_OK) return rc;
  if (!palettes || !used) return SE3DS_E_BADSHAPE;
  hipLaunchKernelGGL(gif_lut_kernel, dim3(kBins / 256, (unsigned)n), dim3(256), 0, as_stream(stream), palettes, used,
                     workspace + l.lut_at);
  return check_launch("gif_lut");
}

extern "C" int se3ds_gif_index(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                               int64_t workspace_bytes, void* stream) {
  Layout l;
  const int rc = check_call(table, host_table, n, workspace, workspace_bytes, &l);
  if (rc != SE3DS_OK) return rc;
  const int64_t blocks = ceil_div(ceil_div(l.max_pixels, 4), 256 * 8);
  const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > 512 ? 512 : blocks);
  hipLaunchKernelGGL(gif_index_kernel, dim3(gx, (unsigned)n), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const Video*>(table), workspace + l.lut_at, workspace + l.index_at);
  return check_launch("gif_index");
}

extern "C" int se3ds_gif_lzw(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                             int64_t workspace_bytes, void* stream) {
  Layout l;
  const int rc = check_call(table, host_table, n, workspace, workspace_bytes, &l);
  if (rc != SE3DS_OK) return rc;
  hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)l.strips), dim3(kWave), 0, as_stream(stream),
                     reinterpret_cast<const Video*>(table), n, workspace + l.index_at, workspace + l.slot_at,
                     reinterpret_cast<uint32_t*>(workspace + l.bits_at));
  return check_launch("gif_lzw");
}

extern "C" int se3ds_gif_pack(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                              int64_t workspace_bytes, uint8_t* out, int64_t out_bytes, void* stream) {
  Layout l;
  const int rc = check_call(table, host_table, n, workspace, workspace_bytes, &l);
  if (rc != SE3DS_OK) return rc;
  if (!out || (reinterpret_cast<uintptr_t>(out) & 7u) != 0 || out_bytes < l.out_bytes) return SE3DS_E_BADSHAPE;
  hipStream_t s = as_stream(stream);
  const Video* videos = reinterpret_cast<const Video*>(table);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(workspace + l.bits_at);
  uint64_t* start = reinterpret_cast<uint64_t*>(workspace + l.start_at);
  hipLaunchKernelGGL(gif_scan_kernel, dim3((unsigned)ceil_div(l.frames, 256)), dim3(256), 0, s, videos, n, l.frames,
                     bits, start);
  const int launched = check_launch("gif_scan");
  if (launched != SE3DS_OK) return launched;
  const int64_t blocks = ceil_div(l.max_frame_data, 256);
  const unsigned gy = (unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks);
  hipLaunchKernelGGL(gif_pack_kernel, dim3((unsigned)l.frames, gy), dim3(256), 0, s, videos, n, workspace + l.slot_at,
                     bits, start, reinterpret_cast<int64_t*>(out), out + l.sizes_bytes);
  return check_launch("gif_pack");
}
