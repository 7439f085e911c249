// PNG reconstruction (un-filtering) on the device: the second half of tf.image.decode_png
// (datasets/indoor_datasets.py:185-228) after the host has inflated the IDAT stream.  One launch
// reconstructs every plane of a batch from the filtered scan lines (filter-type byte + row_bytes
// filtered bytes per row, PNG specification section 9) straight into the raw uint8 / int16 tensors
// se3ds_input_transform reads.
//
// Arithmetic, on bytes: Recon(x) = Filt(x) + pred(a, b, c) mod 256, a = the byte one pixel to the
// left, b = the byte above, c = the byte above-left, all 0 outside the image; pred = 0 (None), a
// (Sub), b (Up), (a + b) >> 1 with a 9-bit sum (Average), Paeth with signed p = a + b - c and the
// tie order a, b, c.  16-bit samples are reconstructed as bytes with a pixel stride of 2 and stored
// byte-swapped (PNG is big-endian, the tensors little-endian).
//
// Schedule: one wavefront (one 64-thread workgroup) per image.  A pixel depends on its left, upper
// and upper-left neighbours, so the parallelism inside an image is a skewed wavefront: lane l owns
// row r0 + l of a band of 64 rows and reconstructs pixel t - l at step t.  a and c stay in the
// lane's registers, b arrives from lane l - 1 by one __shfl_up per step (it reconstructed the same
// column one step earlier).  Lane 0's b is the last row of the previous band: lane 63 leaves its
// row in an LDS carry row, position x at step x + 63, which lane 0 of the next band reads at step
// x -- one buffer is enough, a position is read 63 steps before the same band overwrites it.  No
// inter-wave communication of any kind.
//
// Staging: rows sit one pitch (1 + row_bytes, odd) apart, so a lane walking its own scan line would
// touch 64 cache lines per step for one byte each.  Instead a band is cut into time tiles of 64
// steps; the tile of lane l holds pixel columns [64 T - l, 64 T - l + 64) of its row (the skewed
// parallelogram laid out straight).  The wave fills the tile cooperatively -- for each row the 64
// lanes read 64 consecutive bytes -- the lanes reconstruct it in place, four pixels (BPP dwords) at
// a time, and the wave stores it the same way.  Tile rows are padded by one dword so that the
// lanes' dword accesses fall on distinct banks.
#include "common.h"

namespace se3ds {
namespace {

constexpr int kCols = 64;                    // pixels per lane per time tile
constexpr int kMaxRowBytes = 16384;          // LDS carry row
constexpr int kCarrySlack = 2 * kCols * 3;   // lane 0 reads up to 127 pixels past the row end
constexpr int kFields = 6;                   // int64 per descriptor row

template <int BPP>
struct Tile {
  static constexpr int kRowDwords = kCols * BPP / 4 + 1;   // odd: conflict-free across lanes
};

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int predict(int ft, int a, int b, int c) {
  const int avg = (a + b) >> 1;
  const int pth = paeth(a, b, c);
  int p = 0;
  p = ft == 1 ? a : p;
  p = ft == 2 ? b : p;
  p = ft == 3 ? avg : p;
  p = ft == 4 ? pth : p;
  return p;
}

template <int BPP, bool SWAP>
__device__ void unfilter_image(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int height,
                               int row_bytes, uint32_t* tile, uint32_t* carry) {
  constexpr int RD = Tile<BPP>::kRowDwords;
  constexpr int RB = RD * 4;
  const int lane = (int)threadIdx.x;
  const int width = row_bytes / BPP;
  const int64_t pitch = (int64_t)row_bytes + 1;
  uint8_t* tile8 = reinterpret_cast<uint8_t*>(tile);
  uint8_t* carry8 = reinterpret_cast<uint8_t*>(carry);
  for (int i = lane; i < (kMaxRowBytes + kCarrySlack) / 4; i += kWave) carry[i] = 0u;
  __syncthreads();

  for (int r0 = 0; r0 < height; r0 += kWave) {
    const int nb = height - r0 < kWave ? height - r0 : kWave;   // rows of this band
    const int row = r0 + lane;
    const bool live = row < height;
    int ft = live ? (int)src[(int64_t)row * pitch] : 0;
    ft = ft > 4 ? 0 : ft;   // the host rejects such a stream; never trust it with the predictor
    int a[BPP], c[BPP];
#pragma unroll
    for (int k = 0; k < BPP; ++k) a[k] = c[k] = 0;
    int last = 0;   // the pixel this lane reconstructed one step ago, bytes packed low to high
    const int tiles = (width + nb - 1 + kCols - 1) / kCols;
    for (int T = 0; T < tiles; ++T) {
      // ---- fill: row j of the tile = bytes [(64 T - j) BPP, +64 BPP) of scan line r0 + j
#pragma unroll 8
      for (int j = 0; j < kWave; ++j) {
        const int bs = (T * kCols - j) * BPP;
        const uint8_t* line = src + (int64_t)(r0 + j) * pitch + 1;
#pragma unroll
        for (int k = 0; k < BPP; ++k) {
          const int i = k * kWave + lane;
          const int pos = bs + i;
          uint8_t v = 0;
          if (j < nb && pos >= 0 && pos < row_bytes) v = line[pos];
          tile8[j * RB + i] = v;
        }
      }
      __syncthreads();
      // ---- reconstruct in place, four pixels (BPP dwords) per group
      uint32_t* mine = tile + lane * RD;
#pragma unroll 2
      for (int g = 0; g < kCols / 4; ++g) {
        uint32_t w[BPP], up0[BPP], o[BPP];
        const int xg = T * kCols + g * 4;   // lane 0's column; this lane's is xg - lane
#pragma unroll
        for (int k = 0; k < BPP; ++k) {
          w[k] = mine[g * BPP + k];
          up0[k] = carry[(xg * BPP) / 4 + k];   // wave-uniform address: a broadcast read
          o[k] = 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = xg + j - lane;
          int bpix = __shfl_up(last, 1, kWave);
          if (lane == 0) {
            bpix = 0;
#pragma unroll
            for (int k = 0; k < BPP; ++k) {
              const int bi = j * BPP + k;
              bpix |= (int)((up0[bi >> 2] >> (8 * (bi & 3))) & 0xffu) << (8 * k);
            }
          }
          const bool in = x >= 0;
          bpix = in ? bpix : 0;
          int packed = 0;
#pragma unroll
          for (int k = 0; k < BPP; ++k) {
            const int bi = j * BPP + k;
            const int f = (int)((w[bi >> 2] >> (8 * (bi & 3))) & 0xffu);
            const int b = (bpix >> (8 * k)) & 0xff;
            int r = (f + predict(ft, a[k], b, c[k])) & 0xff;
            r = in ? r : 0;
            a[k] = r;
            c[k] = b;
            packed |= r << (8 * k);
            const int bo = SWAP ? (bi ^ 1) : bi;
            o[bo >> 2] |= (uint32_t)r << (8 * (bo & 3));
          }
          last = packed;
          if (lane == kWave - 1 && in && x < width) {
#pragma unroll
            for (int k = 0; k < BPP; ++k) carry8[x * BPP + k] = (uint8_t)((packed >> (8 * k)) & 0xff);
          }
        }
#pragma unroll
        for (int k = 0; k < BPP; ++k) mine[g * BPP + k] = o[k];
      }
      __syncthreads();
      // ---- drain: the same bytes, reconstructed, to the destination plane
#pragma unroll 8
      for (int j = 0; j < kWave; ++j) {
        const int bs = (T * kCols - j) * BPP;
        uint8_t* line = dst + (int64_t)(r0 + j) * row_bytes;
#pragma unroll
        for (int k = 0; k < BPP; ++k) {
          const int i = k * kWave + lane;
          const int pos = bs + i;
          if (j < nb && pos >= 0 && pos < row_bytes) line[pos] = tile8[j * RB + i];
        }
      }
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(kWave)
png_unfilter_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table) {
  __shared__ uint32_t tile[kWave * Tile<3>::kRowDwords];
  __shared__ uint32_t carry[(kMaxRowBytes + kCarrySlack) / 4];
  const int64_t* d = table + (int64_t)blockIdx.x * kFields;
  const uint8_t* s = src + d[0];
  uint8_t* dst = reinterpret_cast<uint8_t*>(d[1]);
  const int height = (int)d[2], row_bytes = (int)d[3], bpp = (int)d[4];
  const bool swap = d[5] != 0;
  if (bpp == 1) unfilter_image<1, false>(s, dst, height, row_bytes, tile, carry);
  else if (bpp == 3) unfilter_image<3, false>(s, dst, height, row_bytes, tile, carry);
  else if (swap) unfilter_image<2, true>(s, dst, height, row_bytes, tile, carry);
  else unfilter_image<2, false>(s, dst, height, row_bytes, tile, carry);
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_png_unfilter_fields(void) { return kFields; }
extern "C" int se3ds_png_unfilter_max_row_bytes(void) { return kMaxRowBytes; }

extern "C" int se3ds_png_unfilter(const uint8_t* src, int64_t src_bytes, const int64_t* table,
                                  const int64_t* host_table, int n, void* stream) {
  if (n <= 0 || n > 65535 || src_bytes <= 0 || !src || !table || !host_table) return SE3DS_E_BADSHAPE;
  for (int i = 0; i < n; ++i) {
    const int64_t* d = host_table + (int64_t)i * kFields;
    const int64_t off = d[0], height = d[2], row_bytes = d[3], bpp = d[4], swap = d[5];
    if (d[1] == 0 || height < 1 || height > INT32_MAX / 2 || row_bytes < 1) return SE3DS_E_BADSHAPE;
    if (row_bytes > kMaxRowBytes) return SE3DS_E_UNSUPPORTED;
    if (bpp < 1 || bpp > 3 || row_bytes % bpp != 0 || (swap != 0 && swap != 1)) return SE3DS_E_BADSHAPE;
    if (swap && bpp != 2) return SE3DS_E_BADSHAPE;
    if (off < 0 || off > src_bytes || height * (row_bytes + 1) > src_bytes - off) return SE3DS_E_BADSHAPE;
  }
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(kWave), 0, as_stream(stream), src,
                     table);
  return check_launch("png_unfilter");
}
