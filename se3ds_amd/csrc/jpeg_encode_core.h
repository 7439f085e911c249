// Baseline JPEG encoding, the arithmetic: libjpeg's default encoder (jccolor's 16-bit colour
// conversion, h2v1 / h2v2 box downsampling with alternating bias, edge replication, the slow integer
// forward DCT of jfdctint, quantisation by rounded division, the Annex K Huffman tables) restated
// per 8 x 8 block so that every block is independent, and the placement of the blocks' bits as a scan.
// Plain C++17: csrc/jpeg_encode.hip runs these functions one lane a block, and
// tools/jpeg_encode_host_check.cpp runs them lane by lane on the host under the sanitizers.
//
// Three phases.
//   transform  pixels -> int16 quantised coefficients in zig-zag order, blocks in scan (MCU) order.
//              A workgroup stages a tile of one MCU row in LDS (every pixel read and converted
//              once, chroma downsampled on the way), then one lane a block transforms from LDS.
//              A block beyond the component's last block row or column ("dummy") has no AC and the
//              DC of the block libjpeg copies it from.
//   measure    a block's Huffman code, produced once: its bits, packed MSB first into 32-bit words
//              in a slot of kBlockWords words, and its length.  The DC predictor is the previous
//              block of the component in scan order, 0 at the start of a restart interval.
//              Where a block's bits begin in the batch's RAW stream (no FF stuffing yet) is a prefix
//              over `Span`s: a block adds its bits, the last block of an entropy segment also rounds
//              up to a byte and adds the 16 bits of the RSTn marker behind it.  Spans compose
//              associatively (`then`), so groups of kScanGroup blocks scan on their own and one
//              pass over the group aggregates gives every group its start.
//   pack       a unit of kPackBlocks blocks owns the raw bytes that BEGIN inside its blocks.  It ORs
//              the blocks' words (and the first word of the blocks behind it that share its last
//              byte) into a buffer, adds the 1-padding and the markers, counts the FF bytes that
//              are no marker and, once a prefix over the units' stuffed lengths is known, writes
//              the stuffed bytes to their final place.  Every output byte has one writer.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef SE3DS_HD
#if defined(__HIPCC__)
#define SE3DS_HD __host__ __device__ inline
#else
#define SE3DS_HD inline
#endif
#endif
#if defined(__HIPCC__)
#define SE3DS_JE_UNROLL _Pragma("unroll")
#else
#define SE3DS_JE_UNROLL
#endif

namespace se3ds {
namespace jpeg_encode {

constexpr int kFields = 48;          // int64 per row of the table: struct Image
constexpr int kScanGroup = 256;      // blocks per scan group (one workgroup of the measure launch)
constexpr int kPackBlocks = 64;      // blocks per pack unit (one workgroup of the pack launches)
constexpr int kTileBlocks = 240;     // blocks per transform tile at most: whole MCUs of 1, 3, 4 or 6 blocks
// The longest block: DC 11 + 11 bits (chroma category 11), 63 x (16 + 10) bits of AC = 1660 bits.
constexpr int kMaxBlockBits = 22 + 63 * 26;
constexpr int kBlockWords = (kMaxBlockBits + 31) / 32;   // 52: a slot is 208 bytes
// A unit's raw bytes: its blocks, each with up to 7 bits of padding and a marker, the byte it
// shares with the unit in front, one word of the blocks behind; in words, with slack.
constexpr int kUnitRawBytes = kPackBlocks * (4 * kBlockWords + 3) + 16;
constexpr int kUnitRawWords = kUnitRawBytes / 4 + 2;
constexpr int kUnitStageBytes = 2 * kUnitRawBytes + 32;
constexpr int kPackLanes = 256;

struct Image {
  int64_t src;            // device pointer of the pixels: height x width x ncomp uint8, contiguous
  int64_t width, height;  // 1..65535
  int64_t ncomp;          // 1 (a grey file) or 3
  int64_t h0, v0;         // luma sampling: 1x1, 2x1 or 2x2 (grey: 1x1); chroma is 1x1
  int64_t restart;        // MCUs per restart interval, 0: none
  int64_t first_block;    // blocks of the images in front
  int64_t first_tile;     // transform tiles of the images in front
  int64_t reserved[7];
  uint16_t quant[2][64];  // luma, chroma: 1..255, row-major order
};
static_assert(sizeof(Image) == kFields * 8, "a table row");

SE3DS_HD int64_t mcus_x(const Image& im) { return (im.width + 8 * im.h0 - 1) / (8 * im.h0); }
SE3DS_HD int64_t mcus_y(const Image& im) { return (im.height + 8 * im.v0 - 1) / (8 * im.v0); }
SE3DS_HD int slots_of(const Image& im) { return im.ncomp == 1 ? 1 : (int)(im.h0 * im.v0) + 2; }
SE3DS_HD int64_t blocks_of(const Image& im) { return mcus_x(im) * mcus_y(im) * slots_of(im); }
SE3DS_HD int64_t segments_of(const Image& im) {
  const int64_t m = mcus_x(im) * mcus_y(im);
  return im.restart ? (m + im.restart - 1) / im.restart : 1;
}

// the image whose blocks include `block`: the last row with first_block <= block
SE3DS_HD int image_of(const Image* table, int n, int64_t block) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_block <= block) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Where a block lies: its MCU, its component and its block coordinates in the component's plane.
struct Place {
  int64_t mcu;
  int slot, comp, bx, by;
  bool pred_zero;                       // the component's first block of an entropy segment
  bool seg_last, img_last;              // the last block of its entropy segment / of its image
  int rst;                              // the marker behind a seg_last block that is not img_last
};

SE3DS_HD Place place_of(const Image& im, int64_t local) {
  Place p;
  const int slots = slots_of(im), ny = slots == 1 ? 1 : slots - 2;
  p.mcu = local / slots;
  p.slot = (int)(local - p.mcu * slots);
  p.comp = p.slot < ny ? 0 : p.slot - ny + 1;
  p.bx = p.comp == 0 ? p.slot % (int)im.h0 : 0;
  p.by = p.comp == 0 ? p.slot / (int)im.h0 : 0;
  const int64_t mcus = mcus_x(im) * mcus_y(im);
  const bool mcu_first = im.restart ? p.mcu % im.restart == 0 : p.mcu == 0;
  const bool mcu_last = p.mcu + 1 == mcus || (im.restart && (p.mcu + 1) % im.restart == 0);
  p.pred_zero = mcu_first && (p.comp != 0 || p.slot == 0);
  p.seg_last = mcu_last && p.slot == slots - 1;
  p.img_last = p.mcu + 1 == mcus && p.slot == slots - 1;
  p.rst = im.restart ? (int)(((p.mcu + 1) / im.restart - 1) & 7) : 0;
  return p;
}

// ------------------------------------------------------------------------------- transform
// One sample of a component's plane at (x, y), which may lie beyond the plane: jccolor, then
// jcsample's edge rules.  Columns are replicated at full resolution; rows at full resolution only up
// to the vertical factor, and the last DOWNSAMPLED row fills the block.
struct Sampler {
  const uint8_t* src;
  int w, h, nc, h0, v0;

  SE3DS_HD int ycc(int c, int x, int y) const {   // x < w, y < h
    const uint8_t* p = src + ((int64_t)y * w + x) * nc;
    if (nc == 1) return p[0];
    const int r = p[0], g = p[1], b = p[2];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
  }

  SE3DS_HD int at(int c, int x, int y) const {
    if (c == 0 || h0 == 1) return ycc(c, x < w ? x : w - 1, y < h ? y : h - 1);
    const int rows = (h + v0 - 1) / v0;
    if (y > rows - 1) y = rows - 1;
    const int x0 = 2 * x < w ? 2 * x : w - 1, x1 = 2 * x + 1 < w ? 2 * x + 1 : w - 1;
    if (v0 == 1) return (ycc(c, x0, y) + ycc(c, x1, y) + (x & 1)) >> 1;
    const int y0 = 2 * y, y1 = 2 * y + 1 < h ? 2 * y + 1 : h - 1;
    return (ycc(c, x0, y0) + ycc(c, x1, y0) + ycc(c, x0, y1) + ycc(c, x1, y1) + 1 + (x & 1)) >> 2;
  }
};

// jfdctint: 13 constant bits, 2 pass-1 bits.  One pass over eight values; the second pass differs
// in the descaling only.
template <bool kRows>
SE3DS_HD void fdct_pass(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int kC = 13, kP = 2;
  constexpr int kOdd = kRows ? kC - kP : kC + kP;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
  const int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kRows) {
    d0 = (t10 + t11) * (1 << kP);
    d4 = (t10 - t11) * (1 << kP);
  } else {
    d0 = (t10 + t11 + (1 << (kP - 1))) >> kP;
    d4 = (t10 - t11 + (1 << (kP - 1))) >> kP;
  }
  constexpr int kRound = 1 << (kOdd - 1);
  int z1 = (t12 + t13) * 4433;
  d2 = (z1 + t13 * 6270 + kRound) >> kOdd;
  d6 = (z1 - t12 * 15137 + kRound) >> kOdd;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = (a4 + z1 + z3 + kRound) >> kOdd;
  d5 = (a5 + z2 + z4 + kRound) >> kOdd;
  d3 = (a6 + z2 + z3 + kRound) >> kOdd;
  d1 = (a7 + z1 + z4 + kRound) >> kOdd;
}

SE3DS_HD int quantise(int c, int q) {
  const int d = 8 * q, m = c < 0 ? -c : c;
  const int v = (m + (d >> 1)) / d;
  return c < 0 ? -v : v;
}

// 64 samples, fetch(row, column) -> 0..255, to 64 quantised coefficients in zig-zag order at `out`
// (4-byte aligned).  dc_only: a dummy block, which keeps the DC alone.
template <class Fetch>
SE3DS_HD void transform_block(Fetch fetch, const uint16_t* quant, bool dc_only, int16_t* out) {
  static constexpr uint8_t kNatural[64] = {
      0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  int d[64];
  SE3DS_JE_UNROLL
  for (int r = 0; r < 8; ++r) {
    SE3DS_JE_UNROLL
    for (int c = 0; c < 8; ++c) d[8 * r + c] = fetch(r, c) - 128;
    fdct_pass<true>(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5],
                    d[8 * r + 6], d[8 * r + 7]);
  }
  SE3DS_JE_UNROLL
  for (int c = 0; c < 8; ++c)
    fdct_pass<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
  SE3DS_JE_UNROLL
  for (int k = 0; k < 64; k += 2) {
    const int a = (dc_only && k > 0) ? 0 : quantise(d[kNatural[k]], quant[kNatural[k]]);
    const int b = dc_only ? 0 : quantise(d[kNatural[k + 1]], quant[kNatural[k + 1]]);
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint32_t*>(out)[k >> 1] = ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16);   // one store a pair
#else
    out[k] = (int16_t)a;
    out[k + 1] = (int16_t)b;
#endif
  }
}

// Which block of the MCU a luma block's samples come from.  A dummy block takes the DC of the block
// in front of it in the MCU's order: in a dummy row that is the last block of the row above, which
// may itself be a dummy column's copy of its left neighbour.  -> true for a dummy block.
SE3DS_HD bool luma_source(const Image& im, int64_t mx, int64_t my, int* bx, int* by) {
  const int64_t cols = (im.width + 7) / 8, rows = (im.height + 7) / 8;
  bool dummy = false;
  if (my * im.v0 + *by >= rows) {
    *by -= 1;
    *bx = (int)im.h0 - 1;
    dummy = true;
  }
  if (mx * im.h0 + *bx >= cols) {
    *bx -= 1;
    dummy = true;
  }
  return dummy;
}

// The direct form: block `local` of the image (scan order) straight from the pixels, every sample
// converted where it is needed.  The kernels run the tiled form below; the host check holds the
// tiled form against this one.
SE3DS_HD void transform(const Image& im, int64_t local, int16_t* out) {
  const Place p = place_of(im, local);
  const int64_t mx = p.mcu % mcus_x(im), my = p.mcu / mcus_x(im);
  const Sampler s = {reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(im.src)), (int)im.width,
                     (int)im.height, (int)im.ncomp, (int)im.h0, (int)im.v0};
  int bx = p.bx, by = p.by;
  const bool dummy = p.comp == 0 && luma_source(im, mx, my, &bx, &by);
  const int hc = p.comp == 0 ? (int)im.h0 : 1, vc = p.comp == 0 ? (int)im.v0 : 1;
  const int col = (int)(mx * hc + bx), row = (int)(my * vc + by), comp = p.comp;
  transform_block([&](int r, int c) { return s.at(comp, 8 * col + c, 8 * row + r); }, im.quant[comp ? 1 : 0], dummy,
                  out);
}

// The tiled form.  A tile is up to kTileBlocks / slots consecutive MCUs of one MCU row.  Load: the
// lanes walk the tile's pixel groups (h0 x v0 pixels, one chroma sample) in row order, so that
// neighbouring lanes read neighbouring pixels; every pixel is converted once, its Y goes to the luma
// plane in `sh`, the group's Cb and Cr are downsampled on the spot.  Then one lane a block runs the
// DCT on samples it reads from `sh`.
struct TileShared {
  alignas(16) uint8_t y[kTileBlocks * 64];
  alignas(16) uint8_t c[2][(kTileBlocks / 3) * 64];
};

struct Tile {
  int64_t my, mx0;   // the MCU row, the first MCU
  int count;         // MCUs
};

SE3DS_HD int tile_mcus(const Image& im) { return kTileBlocks / slots_of(im); }
SE3DS_HD int64_t tiles_x(const Image& im) { return (mcus_x(im) + tile_mcus(im) - 1) / tile_mcus(im); }
SE3DS_HD int64_t tiles_of(const Image& im) { return tiles_x(im) * mcus_y(im); }

SE3DS_HD int image_of_tile(const Image* table, int n, int64_t tile) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_tile <= tile) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

SE3DS_HD Tile tile_of(const Image& im, int64_t local) {
  Tile t;
  const int64_t tx = local % tiles_x(im);
  t.my = local / tiles_x(im);
  t.mx0 = tx * tile_mcus(im);
  const int64_t left = mcus_x(im) - t.mx0;
  t.count = (int)left < tile_mcus(im) ? (int)left : tile_mcus(im);
  return t;
}

SE3DS_HD void tile_load(int lane, int lanes, const Image& im, const Tile& t, TileShared& sh) {
  const Sampler s = {reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(im.src)), (int)im.width,
                     (int)im.height, (int)im.ncomp, (int)im.h0, (int)im.v0};
  const int across = t.count * 8, groups = across * 8, pitch = across * s.h0;
  const int chroma_rows = (s.h + s.v0 - 1) / s.v0;
  for (int i = lane; i < groups; i += lanes) {
    const int gy = i / across, gx = i - gy * across;
    const int cx = (int)t.mx0 * 8 + gx, cy = (int)t.my * 8 + gy;
    int cb = 0, cr = 0;
    for (int dy = 0; dy < s.v0; ++dy) {
      const int y = cy * s.v0 + dy < s.h ? cy * s.v0 + dy : s.h - 1;
      for (int dx = 0; dx < s.h0; ++dx) {
        const int x = cx * s.h0 + dx < s.w ? cx * s.h0 + dx : s.w - 1;
        const uint8_t* p = s.src + ((int64_t)y * s.w + x) * s.nc;
        int luma = p[0];
        if (s.nc == 3) {
          const int r = p[0], g = p[1], b = p[2];
          luma = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
          cb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
          cr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
        }
        sh.y[(gy * s.v0 + dy) * pitch + gx * s.h0 + dx] = (uint8_t)luma;
      }
    }
    if (s.nc != 3) continue;
    if (s.v0 == 2 && cy > chroma_rows - 1) {   // below the last downsampled row: that row, not the group
      cb = s.at(1, cx, cy);
      cr = s.at(2, cx, cy);
    } else if (s.h0 == 2) {
      const int bias = s.v0 == 2 ? 1 + (cx & 1) : (cx & 1);   // 2 x v0 samples: the shift is v0
      cb = (cb + bias) >> s.v0;
      cr = (cr + bias) >> s.v0;
    }
    sh.c[0][gy * across + gx] = (uint8_t)cb;
    sh.c[1][gy * across + gx] = (uint8_t)cr;
  }
}

// Lane `lane` < t.count * slots: its block of the tile, to `coef` (the image's first block).
SE3DS_HD void tile_dct(int lane, const Image& im, const Tile& t, const TileShared& sh, int16_t* coef) {
  const int slots = slots_of(im);
  if (lane >= t.count * slots) return;
  const int m = lane / slots;
  const Place p = place_of(im, ((t.my * mcus_x(im)) + t.mx0 + m) * slots + (lane - m * slots));
  int16_t* out = coef + ((t.my * mcus_x(im) + t.mx0) * slots + lane) * 64;
  const uint16_t* quant = im.quant[p.comp ? 1 : 0];
  const int across = t.count * 8;
  if (p.comp != 0) {
    const uint8_t* base = sh.c[p.comp - 1] + m * 8;
    transform_block([&](int r, int c) { return (int)base[r * across + c]; }, quant, false, out);
    return;
  }
  int bx = p.bx, by = p.by;
  const bool dummy = im.ncomp == 3 && luma_source(im, t.mx0 + m, t.my, &bx, &by);
  const int pitch = across * (int)im.h0;
  const uint8_t* base = sh.y + (by * 8) * pitch + (m * (int)im.h0 + bx) * 8;
  if (!dummy) {
    transform_block([&](int r, int c) { return (int)base[r * pitch + c]; }, quant, false, out);
    return;
  }
  // the forward DCT's DC is the sum of the 64 samples minus 128 each (pass 1: 4 x the row sums; pass
  // 2: (4 S + 2) >> 2 = S)
  int sum = 0;
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) sum += (int)base[r * pitch + c] - 128;
  for (int k = 0; k < 64; ++k) out[k] = 0;
  out[0] = (int16_t)quantise(sum, quant[0]);
}

// --------------------------------------------------------------------------------- measure
// T.81 Annex K.3 as (code << 8) | length per symbol: DC luma, AC luma, DC chroma, AC chroma.
struct Codes {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};

// Table `t` (0 = DC luma, 1 = AC luma, 2 = DC chroma, 3 = AC chroma) into `codes`: Annex C.
SE3DS_HD void build_codes(int t, Codes& codes) {
  static constexpr uint8_t kCounts[4][16] = {
      {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
      {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
      {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
      {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
  static constexpr uint8_t kAc[2][162] = {
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
       0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
       0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
       0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
       0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
       0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
       0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
       0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
       0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
      {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
       0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
       0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
       0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
       0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
       0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
       0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
       0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
       0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
  const bool ac = t & 1;
  const int id = t >> 1;
  uint32_t* dst = ac ? codes.ac[id] : codes.dc[id];
  if (ac)
    for (int i = 0; i < 256; ++i) dst[i] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < kCounts[t][l - 1]; ++i, ++k, ++code) dst[ac ? kAc[id][k] : k] = (code << 8) | (uint32_t)l;
    code <<= 1;
  }
}

SE3DS_HD int bit_length(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 32 - __clz((int)v);
#else
  int n = 0;
  while (v) {
    ++n;
    v >>= 1;
  }
  return n;
#endif
}

struct BitWriter {
  uint32_t* words;
  uint64_t acc;
  int pending, bits;

  SE3DS_HD void put(uint32_t value, int length) {   // length 1..26, value < 2^length
    acc = (acc << length) | value;
    pending += length;
    bits += length;
    if (pending >= 32) {
      pending -= 32;
      *words++ = (uint32_t)(acc >> pending);
    }
  }
  SE3DS_HD void flush() {   // the last word, zeros behind the bits
    if (pending) *words = (uint32_t)(acc << (32 - pending));
  }
};

// 64 zig-zag coefficients (16-byte aligned) -> the block's bits in `slot` (at most kBlockWords
// words are written, only those the bits reach); returns the bit count.  tab: 0 luma, 1 chroma.
SE3DS_HD int encode_block(const int16_t* zz, int pred, int tab, const Codes& codes, uint32_t* slot) {
  BitWriter w = {slot, 0, 0, 0};
  int run = 0;
  for (int j = 0; j < 8; ++j) {
    uint32_t four[4];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4*>(zz + 8 * j);
    four[0] = v.x, four[1] = v.y, four[2] = v.z, four[3] = v.w;
#else
    memcpy(four, zz + 8 * j, 16);
#endif
    SE3DS_JE_UNROLL
    for (int i = 0; i < 8; ++i) {
      int v = (int16_t)(four[i >> 1] >> (16 * (i & 1)));
      if (j == 0 && i == 0) {
        v -= pred;
        const int n = bit_length((uint32_t)(v < 0 ? -v : v));
        const uint32_t c = codes.dc[tab][n];
        const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1);
        w.put(((c >> 8) << n) | extra, (int)(c & 255) + n);
      } else if (v == 0) {
        ++run;
      } else {
        for (; run > 15; run -= 16) w.put(codes.ac[tab][0xF0] >> 8, (int)(codes.ac[tab][0xF0] & 255));
        const int n = bit_length((uint32_t)(v < 0 ? -v : v));
        const uint32_t c = codes.ac[tab][(run << 4) | n];
        const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1);
        w.put(((c >> 8) << n) | extra, (int)(c & 255) + n);
        run = 0;
      }
    }
  }
  if (run) w.put(codes.ac[tab][0] >> 8, (int)(codes.ac[tab][0] & 255));
  w.flush();
  return w.bits;
}

// The block whose DC is this block's predictor (global index; the caller has checked !pred_zero).
SE3DS_HD int64_t predictor_block(const Image& im, const Place& p, int64_t block) {
  const int slots = slots_of(im), ny = slots == 1 ? 1 : slots - 2;
  if (p.comp == 0) return p.slot > 0 ? block - 1 : block - slots + ny - 1;
  return block - slots;
}

// What a stretch of blocks does to the raw bit position p: p + a, or, when a segment ends inside
// it (r), roundup8(p + a) + b.
struct Span {
  uint64_t a, b;
  uint32_t r;
};

SE3DS_HD uint64_t round8(uint64_t v) { return (v + 7) & ~(uint64_t)7; }

SE3DS_HD Span span_of_block(const Place& p, int bits) {
  Span s = {(uint64_t)bits, 0, 0};
  if (p.seg_last) {
    s.r = 1;
    s.b = p.img_last ? 0 : 16;
  }
  return s;
}

SE3DS_HD Span then(const Span& f, const Span& g) {   // f, then g
  if (!g.r) return f.r ? Span{f.a, f.b + g.a, 1} : Span{f.a + g.a, 0, 0};
  return f.r ? Span{f.a, round8(f.b + g.a) + g.b, 1} : Span{f.a + g.a, g.b, 1};
}

SE3DS_HD uint64_t apply(const Span& f, uint64_t p) { return f.r ? round8(p + f.a) + f.b : p + f.a; }

// Spans inside a group fit 32 bits (256 x 1660 + markers); stored as two words, r in b's top bit.
struct Span32 {
  uint32_t a, b;
};
SE3DS_HD Span32 narrow(const Span& s) { return Span32{(uint32_t)s.a, (uint32_t)s.b | (s.r << 31)}; }
SE3DS_HD Span widen(const Span32& s) { return Span{s.a, s.b & 0x7fffffffu, s.b >> 31}; }

// The raw bit position of block b: `inclusive` holds, per block, the span of its group up to and
// including it; `group_start` the position of every group's first block and, behind the last
// group, the end of the stream.
SE3DS_HD uint64_t block_pos(const Span32* inclusive, const uint64_t* group_start, int64_t b, int64_t total) {
  if (b >= total) return group_start[(total + kScanGroup - 1) / kScanGroup];
  const uint64_t p0 = group_start[b / kScanGroup];
  return b % kScanGroup == 0 ? p0 : apply(widen(inclusive[b - 1]), p0);
}

// One lane's part of the pass over the group aggregates: lane `lane` of `lanes` folds its stretch
// of groups (step 1), lane 0 turns the lanes' spans into starts (step 2), every lane writes the
// starts of its stretch (step 3).  `carry`: one Span and one uint64 per lane.
SE3DS_HD void group_scan(int step, int lane, int lanes, const Span32* aggregate, int64_t groups, Span* carry,
                         uint64_t* carry_pos, uint64_t* group_start) {
  const int64_t per = (groups + lanes - 1) / lanes;
  const int64_t from = lane * per < groups ? lane * per : groups;
  const int64_t to = from + per < groups ? from + per : groups;
  if (step == 1) {
    Span s = {0, 0, 0};
    for (int64_t g = from; g < to; ++g) s = then(s, widen(aggregate[g]));
    carry[lane] = s;
  } else if (step == 2) {
    if (lane != 0) return;
    uint64_t p = 0;
    for (int l = 0; l < lanes; ++l) {
      carry_pos[l] = p;
      p = apply(carry[l], p);
    }
    group_start[groups] = p;
  } else {
    uint64_t p = carry_pos[lane];
    for (int64_t g = from; g < to; ++g) {
      group_start[g] = p;
      p = apply(widen(aggregate[g]), p);
    }
  }
}

// ------------------------------------------------------------------------------------ pack
struct PackShared {
  uint32_t raw[kUnitRawWords];         // the unit's raw bytes, MSB first in every word
  uint32_t marker[kUnitRawWords / 8 + 1];   // one bit a raw byte: a marker's FF, never stuffed
  uint32_t image_end[kPackBlocks];     // per block: the raw byte behind an image's last block, or ~0
  uint32_t image_index[kPackBlocks];
  uint32_t count[kPackLanes];          // FFs to stuff in every lane's stretch
  alignas(16) uint8_t stage[kUnitStageBytes];
};

struct Unit {
  int64_t b0, b1;
  uint64_t base_bit, end_bit;
  uint32_t first_byte, end_byte;   // the unit's own raw bytes, counted from base_bit / 8
};

SE3DS_HD Unit unit_of(int64_t u, int64_t total, const Span32* inclusive, const uint64_t* group_start) {
  Unit n;
  n.b0 = u * kPackBlocks;
  // 32-bit on purpose (the entry refuses more than 2^31 - 1 blocks): hipcc 7.x compiles this
  // wave-uniform select on 64-bit operands to a vector compare followed by a scalar select on SCC.
  // Any other wave-uniform 64-bit min / max / ?: in these kernels is exposed to the same; the clamps
  // in group_scan and jpeg_unit_scan_kernel are per lane, which compiles to vector selects.
  const int left = (int)(total - n.b0);
  n.b1 = n.b0 + (left < kPackBlocks ? left : kPackBlocks);
  const uint64_t p0 = block_pos(inclusive, group_start, n.b0, total);
  const uint64_t p1 = block_pos(inclusive, group_start, n.b1, total);
  n.base_bit = p0 & ~(uint64_t)7;
  n.first_byte = (p0 & 7) ? 1 : 0;
  n.end_byte = (uint32_t)((round8(p1) - n.base_bit) >> 3);
  n.end_bit = n.base_bit + 8 * (uint64_t)n.end_byte;
  return n;
}

SE3DS_HD void or_word(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);   // LDS: neighbouring blocks share words
#else
  *p |= v;
#endif
}

// `count` bits (<= 32), left-aligned in `w`, to bit `at` of the buffer
SE3DS_HD void deposit(uint32_t* raw, uint32_t at, uint32_t w) {
  const uint32_t i = at >> 5, s = at & 31;
  if (w >> s) or_word(raw + i, w >> s);
  if (s && (w << (32 - s))) or_word(raw + i + 1, w << (32 - s));
}

SE3DS_HD uint32_t raw_byte(const uint32_t* raw, uint32_t j) { return (raw[j >> 2] >> (24 - 8 * (j & 3))) & 255u; }

SE3DS_HD void pack_clear(int lane, int lanes, PackShared& sh) {
  for (int i = lane; i < kUnitRawWords; i += lanes) sh.raw[i] = 0;
  for (int i = lane; i < kUnitRawWords / 8 + 1; i += lanes) sh.marker[i] = 0;
  for (int i = lane; i < kPackBlocks; i += lanes) sh.image_end[i] = ~0u;
}

// Lane `lane` of `lanes` (a multiple of 4: four lanes share a block's words): the unit's blocks,
// then the blocks behind it that begin inside its last byte.
SE3DS_HD void pack_deposit(int lane, int lanes, const Unit& n, const Image* table, int n_images, int64_t total,
                           const Span32* inclusive, const uint64_t* group_start, const uint16_t* bits,
                           const uint32_t* slots, PackShared& sh) {
  const int part = lane & 3;
  for (int64_t b = n.b0 + (lane >> 2);; b += lanes >> 2) {
    if (b >= total) break;
    const uint64_t pos = block_pos(inclusive, group_start, b, total);
    const bool own = b < n.b1;
    if (!own && (pos >= n.end_bit || b >= n.b1 + 8)) break;   // 8: a block has 4 bits at least
    const uint32_t at = (uint32_t)(pos - n.base_bit);
    const uint32_t len = bits[b];
    const uint32_t words = own ? (len + 31) >> 5 : 1;
    const uint32_t* slot = slots + b * kBlockWords;
    for (uint32_t w = part; w < words; w += 4) deposit(sh.raw, at + 32 * w, slot[w]);
    if (part != 0) continue;
    const int img = image_of(table, n_images, b);
    const Place p = place_of(table[img], b - table[img].first_block);
    if (!p.seg_last) continue;
    const uint64_t end = pos + len, padded = round8(end);
    if (!own && end >= n.end_bit) continue;
    if (padded > end) deposit(sh.raw, (uint32_t)(end - n.base_bit), ~0u << (32 - (uint32_t)(padded - end)));
    if (!own) continue;
    const uint32_t byte = (uint32_t)((padded - n.base_bit) >> 3);
    if (p.img_last) {
      sh.image_end[b - n.b0] = byte;
      sh.image_index[b - n.b0] = (uint32_t)img;
    } else {
      deposit(sh.raw, 8 * byte, (0xFFD0u + (uint32_t)p.rst) << 16);
      or_word(sh.marker + (byte >> 5), 1u << (byte & 31));
    }
  }
}

SE3DS_HD bool stuffed(const PackShared& sh, uint32_t j) {
  return raw_byte(sh.raw, j) == 0xFF && !((sh.marker[j >> 5] >> (j & 31)) & 1u);
}

// the stretch of the unit's own bytes that lane `lane` counts and writes
SE3DS_HD void stretch(const Unit& n, int lane, int lanes, uint32_t* from, uint32_t* to) {
  const uint32_t own = n.end_byte - n.first_byte, per = (own + lanes - 1) / lanes;
  const uint32_t a = (uint32_t)lane * per < own ? (uint32_t)lane * per : own;
  *from = n.first_byte + a;
  *to = n.first_byte + (a + per < own ? a + per : own);
}

SE3DS_HD void pack_count(int lane, int lanes, const Unit& n, PackShared& sh) {
  uint32_t from, to, c = 0;
  stretch(n, lane, lanes, &from, &to);
  for (uint32_t j = from; j < to; ++j) c += stuffed(sh, j);
  sh.count[lane] = c;
}

// the unit's stuffed length (any lane, after pack_count)
SE3DS_HD uint32_t pack_length(int lanes, const Unit& n, const PackShared& sh) {
  uint32_t c = n.end_byte - n.first_byte;
  for (int l = 0; l < lanes; ++l) c += sh.count[l];
  return c;
}

// the stuffed offset, inside the unit, of its raw byte j (first_byte <= j <= end_byte)
SE3DS_HD uint32_t stuffed_offset(int lanes, const Unit& n, const PackShared& sh, uint32_t j) {
  uint32_t off = j - n.first_byte;
  for (int l = 0; l < lanes; ++l) {
    uint32_t from, to;
    stretch(n, l, lanes, &from, &to);
    if (to <= j) {
      off += sh.count[l];
    } else {
      for (uint32_t i = from; i < j; ++i) off += stuffed(sh, i);
      break;
    }
  }
  return off;
}

// Lane `lane`: its stretch, stuffed, into the stage at `shift` + its stuffed offset; and the start
// of every image that begins behind one of the unit's blocks into `starts`.
SE3DS_HD void pack_stuff(int lane, int lanes, const Unit& n, PackShared& sh, uint32_t shift, uint64_t unit_at,
                         int64_t* starts) {
  uint32_t from, to, off = shift;
  stretch(n, lane, lanes, &from, &to);
  for (int l = 0; l < lane; ++l) off += sh.count[l];
  off += from - n.first_byte;
  for (uint32_t j = from; j < to; ++j) {
    const uint32_t v = raw_byte(sh.raw, j);
    sh.stage[off++] = (uint8_t)v;
    if (stuffed(sh, j)) sh.stage[off++] = 0;
  }
  for (int k = lane; k < kPackBlocks; k += lanes)
    if (sh.image_end[k] != ~0u)
      starts[sh.image_index[k] + 1] = (int64_t)(unit_at + stuffed_offset(lanes, n, sh, sh.image_end[k]));
}

// Lane `lane`: the stage's `length` bytes from `shift` (= the destination's address modulo 16) to
// `dst`, 16 bytes a store where a whole aligned group is the unit's.
SE3DS_HD void pack_store(int lane, int lanes, const PackShared& sh, uint32_t shift, uint32_t length, uint8_t* dst) {
  const uint32_t end = shift + length;
  for (uint32_t g = 16 * (uint32_t)lane; g < end; g += 16 * (uint32_t)lanes) {
    if (g >= shift && g + 16 <= end) {
#if defined(__HIP_DEVICE_COMPILE__)
      *reinterpret_cast<uint4*>(dst + (g - shift)) = *reinterpret_cast<const uint4*>(sh.stage + g);
#else
      memcpy(dst + (g - shift), sh.stage + g, 16);
#endif
    } else {
      for (uint32_t i = g < shift ? shift : g; i < g + 16 && i < end; ++i) dst[i - shift] = sh.stage[i];
    }
  }
}

// ------------------------------------------------------------------------------ the bounds
// Bytes of entropy-coded output an image can need at most.  Raw: every block at most kMaxBlockBits
// bits <= 4 * kBlockWords bytes, every segment less than one byte of padding.  Stuffing doubles a
// byte at worst; every segment but the last adds a two-byte marker:
//   <= 2 * (blocks * 4 * kBlockWords + segments) + 2 * segments.
SE3DS_HD int64_t out_bound(const Image& im) { return blocks_of(im) * (8 * kBlockWords) + segments_of(im) * 4; }

}  // namespace jpeg_encode
}  // namespace se3ds
