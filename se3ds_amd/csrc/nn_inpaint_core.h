// Exact nearest-site transform behind nearest_neighbor_inpaint (utils/utils.py:179-198 of the
// reference): every void pixel takes the value of the nearest non-void pixel ("site") of its image,
// nearest by squared Euclidean distance in pixel units.  One text for two builds: the kernels of
// semantic.hip and a plain C++ program (tools/nn_inpaint_host_check.cpp) that runs both passes
// serially under the host sanitizers.  Everything is `__host__ __device__`; compiled without HIP it
// is ordinary C++.  Integers only.
//
// Tie rule.  The reference takes argmin over the sites in row-major order and the first minimum
// wins: among equidistant sites the smallest row, within that row the smallest column.
//
// Row pass.  table[r][x] = column of the site of row r that is horizontally nearest to x, the left
// one when two are equally far, kNoSite when the row has none.  It comes from two scans: the last
// site at or left of x (a running maximum of `site ? x : kNoSite`) and the first site at or right of
// x (a running minimum of `site ? x : kFarRight`), joined by pick_in_row.  Within one row no other
// site can be the answer: all sites of a row share the vertical distance, so the horizontally nearest
// wins, and two equally near ones differ only in column, where the smaller wins.
//
// Column pass.  nearest_site minimises (r - y)^2 + (table[r][x] - x)^2 over the rows r, comparing
// (distance, r) lexicographically, scanning outward dy = 0, 1, 2, ... with y - dy before y + dy.  It
// stops once dy^2 > the best distance: every later row is strictly farther.  The test is strict,
// because a row at dy^2 == best can tie and then wins if it lies above.
//
// Range: 1 <= H, W <= kMaxSide = 16384, so a column fits the int16 table, a flat index y * W + x
// fits 28 bits and a squared distance (< 2 * 2^28) fits int32.
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

namespace se3ds {
namespace nn_inpaint {

constexpr int kMaxSide = 16384;
constexpr int kNoSite = -1;            // table entry of a row without sites; also "no source"
constexpr int kFarRight = 1 << 20;     // identity of the right-to-left minimum
constexpr int kRowSegment = 256;       // columns a workgroup of the row pass scans at once
constexpr int kColTileRows = 4;        // rows (one wavefront each) of a workgroup of the column pass
constexpr int kColTileCols = 64;       // columns of that workgroup: one per lane
typedef int16_t Entry;                 // table element: W <= 16384 leaves the sign bit free

// pixel kinds: how equality with the void class is taken
constexpr int kKindU8 = 0, kKindI32 = 1, kKindF32 = 2;

// `bits` is the pixel zero-extended to 32 bits.  Integers: equality of the bits.  Floats: IEEE ==,
// so -0.0 equals a 0.0 void class and a NaN pixel (or a NaN void class) never matches.
SE3DS_HD bool is_void(uint32_t bits, uint32_t void_bits, int kind) {
  if (kind != kKindF32) return bits == void_bits;
  float a, b;
  memcpy(&a, &bits, sizeof a);
  memcpy(&b, &void_bits, sizeof b);
  return a == b;
}

// the scans' elements and operators
SE3DS_HD int left_seed(bool site, int x) { return site ? x : kNoSite; }
SE3DS_HD int right_seed(bool site, int x) { return site ? x : kFarRight; }
SE3DS_HD int left_join(int a, int b) { return a > b ? a : b; }
SE3DS_HD int right_join(int a, int b) { return a < b ? a : b; }

// l: last site at or left of x (kNoSite: none); r: first site at or right of x (kFarRight: none)
SE3DS_HD int pick_in_row(int x, int l, int r) {
  if (l == kNoSite) return r == kFarRight ? kNoSite : r;
  if (r == kFarRight) return l;
  return (x - l) <= (r - x) ? l : r;
}

// one candidate row of the column pass
struct Best {
  int32_t dist, row, col;
};
SE3DS_HD void consider(Best* best, const Entry* table, int w, int y, int x, int r) {
  const int sx = table[(int64_t)r * w + x];
  if (sx < 0 || sx >= w) return;   // kNoSite; nothing a stale table holds leads outside the image
  const int dy = r - y, dx = sx - x;
  const int32_t d = dy * dy + dx * dx;
  if (best->row == kNoSite || d < best->dist || (d == best->dist && r < best->row)) {
    best->dist = d;
    best->row = r;
    best->col = sx;
  }
}

// flat index row * w + col of the pixel that (y, x) takes its value from; kNoSite when the image has
// no site.  table: the row pass's h x w table of this image.
SE3DS_HD int32_t nearest_site(const Entry* table, int h, int w, int y, int x) {
  Best best = {0, kNoSite, kNoSite};
  const int last = y > h - 1 - y ? y : h - 1 - y;
  for (int dy = 0; dy <= last; ++dy) {
    if (best.row != kNoSite && dy * dy > best.dist) break;
    if (y - dy >= 0) consider(&best, table, w, y, x, y - dy);
    if (dy > 0 && y + dy < h) consider(&best, table, w, y, x, y + dy);
  }
  return best.row == kNoSite ? kNoSite : best.row * w + best.col;
}

SE3DS_HD bool shape_ok(int64_t n, int64_t h, int64_t w) {
  return n >= 1 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide;
}

// bytes of the table of n images, rounded up to 16
SE3DS_HD uint64_t table_bytes(int64_t n, int64_t h, int64_t w) {
  return (((uint64_t)n * (uint64_t)h * (uint64_t)w * sizeof(Entry)) + 15u) & ~(uint64_t)15u;
}

}  // namespace nn_inpaint
}  // namespace se3ds
