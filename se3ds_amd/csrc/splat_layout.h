// Host arithmetic of the warp's splat (geom.hip): where every array of the caller-owned workspace
// lives, how the points are cut into chunks, and which of the four routes -- scatter, binned, packed,
// sorted -- a call takes.  Each workspace is described ONCE, as a walk of a Carver: with the
// workspace's address the walk hands out the pointers, from address 0 the same walk gives the size.  One
// text for two builds: geom.hip and a plain C++ program (tools/splat_layout_host_check.cpp) under the
// host sanitizers.  Everything is `__host__ __device__`; compiled without HIP it is ordinary C++17.
// It reads no environment variable: geom.hip reads the switches and passes their values in.
//
// Workspace (bytes):
//   header and sink partials          see SplatWs
//   int32 idx[n * m], float z[n * m]  first-stage flat index and depth of every point
//   splat_route_region_offset(n, m):  the arrays of the route the call takes (BinWs / PackWs / SortWs)
// se3ds_splat_workspace_bytes = that offset + the largest of the three routes' regions + 16.
//
// The declarations sit in an unnamed namespace because the *Ws structs are kernel arguments of
// geom.hip's kernels, which live in one: the kernels' symbols name their argument types.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SE3DS_HD
#if defined(__HIPCC__)
#define SE3DS_HD __host__ __device__ inline
#else
#define SE3DS_HD inline
#endif
#endif

namespace se3ds {
namespace {

SE3DS_HD size_t align16(size_t v) { return (v + 15) / 16 * 16; }
SE3DS_HD int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// base + running offset.  take<T>(count) returns the next array and advances by its size rounded up
// to 16 bytes, so every array starts 16-byte aligned when the base is.  Integer arithmetic: base 0 is
// the measuring walk (the "pointers" are then the offsets, `off` at the end is the size).
struct Carver {
  uintptr_t base;
  size_t off;
  template <typename T>
  SE3DS_HD T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += align16(sizeof(T) * count);
    return p;
  }
};

// ------------------------------------------------------------------ header, idx, z (every route)
// [0,256) of the header: u32 sink_z (ordered), u32 sink_feat[C<=60];
//   u32 zpart[kMaxSinkBlocks], u32 fpart[kMaxSinkBlocks][C] (per-block sink partials: the
//   reference's sink pixel collects EVERY invalid point, and one atomic per wave on a single
//   address serialises at ~12 ns each -- 200-600 us at 4 M points; per-block partials plus a
//   one-block reduce cost ~3 us);  then int32 idx[N*M], float z[N*M].
constexpr int kMaxSinkBlocks = 2048;
constexpr int kMaxSplatChannels = 60;
struct SplatWs {
  uint32_t* sink_z;      // word 0; words 1-2 unused, word 3 the sticky promise flag (kPromiseStickyWord)
  uint32_t* sink_feat;   // [kMaxSplatChannels]: the header proper ends at byte 256
  uint32_t* zpart;       // [kMaxSinkBlocks]
  uint32_t* fpart;       // [kMaxSinkBlocks][C]
  int32_t* idx;          // [n * m]
  float* z;              // [n * m]
};
SE3DS_HD size_t splat_points(int n, int64_t m) { return (size_t)n * (size_t)(m > 0 ? m : 0); }
SE3DS_HD SplatWs splat_ws(Carver& c, int n, int64_t m) {
  SplatWs w;
  w.sink_z = c.take<uint32_t>(4);
  w.sink_feat = c.take<uint32_t>(kMaxSplatChannels);
  w.zpart = c.take<uint32_t>(kMaxSinkBlocks);
  w.fpart = c.take<uint32_t>((size_t)kMaxSinkBlocks * kMaxSplatChannels);
  // idx and z are one take: z follows idx without padding (4-byte aligned, as it always was)
  const size_t pts = splat_points(n, m);
  w.idx = c.take<int32_t>(2 * pts);
  w.z = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(w.idx) + sizeof(int32_t) * pts);
  return w;
}
SE3DS_HD SplatWs carve_ws(void* ws, int n, int64_t m) {
  Carver c{(uintptr_t)ws, 0};
  return splat_ws(c, n, m);
}
// where the route's own arrays begin -- and with them the control words of the packed and sorted
// routes, which se3ds_splat_promise_broken reads
SE3DS_HD size_t splat_route_region_offset(int n, int64_t m) {
  Carver c{0, 0};
  splat_ws(c, n, m);
  return c.off;
}
SE3DS_HD Carver route_carver(void* ws, int n, int64_t m) {
  return Carver{(uintptr_t)ws, splat_route_region_offset(n, m)};
}

// ------------------------------------------------------------------ chunks of points
// The points of one image are cut into contiguous CHUNKS (one workgroup each, the same cut in the
// count and the scatter pass).  Each chunk owns a histogram row, so record positions come from a
// column scan of those rows: no global atomics anywhere (2 M cursor atomics cost ~70 us before).
constexpr int kChunkThreads = 512;
constexpr int kChunkPoints = 8192;   // minimum points per chunk (16 per thread)
constexpr int kMaxChunks = 1024;     // per image
struct ChunkGeom {
  int chunks;     // per image
  int64_t per;    // points per chunk (multiple of `unit`)
};
// unit: the points one workgroup iteration takes (kChunkThreads binned, kPGroup packed)
SE3DS_HD ChunkGeom chunk_geom(int64_t m, int n, int unit) {
  int64_t cap = kMaxSinkBlocks / (n > 0 ? n : 1);
  cap = cap < 1 ? 1 : (cap > kMaxChunks ? kMaxChunks : cap);
  int64_t chunks = (m + kChunkPoints - 1) / kChunkPoints;
  chunks = chunks < 1 ? 1 : (chunks > cap ? cap : chunks);
  int64_t per = (m + chunks - 1) / chunks;
  per = (per + unit - 1) / unit * unit;
  if (per < unit) per = unit;
  chunks = (m + per - 1) / per;
  ChunkGeom g;
  g.chunks = (int)(chunks < 1 ? 1 : chunks);
  g.per = per;
  return g;
}
// upper bound of the resolve items: every tile has one band, and a tile with c > slice_records
// records has a power of two < 2 c / slice_records + 1 < 3 c / slice_records of them
SE3DS_HD int64_t resolve_items_max(int64_t nb, int64_t points, uint32_t slice_records) {
  return nb + 3 * ((points + slice_records - 1) / slice_records);
}

// ------------------------------------------------------------------ binned route
constexpr int kTileY = 16, kTileX = 128, kTilePx = kTileY * kTileX;
constexpr int kMaxTiles = 4096;      // per image (LDS histogram)
constexpr int kMaxBinChannels = 7;
constexpr uint32_t kSliceRecords = 8192;   // records per band workgroup aimed at
struct BinWs {
  uint32_t* tile_count;   // [nb]
  uint32_t* hist;         // [n][chunks][ntiles]: counts, then exclusive prefix over the chunks
  uint32_t* fpart2;       // [items][C] sink partials of the occluded points, per resolve item
  uint32_t* rec;          // [N*M][2 + C]: pixel inside the tile, z bits, feature bits
};
SE3DS_HD BinWs bin_ws(Carver& c, int n, int64_t m, int height, int width, int channels, uint32_t slice) {
  const size_t nb = (size_t)n * (size_t)(div_up(height, kTileY) * div_up(width, kTileX));
  const size_t pts = splat_points(n, m);
  const size_t chunks = (size_t)chunk_geom(m, n, kChunkThreads).chunks;
  const size_t items = (size_t)resolve_items_max((int64_t)nb, (int64_t)pts, slice);
  BinWs w;
  w.tile_count = c.take<uint32_t>(nb);
  w.hist = c.take<uint32_t>(nb * chunks);
  w.fpart2 = c.take<uint32_t>(items * channels);
  w.rec = c.take<uint32_t>(pts * (2 + channels));
  return w;
}
SE3DS_HD size_t bin_ws_bytes(int n, int64_t m, int height, int width, int channels, uint32_t slice) {
  Carver c{0, 0};
  bin_ws(c, n, m, height, width, channels, slice);
  return c.off;
}

// ------------------------------------------------------------------ packed route
constexpr int kPTileY = 16, kPTileX = 32, kPTilePx = kPTileY * kPTileX;   // 512 px
constexpr int kPThreads = 512, kPPts = 4;
constexpr int kPGroup = kPThreads * kPPts;     // points per workgroup iteration
constexpr uint32_t kPSlice = 4096;             // records per band workgroup aimed at
constexpr int kPMaxChannels = 3;
constexpr int kSinkSlots = 64;
struct PackWs {
  uint32_t* ctl;          // [8]: 0 colscan tickets, 1 promise violations, 2 items, 3 resolve tickets
  uint32_t* tile_count;   // [nb]
  uint32_t* tile_start;   // [nb + 1] exclusive prefix of tile_count (published by the permute pass)
  uint32_t* tile_lstart;  // [nb]  ... within the tile's group of 64
  uint32_t* tile_litem;   // [nb]  first resolve item of the tile within its group
  uint32_t* group_tot;    // [ngroups][2] records, items per group of 64 tiles
  uint32_t* items;        // [items_max]  tile | band << 20 | log2(bands) << 24
  uint32_t* hist;         // [n][chunks][ntiles]
  uint32_t* fpart2;       // [kSinkSlots][C] ordered max feature of the occluded points (slot = item % kSinkSlots)
  uint16_t* tile_pt;      // [n][mp]  tile of the point, kNoTile: no record
  uint64_t* rec_pt;       // [n][mp]  records in point order
  uint64_t* rec;          // [n * m]  records in tile order
  int64_t mp;             // padded points per image (chunks * per)
  uint32_t epoch;         // this call's promise epoch (kPromiseEpochWord)
};
constexpr int kCtlWords = 16;   // control words at the head of the packed and the sorted region
SE3DS_HD PackWs pack_ws(Carver& c, int n, int64_t m, int height, int width, uint32_t slice) {
  const size_t nb = (size_t)n * (size_t)(div_up(height, kPTileY) * div_up(width, kPTileX));
  const size_t pts = splat_points(n, m);
  const ChunkGeom g = chunk_geom(m, n, kPGroup);
  const size_t mp = (size_t)g.chunks * (size_t)g.per;
  const size_t items = (size_t)resolve_items_max((int64_t)nb, (int64_t)pts, slice);
  PackWs w;
  w.ctl = c.take<uint32_t>(kCtlWords);
  w.tile_count = c.take<uint32_t>(nb);
  w.tile_start = c.take<uint32_t>(nb + 1);
  w.tile_lstart = c.take<uint32_t>(nb);
  w.tile_litem = c.take<uint32_t>(nb);
  w.group_tot = c.take<uint32_t>(2 * (size_t)div_up((int64_t)nb, 64));
  w.items = c.take<uint32_t>(items);
  w.hist = c.take<uint32_t>(nb * (size_t)g.chunks);
  w.fpart2 = c.take<uint32_t>(kSinkSlots * kPMaxChannels);
  w.tile_pt = c.take<uint16_t>((size_t)n * mp);
  w.rec_pt = c.take<uint64_t>((size_t)n * mp);
  w.rec = c.take<uint64_t>(pts);
  w.mp = (int64_t)mp;
  w.epoch = 0u;
  return w;
}
SE3DS_HD size_t pack_ws_bytes(int n, int64_t m, int height, int width, uint32_t slice) {
  Carver c{0, 0};
  pack_ws(c, n, m, height, width, slice);
  return c.off;
}

// ------------------------------------------------------------------ sorted route
constexpr int kSMaxPx = 4096;            // pixels per supertile, upper bound (LDS tile of the resolve: 2 words per pixel)
constexpr int kSDefaultPx = 2048;        // ... default: one full row of a 1024 x 2048 target
constexpr int kSThreads = 512;           // S1 workgroup
constexpr int kSMaxSuper = 2048;         // supertiles per image (S1 LDS histogram, 11-bit field)
constexpr int kSMaxChunks = 4096;        // chunks per image (S2 LDS run prefix)
struct SortWs {
  uint32_t* ctl;      // [16]: 0 ticket, 1 promise violations (same slot as PackWs), 4.. pixel 0 (z, C feature words)
  uint32_t* fpart2;   // [kSinkSlots][C] ordered max feature of the occluded points
  uint32_t* runs;     // [n * nsuper][chunks]  offset << 16 | count
  uint64_t* rec;      // [n * chunks][chunk_pts]
  uint8_t* hi;        // [n * chunks][chunk_pts]
  int chunks;         // per image
  int chunk_pts;
  int cstride;        // row length of `runs`: 8 * ceil(chunks / 8), see run_slot()
  uint32_t epoch;     // this call's promise epoch (kPromiseEpochWord)
};
// Supertile = `rows` FULL-WIDTH image rows (rows x width <= 2048 pixels; images wider than 2048 are
// cut into column strips).  The shape matters: the pole rows of every SOURCE view (thousands of
// pixels looking the same way) land on a near-vertical line of the target, and 32 x 128 supertiles
// put 30 000 (random depth) to 86 000 (smooth room) records into the supertiles on that line against
// a mean of 8 000 -- one workgroup then runs 4-10x longer than the rest.  A line crosses a row
// once: full-row supertiles hold at most 1.35x (random) / 2.3x (room) the mean.
struct SortGeom {
  int pts, chunk_pts, chunks, super_w, rlog, super_x, super_y, nsuper, px;
};
// Geometry of one call.  Both kernels want TWO workgroups per CU (S1 is VALU- and S2 latency-bound: at one
// 8-wave workgroup per CU every barrier and every load round trip is exposed).  Round 5 sized both for
// the 4.2 M points of cfg5; at north_star's 512 x 1024 with two views that left 256 chunks and 256
// supertiles for 256 CUs and each kernel took 16.8 us for a quarter of the work that takes 34-39 us at
// 1024 x 2048 (profiles/r06_warp_512_*).  Now: points per thread = the largest of 16 / 8 / 4 that still
// gives kSTargetWgs chunks, pixels per supertile = the largest of 2048 / 1024 / 512 that gives as
// many supertiles (full image rows first, see above).
constexpr int kSTargetWgs = 512;
SE3DS_HD int sort_super_count(int height, int width, int super_px, int* super_w_out, int* rlog_out) {
  int super_w = width <= super_px ? width : super_px;
  if (width > super_w) {   // column strips of equal width (the last one may be ragged)
    const int strips = (int)div_up(width, super_w);
    super_w = (int)div_up(width, strips);
  }
  int rlog = 0;
  while ((2 << rlog) * super_w <= super_px && (1 << rlog) < height) ++rlog;
  if (super_w_out) *super_w_out = super_w;
  if (rlog_out) *rlog_out = rlog;
  return (int)(div_up(width, super_w) * div_up(height, 1 << rlog));
}
// pts_forced: 4 / 8 / 16 points per thread, px_forced: 256 .. 4096 pixels per supertile; 0 = choose
SE3DS_HD SortGeom sort_geom(int n, int64_t m, int height, int width, int pts_forced, int px_forced) {
  const int64_t mm = m > 0 ? m : 1;
  const int nn = n > 0 ? n : 1;
  SortGeom g;
  g.pts = pts_forced;
  if (!g.pts) {
    g.pts = 4;
    for (int pts = 16; pts > 4; pts >>= 1)
      if (div_up(mm, (int64_t)kSThreads * pts) * nn >= kSTargetWgs) {
        g.pts = pts;
        break;
      }
  }
  g.chunk_pts = kSThreads * g.pts;
  g.chunks = (int)div_up(mm, (int64_t)g.chunk_pts);
  int super_px = px_forced;
  if (!super_px) {
    super_px = kSDefaultPx;
    while (super_px > 512 && (int64_t)nn * sort_super_count(height, width, super_px, nullptr, nullptr) < kSTargetWgs)
      super_px >>= 1;
  }
  g.nsuper = sort_super_count(height, width, super_px, &g.super_w, &g.rlog);
  g.super_x = (int)div_up(width, g.super_w);
  g.super_y = (int)div_up(height, 1 << g.rlog);
  g.px = g.super_w << g.rlog;
  return g;
}
// nsuper: rows of the run table per image -- g.nsuper for a call, kSMaxSuper for the size
SE3DS_HD SortWs sort_ws(Carver& c, int n, const SortGeom& g, int nsuper) {
  SortWs w;
  w.ctl = c.take<uint32_t>(kCtlWords);
  w.fpart2 = c.take<uint32_t>(kSinkSlots * kPMaxChannels);
  w.cstride = 8 * (int)div_up(g.chunks, 8);
  w.runs = c.take<uint32_t>((size_t)n * nsuper * w.cstride);
  w.rec = c.take<uint64_t>((size_t)n * g.chunks * g.chunk_pts);
  w.hi = c.take<uint8_t>((size_t)n * g.chunks * g.chunk_pts);
  w.chunks = g.chunks;
  w.chunk_pts = g.chunk_pts;
  w.epoch = 0u;
  return w;
}
// (independent of the forced geometries: the worst case over every geometry a call may take --
// each points-per-thread choice with the run table at its longest, kSMaxSuper rows)
SE3DS_HD size_t sort_ws_bytes(int n, int64_t m, int height, int width) {
  size_t worst = 0;
  for (int pts = 4; pts <= 16; pts <<= 1) {
    Carver c{0, 0};
    sort_ws(c, n, sort_geom(n, m, height, width, pts, 256), kSMaxSuper);
    worst = c.off > worst ? c.off : worst;
  }
  return worst;
}

// what se3ds_splat_workspace_bytes reports: room for whichever route the call takes
SE3DS_HD size_t splat_workspace_bytes(int n, int64_t m, int height, int width, int channels,
                                      uint32_t bin_slice, uint32_t pack_slice) {
  size_t region = bin_ws_bytes(n, m, height, width, channels > 0 ? channels : 1, bin_slice);
  const size_t packed = pack_ws_bytes(n, m, height, width, pack_slice);
  const size_t sorted = sort_ws_bytes(n, m, height, width);
  if (packed > region) region = packed;
  if (sorted > region) region = sorted;
  return splat_route_region_offset(n, m) + region + 16;
}

// ------------------------------------------------------------------ the route of a call
enum class SplatRoute { Scatter, Binned, Packed, Sorted };
enum class SplatFeat { Float, Int32, Uint8 };
struct SplatSwitches {
  bool scatter;      // SE3DS_SPLAT_SCATTER is set: the global-atomic scatter version, always
  bool packed;       // SE3DS_SPLAT_PACKED is not 0: 8-byte records where the features allow them
  int sort_mode;     // SE3DS_SPLAT_SORT: 0 off, 1 = when the image has enough supertiles to fill the chip, 2 = always
  int pts, superpx;  // SE3DS_SPLAT_PTS, SE3DS_SPLAT_SUPERPX: forced sort geometry (0 = choose)
};
struct SplatChoice {
  SplatRoute route;
  SortGeom sort;     // of a Sorted call; zeros otherwise
};
// Every gate, once.  8-byte records (packed, sorted) need features of valid points that are bytes by
// type (uint8) or by the caller's promise (int32 | SE3DS_FEAT_BYTE_RANGE), <= 3 channels and a
// non-negative output void; every binning route needs n * m < 2^31 records and exact row division
// (height * width^2 < 2^40); wider features and larger tile grids take the scatter version.
SE3DS_HD SplatChoice splat_route(SplatFeat kind, bool byte_range, int n, int64_t m, int channels,
                                 int height, int width, float output_void, const SplatSwitches& sw) {
  SplatChoice ch = {SplatRoute::Scatter, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
  if (sw.scatter || m <= 0 || (int64_t)n * m >= ((int64_t)1 << 31) ||
      (int64_t)height * width * width >= ((int64_t)1 << 40))
    return ch;
  const bool bytes = sw.packed && channels <= kPMaxChannels && output_void >= 0.0f &&
                     (kind == SplatFeat::Uint8 || (kind == SplatFeat::Int32 && byte_range));
  if (bytes && sw.sort_mode != 0) {
    const SortGeom sg = sort_geom(n, m, height, width, sw.pts, sw.superpx);
    if (sg.nsuper <= kSMaxSuper && sg.chunks <= kSMaxChunks && (int64_t)sg.chunks * n <= kMaxSinkBlocks &&
        (int64_t)n * sg.nsuper < ((int64_t)1 << 24) && (sw.sort_mode == 2 || (int64_t)n * sg.nsuper >= 128)) {
      ch.route = SplatRoute::Sorted;
      ch.sort = sg;
      return ch;
    }
  }
  const int64_t ptiles = div_up(height, kPTileY) * div_up(width, kPTileX);
  const int64_t ntiles = div_up(height, kTileY) * div_up(width, kTileX);
  if (bytes && ptiles <= kMaxTiles && (int64_t)n * ptiles < ((int64_t)1 << 20))
    ch.route = SplatRoute::Packed;
  else if (channels <= kMaxBinChannels && ntiles <= kMaxTiles)
    ch.route = SplatRoute::Binned;
  return ch;
}

}  // namespace
}  // namespace se3ds
