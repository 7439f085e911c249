// The host arithmetic of the warp's splat (se3ds_amd/csrc/splat_layout.h) as a plain host program,
// for the sanitizers: the walks that size and carve the splat's workspaces, the chunk geometry and the
// choice of the route.  Built and run by tests/test_splat_layout_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -Werror
//       tools/splat_layout_host_check.cpp -o splat_layout_host_check && ./splat_layout_host_check
//
// Sweep: n in {1, 2, 8} x m in {0, 1, 3, 50, 4099, 8192, 70001, 4194304, 33554432} x height x width in
// {8x16, 48x96, 256x512, 512x1024, 1024x2048} x channels in {1, 2, 3, 5, 7, 9, 60} = 945 cases.  Per case:
//   (a) every workspace (header + idx + z, binned, packed, sorted) is carved from a heap block of
//       exactly the size its walk reports: every array starts 16-byte aligned (z excepted: it follows
//       idx unpadded, as it always did), the arrays are in order and disjoint, the last one ends inside
//       the block, and the first and last byte of every array are written, so a walk that leaves the
//       block is a sanitizer report.  Above 256 MiB the walk starts at address 0 and is checked
//       arithmetically only.  The sorted route: every geometry sort_geom returns with points per thread
//       forced to 4 / 8 / 16 or chosen and supertiles forced to 256 .. 4096 pixels or chosen (those a
//       call can take: at most kSMaxSuper supertiles), in a block of sort_ws_bytes;
//   (b) the sizes and every array's offset equal the yardstick: the closed-form sums and the
//       `p += align16(...)` chains geom.hip held before the walks (old_* below, verbatim);
//   (c) chunk_geom(m, n, unit) equals the two functions it replaced, for both units;
// and once, (d): splat_route on a pinned table of (inputs -> route, points per thread, supertile width,
// log2 rows, supertiles, chunks), recorded from the ladder launch_splat held before splat_route.
// `splat_layout_host_check corrupt` gives the walks half as many resolve items as the yardstick counts
// (one array of the binned and of the packed workspace is then too short): exit status 1.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../se3ds_amd/csrc/splat_layout.h"

using namespace se3ds;

static long long g_cases = 0;
static bool g_corrupt = false;
constexpr size_t kRealBlockMax = (size_t)256 << 20;

// ---------------------------------------------------------------- the yardstick (geom.hip before the walks)
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static ChunkGeom old_chunk_geom(int64_t m, int n) {
  int64_t cap = kMaxSinkBlocks / (n > 0 ? n : 1);
  cap = cap < 1 ? 1 : (cap > kMaxChunks ? kMaxChunks : cap);
  int64_t chunks = (m + kChunkPoints - 1) / kChunkPoints;
  chunks = chunks < 1 ? 1 : (chunks > cap ? cap : chunks);
  int64_t per = (m + chunks - 1) / chunks;
  per = (per + kChunkThreads - 1) / kChunkThreads * kChunkThreads;
  if (per < kChunkThreads) per = kChunkThreads;
  chunks = (m + per - 1) / per;
  ChunkGeom g;
  g.chunks = (int)(chunks < 1 ? 1 : chunks);
  g.per = per;
  return g;
}
static ChunkGeom old_pack_geom(int64_t m, int n) {
  int64_t cap = kMaxSinkBlocks / (n > 0 ? n : 1);
  cap = cap < 1 ? 1 : (cap > kMaxChunks ? kMaxChunks : cap);
  int64_t chunks = (m + kChunkPoints - 1) / kChunkPoints;
  chunks = chunks < 1 ? 1 : (chunks > cap ? cap : chunks);
  int64_t per = (m + chunks - 1) / chunks;
  per = (per + kPGroup - 1) / kPGroup * kPGroup;
  if (per < kPGroup) per = kPGroup;
  chunks = (m + per - 1) / per;
  ChunkGeom g;
  g.chunks = (int)(chunks < 1 ? 1 : chunks);
  g.per = per;
  return g;
}
static size_t old_splat_hdr_bytes() {
  return 256 + sizeof(uint32_t) * (size_t)kMaxSinkBlocks * (size_t)(1 + kMaxSplatChannels);
}
static size_t old_bin_ws_bytes(int n, int64_t m, int height, int width, int channels, uint32_t slice) {
  const size_t ntiles = (size_t)ceil_div(height, kTileY) * ceil_div(width, kTileX);
  const size_t nb = (size_t)n * ntiles;
  const size_t pts = (size_t)n * (size_t)(m > 0 ? m : 0);
  const size_t chunks = (size_t)old_chunk_geom(m, n).chunks;
  const size_t items = (size_t)resolve_items_max((int64_t)nb, (int64_t)pts, slice);
  return align16(4 * nb) + align16(4 * nb * chunks) +
         align16(4 * items * channels) + align16(4 * pts * (2 + channels));
}
static size_t old_pack_ws_bytes(int n, int64_t m, int height, int width, uint32_t slice) {
  const size_t ntiles = (size_t)ceil_div(height, kPTileY) * ceil_div(width, kPTileX);
  const size_t nb = (size_t)n * ntiles;
  const ChunkGeom g = old_pack_geom(m, n);
  const size_t mp = (size_t)g.chunks * (size_t)g.per;
  const size_t items = (size_t)resolve_items_max((int64_t)nb, (int64_t)n * (m > 0 ? m : 0), slice);
  return 64 + align16(4 * nb) + align16(4 * (nb + 1)) + 2 * align16(4 * nb) +
         align16(8 * (size_t)ceil_div(nb, 64)) + align16(4 * items) +
         align16(4 * nb * (size_t)g.chunks) + align16(4 * kSinkSlots * kPMaxChannels) +
         align16(2 * (size_t)n * mp) + align16(8 * (size_t)n * mp) +
         align16(8 * (size_t)n * (size_t)(m > 0 ? m : 0));
}
static size_t old_sort_ws_bytes(int n, int64_t m, int height, int width) {
  size_t worst = 0;
  for (int pts = 4; pts <= 16; pts <<= 1) {
    const SortGeom g = sort_geom(n, m, height, width, pts, 256);   // (256-pixel supertiles: the longest run table)
    const size_t b = 64 + align16(4 * kSinkSlots * kPMaxChannels) +
                     align16(4 * (size_t)n * kSMaxSuper * (size_t)(8 * ceil_div(g.chunks, 8))) +
                     align16(8 * (size_t)n * g.chunks * g.chunk_pts) +
                     align16((size_t)n * g.chunks * g.chunk_pts);
    worst = b > worst ? b : worst;
  }
  return worst;
}
static size_t old_route_region_offset(int n, int64_t m) {
  const size_t base = old_splat_hdr_bytes() +
                      (sizeof(int32_t) + sizeof(float)) * (size_t)n * (size_t)(m > 0 ? m : 0);
  return align16(base);
}
static size_t old_splat_workspace_bytes(int n, int64_t m, int height, int width, int channels, uint32_t bin_slice,
                                        uint32_t pack_slice) {
  const int c = channels > 0 ? channels : 1;
  const size_t three_pass = old_bin_ws_bytes(n, m, height, width, c, bin_slice);
  const size_t packed = old_pack_ws_bytes(n, m, height, width, pack_slice);
  const size_t sorted = old_sort_ws_bytes(n, m, height, width);
  size_t bins = three_pass;
  if (packed > bins) bins = packed;
  if (sorted > bins) bins = sorted;
  return old_route_region_offset(n, m) + bins + 16;
}

// one array of a workspace: where the old carve put it (offset) and the bytes its element count needs
struct Want {
  size_t offset, bytes;
};
// the old `w.x = (T*)p; p += align16(bytes);` chains
struct OldChain {
  size_t p = 0;
  std::vector<Want> arrays;
  void put(size_t bytes) {
    arrays.push_back({p, bytes});
    p += align16(bytes);
  }
};
static std::vector<Want> old_splat_arrays(int n, int64_t m) {   // carve_ws
  const size_t pts = (size_t)n * (size_t)m;
  const size_t q = old_splat_hdr_bytes();
  return {{0, 16}, {16, 4 * (size_t)kMaxSplatChannels}, {256, 4 * (size_t)kMaxSinkBlocks},
          {256 + 4 * (size_t)kMaxSinkBlocks, 4 * (size_t)kMaxSinkBlocks * kMaxSplatChannels},
          {q, sizeof(int32_t) * pts}, {q + sizeof(int32_t) * pts, sizeof(float) * pts}};
}
static std::vector<Want> old_bin_arrays(int n, int64_t m, int height, int width, int channels, uint32_t slice) {
  const size_t ntiles = (size_t)ceil_div(height, kTileY) * ceil_div(width, kTileX);
  const size_t nb = (size_t)n * ntiles;
  const size_t chunks = (size_t)old_chunk_geom(m, n).chunks;
  const size_t items = (size_t)resolve_items_max((int64_t)nb, (int64_t)n * (m > 0 ? m : 0), slice);
  OldChain c;
  c.put(4 * nb);
  c.put(4 * nb * chunks);
  c.put(4 * items * channels);
  c.put(4 * (size_t)n * (size_t)m * (2 + channels));   // rec [N*M][2 + C]
  return c.arrays;
}
static std::vector<Want> old_pack_arrays(int n, int64_t m, int height, int width, uint32_t slice) {
  const size_t ntiles = (size_t)ceil_div(height, kPTileY) * ceil_div(width, kPTileX);
  const size_t nb = (size_t)n * ntiles;
  const ChunkGeom g = old_pack_geom(m, n);
  const size_t mp = (size_t)g.chunks * (size_t)g.per;
  const size_t items = (size_t)resolve_items_max((int64_t)nb, (int64_t)n * (m > 0 ? m : 0), slice);
  OldChain c;
  c.put(64);
  c.put(4 * nb);
  c.put(4 * (nb + 1));
  c.put(4 * nb);
  c.put(4 * nb);
  c.put(8 * (size_t)ceil_div(nb, 64));
  c.put(4 * items);
  c.put(4 * nb * (size_t)g.chunks);
  c.put(4 * kSinkSlots * kPMaxChannels);
  c.put(2 * (size_t)n * mp);
  c.put(8 * (size_t)n * mp);
  c.put(8 * (size_t)n * (size_t)m);   // rec [n * m]
  return c.arrays;
}
static std::vector<Want> old_sort_arrays(int n, const SortGeom& g) {
  OldChain c;
  c.put(64);
  c.put(4 * kSinkSlots * kPMaxChannels);
  const int cstride = 8 * (int)ceil_div(g.chunks, 8);
  c.put(4 * (size_t)n * g.nsuper * cstride);
  c.put(8 * (size_t)n * g.chunks * g.chunk_pts);
  c.put((size_t)n * g.chunks * g.chunk_pts);   // hi [n * chunks][chunk_pts]
  return c.arrays;
}

// ---------------------------------------------------------------- (a) + (b) for one workspace
static bool fail(const std::string& what, const char* array, long long got, long long want) {
  fprintf(stderr, "%s: %s: got %lld, expected %lld\n", what.c_str(), array, got, want);
  return false;
}

// a heap block of exactly `bytes`; above kRealBlockMax none, and the walk starts at address 0
struct Block {
  size_t bytes;
  std::unique_ptr<char[]> mem;
  explicit Block(size_t b) : bytes(b), mem(b <= kRealBlockMax ? new char[b ? b : 1] : nullptr) {}
};
// `carve` walks the block and returns the arrays' addresses in the order of the workspace struct.
// unaligned: index of the one array that may start off a 16-byte boundary (-1: none).
template <typename Carve>
static bool check_workspace(const std::string& what, const Block& block, const std::vector<Want>& want, Carve carve,
                            int unaligned = -1) {
  static const char* const kNth[] = {"array 0", "array 1", "array 2", "array 3", "array 4", "array 5", "array 6",
                                     "array 7", "array 8", "array 9", "array 10", "array 11"};
  const size_t bytes = block.bytes;
  const bool real = block.mem != nullptr;
  const uintptr_t base = (uintptr_t)block.mem.get();
  if (base % 16) return fail(what, "block alignment", (long long)(base % 16), 0);
  Carver c{base, 0};
  const std::vector<uintptr_t> at = carve(c);
  if (at.size() != want.size()) return fail(what, "arrays", (long long)at.size(), (long long)want.size());
  size_t end = 0;
  for (size_t k = 0; k < at.size(); ++k) {
    const size_t off = at[k] - base;
    if (off != want[k].offset) return fail(what, kNth[k], (long long)off, (long long)want[k].offset);
    if ((int)k != unaligned && off % 16) return fail(what, kNth[k], (long long)(off % 16), 0);
    if (off < end) return fail(what, kNth[k], (long long)off, (long long)end);   // in order, disjoint
    end = off + want[k].bytes;
    if (end > bytes) return fail(what, kNth[k], (long long)end, (long long)bytes);
    if (real && want[k].bytes) {
      volatile char* p = (volatile char*)at[k];
      p[0] = (char)k;
      p[want[k].bytes - 1] = (char)k;
    }
  }
  if (c.off > bytes) return fail(what, "end of the walk", (long long)c.off, (long long)bytes);
  return true;
}

static bool check_case(int n, int64_t m, int height, int width, int channels) {
  char tag[96];
  snprintf(tag, sizeof tag, "n %d m %lld %dx%d c %d", n, (long long)m, height, width, channels);
  const std::string t(tag);
  // what the walks are given; `corrupt` doubles the slices behind the yardstick's back
  const uint32_t bin_slice = kSliceRecords * (g_corrupt ? 2u : 1u), pack_slice = kPSlice * (g_corrupt ? 2u : 1u);

  // header, idx, z
  const size_t region = splat_route_region_offset(n, m);
  if (region != old_route_region_offset(n, m))
    return fail(t, "region offset", (long long)region, (long long)old_route_region_offset(n, m));
  if (!check_workspace(t + " SplatWs", Block(region), old_splat_arrays(n, m), [&](Carver& c) {
        const SplatWs w = splat_ws(c, n, m);
        return std::vector<uintptr_t>{(uintptr_t)w.sink_z, (uintptr_t)w.sink_feat, (uintptr_t)w.zpart,
                                      (uintptr_t)w.fpart, (uintptr_t)w.idx, (uintptr_t)w.z};
      }, 5))
    return false;
  {   // the launchers' two calls agree with the one walk
    const SplatWs w = carve_ws(nullptr, n, m);
    const Carver r = route_carver(nullptr, n, m);
    if ((uintptr_t)w.idx != old_splat_hdr_bytes() || r.base != 0 || r.off != region)
      return fail(t, "carve_ws / route_carver", (long long)r.off, (long long)region);
  }

  // binned
  const size_t bin_bytes = bin_ws_bytes(n, m, height, width, channels, bin_slice);
  if (bin_bytes != old_bin_ws_bytes(n, m, height, width, channels, kSliceRecords))
    return fail(t, "bin_ws_bytes", (long long)bin_bytes,
                (long long)old_bin_ws_bytes(n, m, height, width, channels, kSliceRecords));
  if (!check_workspace(t + " BinWs", Block(bin_bytes), old_bin_arrays(n, m, height, width, channels, kSliceRecords), [&](Carver& c) {
        const BinWs w = bin_ws(c, n, m, height, width, channels, bin_slice);
        return std::vector<uintptr_t>{(uintptr_t)w.tile_count, (uintptr_t)w.hist, (uintptr_t)w.fpart2, (uintptr_t)w.rec};
      }))
    return false;

  // packed
  const size_t pack_bytes = pack_ws_bytes(n, m, height, width, pack_slice);
  if (pack_bytes != old_pack_ws_bytes(n, m, height, width, kPSlice))
    return fail(t, "pack_ws_bytes", (long long)pack_bytes, (long long)old_pack_ws_bytes(n, m, height, width, kPSlice));
  const ChunkGeom pg = old_pack_geom(m, n);
  int64_t mp = 0;
  if (!check_workspace(t + " PackWs", Block(pack_bytes), old_pack_arrays(n, m, height, width, kPSlice), [&](Carver& c) {
        const PackWs w = pack_ws(c, n, m, height, width, pack_slice);
        mp = w.mp;
        return std::vector<uintptr_t>{(uintptr_t)w.ctl, (uintptr_t)w.tile_count, (uintptr_t)w.tile_start,
                                      (uintptr_t)w.tile_lstart, (uintptr_t)w.tile_litem, (uintptr_t)w.group_tot,
                                      (uintptr_t)w.items, (uintptr_t)w.hist, (uintptr_t)w.fpart2,
                                      (uintptr_t)w.tile_pt, (uintptr_t)w.rec_pt, (uintptr_t)w.rec};
      }))
    return false;
  if (mp != (int64_t)pg.chunks * pg.per) return fail(t, "PackWs.mp", mp, (int64_t)pg.chunks * pg.per);

  // sorted: the size, then every geometry a call can take inside a block of that size
  const size_t sort_bytes = sort_ws_bytes(n, m, height, width);
  if (sort_bytes != old_sort_ws_bytes(n, m, height, width))
    return fail(t, "sort_ws_bytes", (long long)sort_bytes, (long long)old_sort_ws_bytes(n, m, height, width));
  const Block sort_block(sort_bytes);
  for (int pts : {0, 4, 8, 16})
    for (int px : {0, 256, 512, 1024, 2048, 4096}) {
      const SortGeom g = sort_geom(n, m, height, width, pts, px);
      if (g.nsuper > kSMaxSuper) continue;   // (splat_route never takes it)
      SortWs w = {};
      if (!check_workspace(t + " SortWs pts " + std::to_string(pts) + " px " + std::to_string(px), sort_block,
                           old_sort_arrays(n, g), [&](Carver& c) {
            w = sort_ws(c, n, g, g.nsuper);
            return std::vector<uintptr_t>{(uintptr_t)w.ctl, (uintptr_t)w.fpart2, (uintptr_t)w.runs,
                                          (uintptr_t)w.rec, (uintptr_t)w.hi};
          }))
        return false;
      if (w.chunks != g.chunks || w.chunk_pts != g.chunk_pts || w.cstride != 8 * (int)ceil_div(g.chunks, 8) || w.epoch != 0u)
        return fail(t, "SortWs scalars", w.cstride, 8 * ceil_div(g.chunks, 8));
    }

  // the reported total
  const size_t total = splat_workspace_bytes(n, m, height, width, channels, bin_slice, pack_slice);
  const size_t old_total = old_splat_workspace_bytes(n, m, height, width, channels, kSliceRecords, kPSlice);
  if (total != old_total) return fail(t, "splat_workspace_bytes", (long long)total, (long long)old_total);

  // (c) one chunk geometry for both units
  const ChunkGeom a = chunk_geom(m, n, kChunkThreads), a0 = old_chunk_geom(m, n);
  const ChunkGeom b = chunk_geom(m, n, kPGroup);
  if (a.chunks != a0.chunks || a.per != a0.per) return fail(t, "chunk_geom(kChunkThreads)", a.per, a0.per);
  if (b.chunks != pg.chunks || b.per != pg.per) return fail(t, "chunk_geom(kPGroup)", b.per, pg.per);
  ++g_cases;
  return true;
}

// ---------------------------------------------------------------- (d) the route
struct RouteRow {
  SplatFeat kind;
  int byte_range, n;
  long long m;
  int channels, height, width;
  float output_void;
  SplatSwitches sw;   // scatter, packed, sort_mode, pts, superpx
  SplatRoute route;
  int pts, super_w, rlog, nsuper, chunks;
};
static bool check_routes() {
  const SplatFeat F = SplatFeat::Float, I = SplatFeat::Int32, U = SplatFeat::Uint8;
  static const RouteRow rows[] = {
      // the bench's and the configurations' shapes: two views, RGB (promised int32) and semantics (uint8)
      {I, 1, 1, 1048576, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 4, 1024, 0, 512, 512},
      {U, 0, 1, 1048576, 1, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 4, 1024, 0, 512, 512},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 4, 1024, 0, 512, 512},
      {I, 1, 8, 1048576, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 16, 1024, 1, 256, 128},
      {U, 0, 8, 1048576, 1, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 16, 1024, 1, 256, 128},
      {U, 0, 8, 1048576, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 16, 1024, 1, 256, 128},
      {I, 1, 1, 4194304, 3, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 16, 2048, 0, 1024, 512},
      {U, 0, 1, 4194304, 1, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 16, 2048, 0, 1024, 512},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 16, 2048, 0, 1024, 512},
      {I, 1, 8, 4194304, 3, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 8, 4194304, 1, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 8, 4194304, 3, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      // tests/test_warp_gpu.py: the wide-feature, edge-case and packed-variant shapes
      {I, 0, 2, 6000, 9, 32, 64, -1.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {I, 1, 2, 6000, 9, 32, 64, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 0, 1, 8, 16, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {I, 1, 2, 50, 3, 8, 16, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 5000, 1, 8, 16, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 1, 1, 70001, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 4099, 1, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 1, 1, 12345, 2, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 8192, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 0, 1, 30000, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 1, 5000, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      // ... the bit-exact projection shapes (n, h, views), default switches and the child-process variants
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 4, 512, 0, 256, 64},
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, true, 2, 16, 0}, SplatRoute::Sorted, 16, 32, 4, 1, 1},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, true, 2, 16, 0}, SplatRoute::Sorted, 16, 64, 3, 4, 1},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, true, 2, 16, 0}, SplatRoute::Sorted, 16, 256, 1, 64, 8},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, true, 2, 16, 0}, SplatRoute::Sorted, 16, 512, 0, 256, 16},
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, true, 2, 8, 0}, SplatRoute::Sorted, 8, 32, 4, 1, 1},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, true, 2, 8, 0}, SplatRoute::Sorted, 8, 64, 3, 4, 1},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, true, 2, 8, 0}, SplatRoute::Sorted, 8, 256, 1, 64, 16},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, true, 2, 8, 0}, SplatRoute::Sorted, 8, 512, 0, 256, 32},
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, true, 2, 4, 0}, SplatRoute::Sorted, 4, 32, 4, 1, 1},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, true, 2, 4, 0}, SplatRoute::Sorted, 4, 64, 3, 4, 2},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, true, 2, 4, 0}, SplatRoute::Sorted, 4, 256, 1, 64, 32},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, true, 2, 4, 0}, SplatRoute::Sorted, 4, 512, 0, 256, 64},
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, true, 2, 0, 4096}, SplatRoute::Sorted, 4, 32, 4, 1, 1},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, true, 2, 0, 4096}, SplatRoute::Sorted, 4, 64, 5, 1, 2},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, true, 2, 0, 4096}, SplatRoute::Sorted, 4, 256, 4, 8, 32},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, true, 2, 0, 4096}, SplatRoute::Sorted, 4, 512, 3, 32, 64},
      {I, 1, 1, 512, 3, 16, 32, 0.0f, {false, true, 2, 0, 512}, SplatRoute::Sorted, 4, 32, 4, 1, 1},
      {I, 1, 2, 4096, 3, 32, 64, 0.0f, {false, true, 2, 0, 512}, SplatRoute::Sorted, 4, 64, 3, 4, 2},
      {I, 1, 1, 65536, 3, 128, 256, 0.0f, {false, true, 2, 0, 512}, SplatRoute::Sorted, 4, 256, 1, 64, 32},
      {I, 1, 1, 131072, 3, 256, 512, 0.0f, {false, true, 2, 0, 512}, SplatRoute::Sorted, 4, 512, 0, 256, 64},
      // float features, int32 without the promise, 5 / 7 / 9 channels
      {F, 0, 2, 4099, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {F, 0, 1, 9216, 1, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 5, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 2, 4099, 5, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 2, 4099, 5, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 5, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 7, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 2, 4099, 7, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 2, 4099, 7, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 7, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 9, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {I, 1, 2, 4099, 9, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 2, 4099, 9, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 9, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {F, 0, 1, 1048576, 1, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 5, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 2, 4099, 5, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 2, 4099, 5, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 5, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 7, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 2, 4099, 7, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 2, 4099, 7, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 7, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 9, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {I, 1, 2, 4099, 9, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 2, 4099, 9, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 9, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      // a negative output void, no points
      {U, 0, 1, 9216, 3, 48, 96, -1.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 1, 9216, 3, 48, 96, -1.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 1, 0, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {F, 0, 1, 0, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 1048576, 3, 512, 1024, -1.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 1, 1, 1048576, 3, 512, 1024, -1.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 1, 0, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {F, 0, 1, 0, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      // each switch off, SE3DS_SPLAT_SORT=2, forced geometries at full size
      {U, 0, 1, 9216, 3, 48, 96, 0.0f, {true, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 9216, 3, 48, 96, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 1, 9216, 3, 48, 96, 0.0f, {false, true, 0, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 9216, 3, 48, 96, 0.0f, {false, true, 2, 0, 0}, SplatRoute::Sorted, 4, 96, 2, 12, 5},
      {F, 0, 1, 9216, 3, 48, 96, 0.0f, {true, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 9216, 3, 48, 96, 0.0f, {false, true, 1, 4, 256}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 9216, 3, 48, 96, 0.0f, {false, true, 1, 16, 4096}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {true, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {false, true, 0, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {false, true, 2, 0, 0}, SplatRoute::Sorted, 4, 1024, 0, 512, 512},
      {F, 0, 1, 1048576, 3, 512, 1024, 0.0f, {true, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {false, true, 1, 4, 256}, SplatRoute::Sorted, 4, 256, 0, 2048, 512},
      {U, 0, 1, 1048576, 3, 512, 1024, 0.0f, {false, true, 1, 16, 4096}, SplatRoute::Sorted, 16, 1024, 2, 128, 128},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {true, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {false, false, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {false, true, 0, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {false, true, 2, 0, 0}, SplatRoute::Sorted, 16, 2048, 0, 1024, 512},
      {F, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {true, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {false, true, 1, 4, 256}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 1024, 2048, 0.0f, {false, true, 1, 16, 4096}, SplatRoute::Sorted, 16, 2048, 1, 512, 512},
      // the limits: too many chunks for the sorted route, a tile grid too large for any binning, n * m at 2^31
      {U, 0, 8, 33554432, 3, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 33554432, 3, 1024, 2048, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 2048, 4096, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 1, 4194304, 3, 2048, 4096, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {U, 0, 1, 4194304, 3, 4096, 8192, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      {U, 0, 64, 33554432, 3, 512, 1024, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
      // tests/test_warp_gpu.py::test_splat_exact_size_workspace_guard
      {U, 0, 1, 20001, 3, 256, 512, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 4, 512, 0, 256, 10},
      {U, 0, 2, 4099, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {I, 1, 1, 20001, 3, 256, 512, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Sorted, 4, 512, 0, 256, 10},
      {I, 1, 2, 4099, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Packed, 0, 0, 0, 0, 0},
      {F, 0, 2, 4099, 3, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 4099, 5, 48, 96, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Binned, 0, 0, 0, 0, 0},
      {I, 0, 2, 6000, 9, 32, 64, 0.0f, {false, true, 1, 0, 0}, SplatRoute::Scatter, 0, 0, 0, 0, 0},
  };
  for (const RouteRow& r : rows) {
    const SplatChoice ch = splat_route(r.kind, r.byte_range != 0, r.n, r.m, r.channels, r.height, r.width,
                                       r.output_void, r.sw);
    char tag[128];
    snprintf(tag, sizeof tag, "route of kind %d promise %d n %d m %lld c %d %dx%d void %g switches %d %d %d %d %d",
             (int)r.kind, r.byte_range, r.n, r.m, r.channels, r.height, r.width, r.output_void, (int)r.sw.scatter,
             (int)r.sw.packed, r.sw.sort_mode, r.sw.pts, r.sw.superpx);
    if (ch.route != r.route) return fail(tag, "route", (long long)ch.route, (long long)r.route);
    const int got[5] = {ch.sort.pts, ch.sort.super_w, ch.sort.rlog, ch.sort.nsuper, ch.sort.chunks};
    const int want[5] = {r.pts, r.super_w, r.rlog, r.nsuper, r.chunks};
    static const char* const kField[5] = {"pts", "super_w", "rlog", "nsuper", "chunks"};
    for (int k = 0; k < 5; ++k)
      if (got[k] != want[k]) return fail(tag, kField[k], got[k], want[k]);
    if (ch.route == SplatRoute::Sorted &&
        (ch.sort.chunk_pts != kSThreads * ch.sort.pts || ch.sort.px != ch.sort.super_w << ch.sort.rlog ||
         ch.sort.super_x * ch.sort.super_y != ch.sort.nsuper))
      return fail(tag, "derived geometry", ch.sort.px, ch.sort.super_w << ch.sort.rlog);
  }
  return true;
}

static bool sweep() {
  const int heights[] = {8, 48, 256, 512, 1024};
  for (int n : {1, 2, 8})
    for (long long m : {0LL, 1LL, 3LL, 50LL, 4099LL, 8192LL, 70001LL, 4194304LL, 33554432LL})
      for (int h : heights)
        for (int c : {1, 2, 3, 5, 7, 9, 60})
          if (!check_case(n, m, h, 2 * h, c)) return false;
  return check_routes();
}

int main(int argc, char** argv) {
  const std::string mode = argc >= 2 ? argv[1] : "";
  if (mode == "corrupt" && argc == 2) {
    g_corrupt = true;
    if (sweep()) {
      fprintf(stderr, "walks with too few resolve items went unnoticed\n");
      return 3;
    }
    return 1;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: %s [corrupt]\n", argv[0]);
    return 2;
  }
  if (!sweep()) return 1;
  printf("splat_layout_host_check: %lld cases OK\n", g_cases);
  return 0;
}
