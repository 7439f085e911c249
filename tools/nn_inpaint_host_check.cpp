// The nearest-site transform of nearest_neighbor_inpaint (se3ds_amd/csrc/nn_inpaint_core.h) as a
// plain host program, for the sanitizers: the row pass and the column pass run serially with the
// functions the kernels of semantic.hip call (the scans' seeds and joins, pick_in_row, nearest_site),
// segment by segment with a carry as the row kernel walks a wide row.  Built and run by
// tests/test_semantic_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/nn_inpaint_host_check.cpp -o nn_inpaint_host_check && ./nn_inpaint_host_check
//
// Cases: (H, W) of {(1,1), (1,9), (7,5), (13,17), (16,33), (3,63), (3,64), (3,65), (2,S-1), (2,S),
// (2,S+1), (3,2S+5), (T+1,70)} (S = kRowSegment, T = kColTileRows) x the three pixel kinds x void
// shares 0.02, 0.5, 0.97 with seeded patterns, plus per shape an image that is all void, one without a
// void pixel and one whose every second row is void; then the twelve-point tie ring, peeled winner by
// winner.  Image, table, output and index plane are heap allocations of exactly their size, so a read
// or write past a row or an image is a sanitizer report.  The yardstick is the pairwise definition
// written below: all sites in row-major order, the first minimum wins.
// `nn_inpaint_host_check corrupt` flips one table entry between the passes: exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../se3ds_amd/csrc/nn_inpaint_core.h"

using namespace se3ds::nn_inpaint;

static uint32_t g_rng = 2463534242u;
static uint32_t next_u32() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

static uint32_t void_bits_of(int kind) {
  if (kind == kKindU8) return 255u;
  if (kind == kKindI32) return 0u;
  const float v = 0.0f;   // -0.0 is void as well, a NaN is not
  uint32_t b;
  memcpy(&b, &v, sizeof b);
  return b;
}

// a non-void value that names its pixel
static uint32_t site_bits(int kind, int flat) {
  if (kind == kKindU8) return (uint32_t)(flat % 255);
  if (kind == kKindI32) return (uint32_t)(1 + flat);
  if (flat % 7 == 3) return 0x7fc00001u;   // a NaN: never void
  const float v = (float)(1 + flat);
  uint32_t b;
  memcpy(&b, &v, sizeof b);
  return b;
}

static uint32_t a_void(int kind, int flat) {
  if (kind == kKindF32 && (flat & 1)) return 0x80000000u;   // -0.0
  return void_bits_of(kind);
}

// the row kernel's walk: segments left to right with a carry, then right to left
static void row_pass(const uint32_t* image, uint32_t void_bits, int kind, int h, int w, Entry* table) {
  const int segments = (w + kRowSegment - 1) / kRowSegment;
  for (int r = 0; r < h; ++r) {
    const uint32_t* row = image + (size_t)r * w;
    Entry* out = table + (size_t)r * w;
    int carry = kNoSite;
    for (int seg = 0; seg < segments; ++seg) {
      int run = carry;
      for (int x = seg * kRowSegment; x < (seg + 1) * kRowSegment && x < w; ++x) {
        run = left_join(run, left_seed(!is_void(row[x], void_bits, kind), x));
        out[x] = (Entry)run;
      }
      carry = run;
    }
    carry = kFarRight;
    for (int seg = segments - 1; seg >= 0; --seg) {
      int run = carry;
      const int end = (seg + 1) * kRowSegment < w ? (seg + 1) * kRowSegment : w;
      for (int x = end - 1; x >= seg * kRowSegment; --x) {
        run = right_join(run, right_seed(!is_void(row[x], void_bits, kind), x));
        out[x] = (Entry)pick_in_row(x, out[x], run);
      }
      carry = run;
    }
  }
}

static void column_pass(const uint32_t* image, uint32_t void_bits, int kind, int h, int w, const Entry* table,
                        uint32_t* out, int32_t* indices) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int32_t src = y * w + x;
      uint32_t bits = image[src];
      if (is_void(bits, void_bits, kind)) {
        src = nearest_site(table, h, w, y, x);
        if (src != kNoSite) bits = image[src];
      }
      out[(size_t)y * w + x] = bits;
      indices[(size_t)y * w + x] = src;
    }
}

// the definition: every site in row-major order, int64 distances, the first minimum wins
static int32_t pairwise(const uint32_t* image, uint32_t void_bits, int kind, int h, int w, int y, int x) {
  int64_t best = -1;
  int32_t arg = -1;
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < w; ++c) {
      if (is_void(image[(size_t)r * w + c], void_bits, kind)) continue;
      const int64_t d = (int64_t)(r - y) * (r - y) + (int64_t)(c - x) * (c - x);
      if (arg < 0 || d < best) {
        best = d;
        arg = r * w + c;
      }
    }
  return arg;
}

static int g_cases = 0;

// runs both passes on `image` and compares with the definition; false (and a message) on a difference
static bool check(const uint32_t* image, int kind, int h, int w, bool corrupt, const char* what) {
  const size_t px = (size_t)h * w;
  const uint32_t void_bits = void_bits_of(kind);
  std::unique_ptr<Entry[]> table(new Entry[px]);
  std::unique_ptr<uint32_t[]> out(new uint32_t[px]);
  std::unique_ptr<int32_t[]> indices(new int32_t[px]);
  row_pass(image, void_bits, kind, h, w, table.get());
  if (corrupt) table[0] = (Entry)(table[0] ^ 1);
  column_pass(image, void_bits, kind, h, w, table.get(), out.get(), indices.get());
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t at = (size_t)y * w + x;
      const bool is_hole = is_void(image[at], void_bits, kind);
      const int32_t want = is_hole ? pairwise(image, void_bits, kind, h, w, y, x) : (int32_t)at;
      const uint32_t want_bits = want < 0 ? image[at] : image[want];
      if (indices[at] != want || out[at] != want_bits) {
        fprintf(stderr, "%s kind %d %d x %d at (%d, %d): source %d value %08x, expected %d %08x\n", what, kind, h,
                w, y, x, indices[at], out[at], want, want_bits);
        return false;
      }
    }
  ++g_cases;
  return true;
}

static bool ring(int kind) {
  const int h = 11, w = 11, cy = 5, cx = 5;
  const int order[12][2] = {{-5, 0}, {-4, -3}, {-4, 3}, {-3, -4}, {-3, 4}, {0, -5},
                            {0, 5},  {3, -4},  {3, 4},  {4, -3},  {4, 3},  {5, 0}};
  std::unique_ptr<uint32_t[]> image(new uint32_t[(size_t)h * w]);
  for (int i = 0; i < h * w; ++i) image[i] = a_void(kind, i);
  for (const auto& p : order) image[(cy + p[0]) * w + cx + p[1]] = site_bits(kind, (cy + p[0]) * w + cx + p[1]);
  for (const auto& p : order) {
    if (!check(image.get(), kind, h, w, false, "ring")) return false;
    // the definition itself must name the stated winner
    const int32_t got = pairwise(image.get(), void_bits_of(kind), kind, h, w, cy, cx);
    if (got != (cy + p[0]) * w + cx + p[1]) {
      fprintf(stderr, "ring kind %d: the definition picks %d, expected (%d, %d)\n", kind, got, p[0], p[1]);
      return false;
    }
    image[got] = a_void(kind, got);
  }
  return check(image.get(), kind, h, w, false, "empty ring");
}

int main(int argc, char** argv) {
  const bool corrupt = argc == 2 && strcmp(argv[1], "corrupt") == 0;
  if (argc > 2 || (argc == 2 && !corrupt)) {
    fprintf(stderr, "usage: %s [corrupt]\n", argv[0]);
    return 2;
  }
  if (corrupt) {
    // one site in the middle of a 1 x 9 row: every entry is 4, entry 0 becomes 5
    uint32_t row[9];
    for (int x = 0; x < 9; ++x) row[x] = x == 4 ? site_bits(kKindI32, x) : a_void(kKindI32, x);
    if (check(row, kKindI32, 1, 9, true, "corrupt")) {
      fprintf(stderr, "a corrupted table went unnoticed\n");
      return 3;
    }
    return 1;
  }
  const int S = kRowSegment, T = kColTileRows;
  const int shapes[][2] = {{1, 1}, {1, 9},     {7, 5},     {13, 17},        {16, 33},   {3, 63}, {3, 64},
                           {3, 65}, {2, S - 1}, {2, S},     {2, S + 1},      {3, 2 * S + 5}, {T + 1, 70}};
  const int shares[] = {2, 50, 97};   // per cent void
  for (const auto& s : shapes) {
    const int h = s[0], w = s[1];
    for (int kind = 0; kind < 3; ++kind) {
      std::unique_ptr<uint32_t[]> image(new uint32_t[(size_t)h * w]);
      for (int pattern = 0; pattern < 6; ++pattern) {
        for (int i = 0; i < h * w; ++i) {
          bool hole;
          if (pattern < 3) hole = (int)(next_u32() % 100u) < shares[pattern];
          else if (pattern == 3) hole = true;
          else if (pattern == 4) hole = false;
          else hole = ((i / w) & 1) == 0 || next_u32() % 3u == 0;
          image[i] = hole ? a_void(kind, i) : site_bits(kind, i);
        }
        if (!check(image.get(), kind, h, w, false, "sweep")) return 1;
      }
    }
  }
  for (int kind = 0; kind < 3; ++kind)
    if (!ring(kind)) return 1;
  printf("nn_inpaint_host_check: %d cases OK\n", g_cases);
  return 0;
}
