// The device JPEG encoder (se3ds_amd/csrc/jpeg_encode_core.h) as a plain host program, for the
// sanitizers: the same phase functions as the kernels of csrc/jpeg_encode.hip, with the lanes of a
// workgroup run one after the other.  Built and run by tests/test_jpeg_encode_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/jpeg_encode_host_check.cpp -o jpeg_encode_host_check && ./jpeg_encode_host_check CORPUS
//
// Corpus file, little-endian: "JPGE", uint32 count, then per case the table row (jpeg_encode::Image,
// 48 int64; pointer, first_block and first_tile unused), uint32 pixel byte count, uint32 expected byte count,
// the pixels, the expected entropy-coded bytes (what lies between the SOS header and EOI).  Every
// buffer is allocated at its exact size so that an access one byte outside it is a sanitizer
// report.  Every case runs alone and all cases run as one batch, each with 4, 64 and 256 lanes in
// the scans and the pack.  Exit status 0: every run gave the expected bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../se3ds_amd/csrc/jpeg_encode_core.h"

using namespace se3ds::jpeg_encode;

struct Case {
  Image image;
  std::vector<uint8_t> pixels, want;
};

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

// cases [from, to) as one batch with `lanes` lanes -> 0, or 1 after a message
static int run(const std::vector<Case>& cases, size_t from, size_t to, int lanes) {
  const int n = (int)(to - from);
  std::vector<Image> table(n);
  int64_t blocks = 0, tiles = 0;
  size_t want_bytes = 0;
  for (int i = 0; i < n; ++i) {
    table[i] = cases[from + i].image;
    table[i].src = (int64_t) reinterpret_cast<uintptr_t>(cases[from + i].pixels.data());
    table[i].first_block = blocks;
    table[i].first_tile = tiles;
    tiles += tiles_of(table[i]);
    blocks += blocks_of(table[i]);
    want_bytes += cases[from + i].want.size();
  }
  const int64_t groups = (blocks + kScanGroup - 1) / kScanGroup, units = (blocks + kPackBlocks - 1) / kPackBlocks;
  // phase 1: the tiled form, lane by lane, held against the direct form
  std::unique_ptr<int16_t[]> coef(new int16_t[blocks * 64]), direct(new int16_t[64]);
  std::unique_ptr<TileShared> tile_sh(new TileShared);
  for (int64_t tile = 0; tile < tiles; ++tile) {
    const Image& im = table[image_of_tile(table.data(), n, tile)];
    const Tile t = tile_of(im, tile - im.first_tile);
    memset(tile_sh.get(), 0xA5, sizeof(TileShared));
    for (int l = 0; l < lanes; ++l) tile_load(l, lanes, im, t, *tile_sh);
    for (int l = 0; l < kTileBlocks; ++l) tile_dct(l, im, t, *tile_sh, coef.get() + im.first_block * 64);
  }
  for (int64_t b = 0; b < blocks; ++b) {
    const Image& im = table[image_of(table.data(), n, b)];
    transform(im, b - im.first_block, direct.get());
    if (memcmp(direct.get(), coef.get() + b * 64, 128) != 0)
      return fprintf(stderr, "block %lld: the tiled transform differs from the direct one\n", (long long)b), 1;
  }
  // phase 2
  std::unique_ptr<Codes> codes(new Codes);
  for (int t = 0; t < 4; ++t) build_codes(t, *codes);
  std::unique_ptr<uint32_t[]> slots(new uint32_t[blocks * kBlockWords]);
  memset(slots.get(), 0xA5, sizeof(uint32_t) * blocks * kBlockWords);
  std::unique_ptr<uint16_t[]> bits(new uint16_t[blocks]);
  std::unique_ptr<Span32[]> inclusive(new Span32[blocks]), aggregate(new Span32[groups]);
  std::unique_ptr<uint64_t[]> group_start(new uint64_t[groups + 1]);
  // a group as jpeg_measure_kernel scans it: every lane's span, then log2(kScanGroup) doubling steps
  // between two buffers (the lanes behind the last block hold the identity)
  std::vector<Span32> scan[2] = {std::vector<Span32>(kScanGroup), std::vector<Span32>(kScanGroup)};
  for (int64_t g = 0; g < groups; ++g) {
    for (int lane = 0; lane < kScanGroup; ++lane) {
      const int64_t b = g * kScanGroup + lane;
      Span mine = {0, 0, 0};
      if (b < blocks) {
        const Image& im = table[image_of(table.data(), n, b)];
        const Place p = place_of(im, b - im.first_block);
        const int pred = p.pred_zero ? 0 : coef[predictor_block(im, p, b) * 64];
        const int len = encode_block(coef.get() + b * 64, pred, p.comp ? 1 : 0, *codes, slots.get() + b * kBlockWords);
        if (len < 4 || len > kMaxBlockBits) return fprintf(stderr, "block %lld: %d bits\n", (long long)b, len), 1;
        bits[b] = (uint16_t)len;
        mine = span_of_block(p, len);
      }
      scan[0][lane] = narrow(mine);
    }
    int cur = 0;
    for (int step = 1; step < kScanGroup; step <<= 1, cur ^= 1)
      for (int lane = 0; lane < kScanGroup; ++lane) {
        Span s = widen(scan[cur][lane]);
        if (lane >= step) s = then(widen(scan[cur][lane - step]), s);
        scan[cur ^ 1][lane] = narrow(s);
      }
    for (int lane = 0; lane < kScanGroup && g * kScanGroup + lane < blocks; ++lane)
      inclusive[g * kScanGroup + lane] = scan[cur][lane];
    aggregate[g] = scan[cur][kScanGroup - 1];
  }
  {
    std::unique_ptr<Span[]> carry(new Span[lanes]);
    std::unique_ptr<uint64_t[]> carry_pos(new uint64_t[lanes]);
    for (int step = 1; step <= 3; ++step)
      for (int l = 0; l < lanes; ++l)
        group_scan(step, l, lanes, aggregate.get(), groups, carry.get(), carry_pos.get(), group_start.get());
  }
  // phase 4
  std::unique_ptr<PackShared> sh(new PackShared);
  std::unique_ptr<uint64_t[]> unit_start(new uint64_t[units + 1]);
  std::unique_ptr<uint8_t[]> out(new uint8_t[want_bytes]);
  std::vector<int64_t> starts(n + 1, -1);
  for (int pass = 0; pass < 2; ++pass) {
    uint64_t at = 0;
    for (int64_t u = 0; u < units; ++u) {
      const Unit unit = unit_of(u, blocks, inclusive.get(), group_start.get());
      if (unit.end_byte > (uint32_t)kUnitRawBytes) return fprintf(stderr, "unit %lld: %u raw bytes\n", (long long)u, unit.end_byte), 1;
      memset(sh.get(), 0xA5, sizeof(PackShared));
      for (int l = 0; l < lanes; ++l) pack_clear(l, lanes, *sh);
      for (int l = 0; l < lanes; ++l)
        pack_deposit(l, lanes, unit, table.data(), n, blocks, inclusive.get(), group_start.get(), bits.get(),
                     slots.get(), *sh);
      for (int l = 0; l < lanes; ++l) pack_count(l, lanes, unit, *sh);
      const uint32_t length = pack_length(lanes, unit, *sh);
      if (pass == 0) {
        unit_start[u] = at;
        at += length;
        unit_start[u + 1] = at;
        continue;
      }
      if (unit_start[units] != want_bytes)
        return fprintf(stderr, "%llu bytes, expected %zu\n", (unsigned long long)unit_start[units], want_bytes), 1;
      uint8_t* dst = out.get() + unit_start[u];
      const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
      for (int l = 0; l < lanes; ++l) pack_stuff(l, lanes, unit, *sh, shift, unit_start[u], starts.data());
      if (u == 0) starts[0] = 0;
      for (int l = 0; l < lanes; ++l) pack_store(l, lanes, *sh, shift, length, dst);
    }
  }
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    const std::vector<uint8_t>& want = cases[from + i].want;
    if (starts[i] != (int64_t)at || starts[i + 1] != (int64_t)(at + want.size()))
      return fprintf(stderr, "case %zu: bytes [%lld, %lld), expected [%zu, %zu)\n", from + i, (long long)starts[i],
                     (long long)starts[i + 1], at, at + want.size()), 1;
    if (memcmp(out.get() + at, want.data(), want.size()) != 0) {
      size_t d = 0;
      while (out[at + d] == want[d]) ++d;
      return fprintf(stderr, "case %zu: bytes differ at %zu of %zu\n", from + i, d, want.size()), 1;
    }
    at += want.size();
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s CORPUS\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  char magic[4];
  uint32_t count = 0;
  if (!read_exact(f, magic, 4) || memcmp(magic, "JPGE", 4) != 0 || !read_exact(f, &count, 4))
    return fprintf(stderr, "not a corpus file\n"), 2;
  std::vector<Case> cases(count);
  for (Case& c : cases) {
    uint32_t sizes[2];
    if (!read_exact(f, &c.image, sizeof(Image)) || !read_exact(f, sizes, 8)) return fprintf(stderr, "truncated corpus\n"), 2;
    c.pixels.resize(sizes[0]);
    c.want.resize(sizes[1]);
    if (!read_exact(f, c.pixels.data(), sizes[0]) || !read_exact(f, c.want.data(), sizes[1]))
      return fprintf(stderr, "truncated corpus\n"), 2;
    if ((int64_t)sizes[0] != c.image.width * c.image.height * c.image.ncomp) return fprintf(stderr, "pixel count\n"), 2;
  }
  fclose(f);
  static const int kLaneCounts[3] = {4, 64, 256};
  for (int lanes : kLaneCounts) {
    for (size_t i = 0; i < cases.size(); ++i)
      if (run(cases, i, i + 1, lanes)) return fprintf(stderr, "  (case %zu alone, %d lanes)\n", i, lanes), 1;
    if (run(cases, 0, cases.size(), lanes)) return fprintf(stderr, "  (the batch, %d lanes)\n", lanes), 1;
  }
  printf("%u cases x 3 lane counts, alone and as one batch OK\n", count);
  return 0;
}
