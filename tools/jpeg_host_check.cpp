// The device JPEG decoder (se3ds_amd/csrc/jpeg_core.h) as a plain host program, for the sanitizers:
// the same phase functions as the kernels, with the lanes of a workgroup simulated one after the
// other -- so the SPECULATION runs here too, decoding from wrong states included.  Built and run by
// tests/test_jpeg_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/jpeg_host_check.cpp -o jpeg_host_check && ./jpeg_host_check CORPUS
//
// Corpus file, little-endian: "JPGC", uint32 count, then per case int32 expected status code, uint32
// segment count, uint32 entropy byte count, uint32 pixel byte count (0 unless the status is 0), the
// image row (jpeg::Image; offsets and pointer unused), the segment rows (int64 x 5; offsets count
// from the entropy bytes' start), the entropy bytes, the expected pixels.  Every buffer is allocated
// at its exact size so that an access one byte outside it is a sanitizer report.  Each case runs
// with (lanes, chunk bytes) = (1, 16), (4, 16), (64, 16), (8, 128) and the kernel's (256, 128), and
// with the entropy bytes at two alignments.  Exit status 0: every case gave its status, and every
// good one its pixels, in every configuration.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../se3ds_amd/csrc/jpeg_core.h"

using namespace se3ds::jpeg;

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

struct Case {
  int32_t want;
  Image image;
  std::vector<int64_t> segments;
  std::vector<uint8_t> entropy, pixels;
};

// -> the status code of the first segment that failed (0: none); coefficients into `coef`.
template <int LANES, int CHUNK>
static int32_t entropy(const Case& c, const uint8_t* bytes, int16_t* coef, uint32_t* rounds_out) {
  using Sh = Shared<LANES, CHUNK>;
  std::unique_ptr<Sh> shared(new Sh);
  const int slots = slots_of(c.image);
  int32_t first = 0;
  for (size_t s = 0; s < c.segments.size() / kSegmentFields; ++s) {
    const int64_t* d = c.segments.data() + s * kSegmentFields;
    memset(shared.get(), 0xA5, sizeof(Sh));
    Decoder<LANES, CHUNK> decoder(*shared, c.image, bytes + d[1], (uint32_t)d[2], coef + d[3] * slots * 64,
                                  (uint32_t)(d[4] * slots));
    const HostPolicy<LANES> policy;
    const int32_t word = decoder.run(policy);
    const uint32_t windows = ((uint32_t)d[2] + Sh::kWindow - 1) / Sh::kWindow;
    if ((uint32_t)(word >> 8) > windows * (LANES + 1)) return -1;   // the bound on the rounds
    *rounds_out += (uint32_t)(word >> 8);
    if (!first) first = word & 255;
  }
  return first;
}

template <int LANES, int CHUNK>
static int run_case(const Case& c, uint32_t index, int misalign) {
  const Image& im = c.image;
  const size_t n = c.entropy.size();
  // exact size: the copy ends where the allocation ends (operator new aligns to 16)
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n + misalign]);
  uint8_t* bytes = exact.get() + misalign;
  if (n) memcpy(bytes, c.entropy.data(), n);
  const size_t blocks = (size_t)blocks_of(im);
  std::unique_ptr<int16_t[]> coef(new int16_t[blocks * 64]);
  memset(coef.get(), 0, blocks * 128);
  uint32_t rounds = 0;
  const int32_t got = entropy<LANES, CHUNK>(c, bytes, coef.get(), &rounds);
  if (got != c.want) {
    fprintf(stderr, "case %u (%d lanes x %d bytes, misalign %d): status %d, expected %d\n", index, LANES,
            CHUNK, misalign, got, c.want);
    return 1;
  }
  if (c.want != 0) return 0;
  std::unique_ptr<uint8_t[]> planes(new uint8_t[(size_t)plane_bytes(im)]);
  const int slots = slots_of(im), ny = slots == 1 ? 1 : slots - 2;
  for (size_t b = 0; b < blocks; ++b) {
    const int64_t mcu = (int64_t)b / slots;
    const int slot = (int)((int64_t)b - mcu * slots);
    const int comp = slot < ny ? 0 : slot - ny + 1;
    const int bx = comp == 0 ? slot % (int)im.h0 : 0, by = comp == 0 ? slot / (int)im.h0 : 0;
    const int64_t col = (mcu % im.mcus_x) * comp_h(im, comp) + bx;
    const int64_t row = (mcu / im.mcus_x) * comp_v(im, comp) + by;
    uint8_t* plane = planes.get();
    for (int i = 0; i < comp; ++i) plane += plane_w(im, i) * plane_h(im, i);
    const int64_t pitch = plane_w(im, comp);
    idct_block(coef.get() + b * 64, im.quant[comp], plane + row * 8 * pitch + col * 8, pitch);
  }
  const size_t out_bytes = (size_t)(im.width * im.height * im.out_channels);
  if (out_bytes != c.pixels.size()) {
    fprintf(stderr, "case %u: %zu expected pixel bytes for a %zu byte image\n", index, c.pixels.size(), out_bytes);
    return 2;
  }
  std::unique_ptr<uint8_t[]> out(new uint8_t[out_bytes]);
  for (int64_t y = 0; y < im.height; ++y)
    for (int64_t x = 0; x < im.width; ++x) pixel(im, planes.get(), out.get(), x, y);
  if (memcmp(out.get(), c.pixels.data(), out_bytes) != 0) {
    fprintf(stderr, "case %u (%d lanes x %d bytes, misalign %d): pixels differ\n", index, LANES, CHUNK,
            misalign);
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  char magic[4];
  uint32_t count = 0;
  if (!read_exact(f, magic, 4) || memcmp(magic, "JPGC", 4) != 0 || !read_exact(f, &count, 4)) {
    fprintf(stderr, "bad corpus header\n");
    return 2;
  }
  int failures = 0, runs = 0;
  for (uint32_t i = 0; i < count; ++i) {
    Case c;
    uint32_t head[3];
    if (!read_exact(f, &c.want, 4) || !read_exact(f, head, sizeof head) || !read_exact(f, &c.image, sizeof c.image)) {
      fprintf(stderr, "case %u: truncated corpus\n", i);
      return 2;
    }
    if (head[0] < 1 || head[0] > 65536 || head[1] > (1u << 24) || head[2] > (1u << 26)) {
      fprintf(stderr, "case %u: bad sizes\n", i);
      return 2;
    }
    c.segments.resize((size_t)head[0] * kSegmentFields);
    c.entropy.resize(head[1]);
    c.pixels.resize(head[2]);
    if (!read_exact(f, c.segments.data(), c.segments.size() * 8) || !read_exact(f, c.entropy.data(), head[1]) ||
        !read_exact(f, c.pixels.data(), head[2])) {
      fprintf(stderr, "case %u: truncated corpus\n", i);
      return 2;
    }
    // the checks of se3ds_jpeg_decode that the core relies on
    const Image& im = c.image;
    int64_t mcu = 0;
    bool ok = im.width >= 1 && im.height >= 1 && (im.ncomp == 1 || im.ncomp == 3) && im.h0 >= 1 && im.h0 <= 2 &&
              im.v0 >= 1 && im.v0 <= 2 && (im.ncomp == 3 || (im.h0 == 1 && im.v0 == 1)) &&
              (im.out_channels == 1 || im.out_channels == 3) &&
              im.mcus_x == (im.width + 8 * im.h0 - 1) / (8 * im.h0) &&
              im.mcus_y == (im.height + 8 * im.v0 - 1) / (8 * im.v0);
    for (size_t s = 0; ok && s < head[0]; ++s) {
      const int64_t* d = c.segments.data() + s * kSegmentFields;
      ok = d[1] >= 0 && d[2] >= 0 && d[1] + d[2] <= (int64_t)head[1] && d[3] == mcu && d[4] >= 1;
      mcu += d[4];
    }
    if (!ok || mcu != im.mcus_x * im.mcus_y) {
      fprintf(stderr, "case %u: bad tables\n", i);
      return 2;
    }
    for (int misalign = 0; misalign < 4; misalign += 3) {
      const int results[5] = {run_case<1, 16>(c, i, misalign), run_case<4, 16>(c, i, misalign),
                              run_case<64, 16>(c, i, misalign), run_case<8, 128>(c, i, misalign),
                              run_case<kLanes, kChunkBytes>(c, i, misalign)};
      for (int r : results) {
        if (r == 2) return 2;
        failures += r;
        ++runs;
      }
    }
  }
  fclose(f);
  if (failures) {
    fprintf(stderr, "%d of %d runs failed\n", failures, runs);
    return 1;
  }
  printf("jpeg_host_check: %u cases x 5 configurations x 2 alignments OK\n", count);
  return 0;
}
