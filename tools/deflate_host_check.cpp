// The device PNG encoder's core (se3ds_amd/csrc/deflate_core.h) as a plain host program, for the
// sanitizers and as the byte-exact twin of the kernel: the same code with the one-lane HostPolicy.
// Built and run by tests/test_png_encode_cpu.py (sanitised) and tests/test_png_encode_gpu.py (plain):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/deflate_host_check.cpp -o deflate_host_check && ./deflate_host_check CORPUS RESULT
//
// Corpus file, little-endian: "DEFC", uint32 count, then per case uint32 kind.
//   kind 0, one strip of filtered bytes: uint32 n (<= 65535), uint32 final flag, the n bytes.
//   kind 1, an image: uint32 height, row_bytes, bytes per pixel, filter mode (0..4, 5 adaptive),
//           then height x row_bytes pixel bytes; it is cut into strips as the kernel cuts it.
//   kind 2, a 16-bit grey image: the header of kind 1 with bytes per pixel 2, then height x
//           row_bytes bytes of little-endian samples; the encoder filters their big-endian bytes.
// Result file, per case: uint32 stream length, Adler-32 s1, s2 of the filtered bytes, the stream (for
// an image: the strips' streams joined, the sums combined).  Every buffer is allocated at its exact
// size -- a strip's slot at its bound of 10 + filtered bytes -- so that a read or write one byte
// outside it is a sanitizer report.  Exit status 0: every case was encoded within its bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../se3ds_amd/csrc/deflate_core.h"

using namespace se3ds::deflate;

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }
static bool write_exact(FILE* f, const void* src, size_t n) { return n == 0 || fwrite(src, 1, n, f) == n; }

// one strip: s.data[0, n) -> appended to `stream`; false when the bound is broken
static bool strip(Encoder<HostPolicy>& enc, uint8_t* slot, uint32_t n, bool final_strip,
                  std::vector<uint8_t>* stream) {
  const uint32_t len = enc.compress(n, final_strip);
  if (len > kStripOverhead + n) return false;
  stream->insert(stream->end(), slot, slot + len);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s CORPUS RESULT\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  FILE* g = f ? fopen(argv[2], "wb") : nullptr;
  if (!f || !g) {
    perror(f ? argv[2] : argv[1]);
    return 2;
  }
  char magic[4];
  uint32_t count = 0;
  if (!read_exact(f, magic, 4) || memcmp(magic, "DEFC", 4) != 0 || !read_exact(f, &count, 4)) {
    fprintf(stderr, "bad corpus header\n");
    return 2;
  }
  std::unique_ptr<Shared> shared(new Shared);
  const HostPolicy policy;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t kind = 0;
    std::vector<uint8_t> stream;
    uint32_t s1 = 1, s2 = 0;
    bool ok = read_exact(f, &kind, 4) && kind <= 2;
    if (ok && kind == 0) {
      uint32_t head[2];
      ok = read_exact(f, head, sizeof head) && head[0] <= kMaxStripBytes;
      if (ok) {
        const uint32_t n = head[0];
        memset(shared.get(), 0xA5, sizeof(Shared));
        ok = read_exact(f, shared->data, n);
        void* block = nullptr;
        if (ok && posix_memalign(&block, 8, (size_t)kStripOverhead + n) != 0) ok = false;
        std::unique_ptr<void, decltype(&free)> slot_mem(block, &free);
        if (ok) {
          uint8_t* slot = static_cast<uint8_t*>(block);
          Encoder<HostPolicy> enc(policy, *shared, slot);
          ok = strip(enc, slot, n, head[1] != 0, &stream);
          s1 = enc.s1();
          s2 = enc.s2();
        }
      }
    } else if (ok) {
      uint32_t head[4];
      ok = read_exact(f, head, sizeof head);
      const uint32_t height = head[0], row_bytes = head[1], bpp = head[2], mode = head[3];
      ok = ok && height >= 1 && height < (1u << 20) && row_bytes >= 1 && row_bytes < kMaxStripBytes &&
           (kind == 2 ? bpp == 2 : (bpp == 1 || bpp == 3)) && row_bytes % bpp == 0 &&
           mode <= kFilterAdaptive;
      if (ok) {
        std::unique_ptr<uint8_t[]> image(new uint8_t[(size_t)height * row_bytes]);   // exact size
        ok = read_exact(f, image.get(), (size_t)height * row_bytes);
        const uint32_t per = strip_rows(row_bytes);
        for (uint32_t row0 = 0; ok && row0 < height; row0 += per) {
          const uint32_t rows = height - row0 < per ? height - row0 : per;
          void* block = nullptr;
          if (posix_memalign(&block, 8, (size_t)kStripOverhead + (size_t)rows * (1 + row_bytes)) != 0) {
            ok = false;
            break;
          }
          std::unique_ptr<void, decltype(&free)> slot_mem(block, &free);
          uint8_t* slot = static_cast<uint8_t*>(block);
          memset(shared.get(), 0xA5, sizeof(Shared));
          Encoder<HostPolicy> enc(policy, *shared, slot);
          const uint32_t n = enc.filter(image.get(), row_bytes, bpp, mode, row0, rows, kind == 2);
          ok = strip(enc, slot, n, row0 + rows == height, &stream);
          adler_combine(s1, s2, enc.s1(), enc.s2(), n, &s1, &s2);
        }
      }
    }
    if (!ok) {
      fprintf(stderr, "case %u: bad corpus entry, or a strip beyond its bound\n", i);
      return 1;
    }
    const uint32_t out_head[3] = {(uint32_t)stream.size(), s1, s2};
    if (!write_exact(g, out_head, sizeof out_head) || !write_exact(g, stream.data(), stream.size())) {
      perror(argv[2]);
      return 2;
    }
  }
  fclose(f);
  if (fclose(g) != 0) {
    perror(argv[2]);
    return 2;
  }
  printf("deflate_host_check: %u cases OK\n", count);
  return 0;
}
