// The device inflate's decoder (se3ds_amd/csrc/inflate_core.h) as a plain host program, for the
// sanitizers: the same code as the kernel with the one-lane HostPolicy.  Built and run by
// tests/test_inflate_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/inflate_host_check.cpp -o inflate_host_check && ./inflate_host_check CORPUS
//
// Corpus file, little-endian: "INFC", uint32 count, then per case uint32 compressed length, uint32
// expected inflated length, uint32 pitch, int32 expected status word, the compressed bytes and --
// for status 0 only -- the expected inflated bytes.  Every buffer is allocated at its exact size so
// that a read or write one byte outside it is a sanitizer report.  Each case runs twice: into a
// 16-byte aligned destination (the 16-byte flush) and into a misaligned one (the byte flush).
// Exit status 0: every case gave its status and every good one its bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../se3ds_amd/csrc/inflate_core.h"

using namespace se3ds::inflate;

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

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
  if (!read_exact(f, magic, 4) || memcmp(magic, "INFC", 4) != 0 || !read_exact(f, &count, 4)) {
    fprintf(stderr, "bad corpus header\n");
    return 2;
  }
  std::unique_ptr<Shared> shared(new Shared);
  int failures = 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t head[3];
    int32_t want = 0;
    if (!read_exact(f, head, sizeof head) || !read_exact(f, &want, 4)) {
      fprintf(stderr, "case %u: truncated corpus\n", i);
      return 2;
    }
    const uint32_t in_len = head[0], expected = head[1], pitch = head[2];
    if (in_len > kMaxStreamBytes || expected > kMaxStreamBytes || pitch < 1) {
      fprintf(stderr, "case %u: bad sizes\n", i);
      return 2;
    }
    std::unique_ptr<uint8_t[]> in(new uint8_t[in_len]);   // exact size, also when 0
    std::vector<uint8_t> want_out(want == 0 ? expected : 0);
    if (!read_exact(f, in.get(), in_len) || !read_exact(f, want_out.data(), want_out.size())) {
      fprintf(stderr, "case %u: truncated corpus\n", i);
      return 2;
    }
    for (int misalign = 0; misalign < 2; ++misalign) {
      void* block = nullptr;
      if (posix_memalign(&block, 16, (size_t)expected + misalign) != 0) {
        fprintf(stderr, "case %u: out of memory\n", i);
        return 2;
      }
      std::unique_ptr<void, decltype(&free)> out_mem(block, &free);
      uint8_t* out = static_cast<uint8_t*>(block) + misalign;
      if (expected) memset(out, 0xA5, expected);
      memset(shared.get(), 0xA5, sizeof(Shared));
      const HostPolicy policy;
      Inflater<HostPolicy> inflater(policy, *shared, in.get(), in_len, out, expected, pitch);
      const int32_t got = inflater.run();
      if (got != want) {
        fprintf(stderr, "case %u (misalign %d): status %d (detail %d), expected %d\n", i, misalign,
                got & 255, got >> 8, want);
        ++failures;
        continue;
      }
      if (want == 0) {
        if (expected && memcmp(out, want_out.data(), expected) != 0) {
          fprintf(stderr, "case %u (misalign %d): inflated bytes differ\n", i, misalign);
          ++failures;
        }
      }
    }
  }
  fclose(f);
  if (failures) {
    fprintf(stderr, "%d of %u cases failed\n", failures, 2 * count);
    return 1;
  }
  printf("inflate_host_check: %u cases x 2 alignments OK\n", count);
  return 0;
}
