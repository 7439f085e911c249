// Stand-alone host program around se3ds_amd/csrc/gif_lzw_core.h, the strip coder of the GIF
// encoder, for tests/test_gif_cpu.py: built with -fsanitize=address,undefined, it reads strips
//     uint32 pixels, uint8 first, uint8 last, uint8 pad[2], pixels bytes
// from the file named first and writes, per strip, to the file named second
//     uint64 bits, uint64 slot bytes, ceil(bits / 8) bytes of the code stream
// (little-endian throughout).  Every strip is coded into a heap block of exactly its slot size and
// with a hash table left dirty by the strip before, so that an overrun of the stated bound or a
// missed clear is the sanitizer's or the test's to see.  Nothing here is loaded into Python.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../se3ds_amd/csrc/gif_lzw_core.h"

namespace gif = se3ds::gif;

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: gif_host_check <strips in> <streams out>\n");
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "gif_host_check: cannot open the files\n");
    return 2;
  }
  std::vector<uint32_t> table(gif::kTableSlots, 0u);   // zero is a live entry: the clear must come first
  size_t strips = 0;
  for (;;) {
    unsigned char head[8];
    const size_t got = std::fread(head, 1, sizeof(head), in);
    if (got == 0) break;
    uint32_t pixels;
    std::memcpy(&pixels, head, 4);
    if (got != sizeof(head) || pixels < 1) {
      std::fprintf(stderr, "gif_host_check: strip %zu is malformed\n", strips);
      return 2;
    }
    std::vector<uint8_t> px(pixels);
    if (std::fread(px.data(), 1, pixels, in) != pixels) {
      std::fprintf(stderr, "gif_host_check: strip %zu is cut short\n", strips);
      return 2;
    }
    const uint64_t slot = (uint64_t)gif::strip_slot_bytes(pixels);
    std::vector<uint32_t> words(slot / 4);
    const gif::HostWave wave;
    const uint64_t bits = gif::lzw_strip(wave, px.data(), pixels, head[4] != 0, head[5] != 0, table.data(),
                                         words.data());
    if ((int64_t)bits > gif::strip_bits_bound(pixels)) {
      std::fprintf(stderr, "gif_host_check: strip %zu: %llu bits exceed the bound\n", strips,
                   (unsigned long long)bits);
      return 1;
    }
    std::fwrite(&bits, 8, 1, out);
    std::fwrite(&slot, 8, 1, out);
    std::fwrite(words.data(), 1, (size_t)((bits + 7) / 8), out);
    ++strips;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  std::printf("gif_host_check: %zu strips OK\n", strips);
  return 0;
}
