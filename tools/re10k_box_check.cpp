// Stand-alone host program around se3ds_amd/csrc/re10k_box_core.h, the crop-box arithmetic of the
// RE10K input transform, for tests/test_re10k_cpu.py: built with -fsanitize=address,undefined and
// -ffp-contract=off, it reads rows of
//     r0 r1 c0 c1 height width pad x_shift y_shift
// from standard input (the three draws as the hexadecimal bit patterns of their fp32 values, so that
// no decimal conversion stands between the test's numbers and these) and prints, per row,
//     x_min y_min x_max y_max status
// The test compares that with its NumPy restatement.  Nothing here is loaded into Python.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../se3ds_amd/csrc/re10k_box_core.h"

static float from_bits(unsigned bits) {
  float f;
  static_assert(sizeof(f) == sizeof(bits), "fp32 bit pattern");
  std::memcpy(&f, &bits, sizeof(f));
  return f;
}

int main() {
  struct Row { int r0, r1, c0, c1, h, w; unsigned pad, xs, ys; };
  std::vector<Row> rows;   // on the heap: an overrun is the sanitizer's to see
  Row r;
  for (;;) {
    const int got = std::scanf("%d %d %d %d %d %d %x %x %x", &r.r0, &r.r1, &r.c0, &r.c1, &r.h, &r.w,
                               &r.pad, &r.xs, &r.ys);
    if (got == EOF) break;
    if (got != 9 || r.h <= 0 || r.w <= 0) {
      std::fprintf(stderr, "re10k_box_check: row %zu is malformed\n", rows.size());
      return 2;
    }
    rows.push_back(r);
  }
  for (const Row& q : rows) {
    const se3ds::Re10kBox b = se3ds::re10k_box(q.r0, q.r1, q.c0, q.c1, q.h, q.w, from_bits(q.pad),
                                               from_bits(q.xs), from_bits(q.ys));
    std::printf("%d %d %d %d %d\n", b.x_min, b.y_min, b.x_max, b.y_max, b.status);
  }
  std::fprintf(stderr, "re10k_box_check: %zu rows\n", rows.size());
  return 0;
}
