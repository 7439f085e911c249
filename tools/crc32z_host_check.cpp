// The device zip / zlib CRC-32 (the kPolyZip, seeded instantiation of se3ds_amd/csrc/crc32c_core.h)
// as a plain host program, for the sanitizers: the same slice routine, block walk and combine order
// as the kernel, with a serial policy that visits the 64 lanes one after the other.  The sibling of
// tools/crc32c_host_check.cpp.  Built and run by tests/test_crc32z_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/crc32z_host_check.cpp -o crc32z_host_check && ./crc32z_host_check
//
// Cases: every length of {0..9, 15..17, 63..65, 255..257, B-1, B, B+1, 2B-1, 2B, 2B+1, 3B+5}
// (B = kBlockBytes) at every start alignment 0..15, over random bytes, zeros, 0xff and random bytes
// behind a long run of zeros.  Every case lies at the END of a heap allocation of exactly
// alignment + length bytes, so a 4- or 16-byte load that leaves the range is a sanitizer report.
// Each case is walked with runs of 1, 2, 3 and 64 blocks per "wave" and from the seeds 0, 0xffffffff
// and one arbitrary value.  Then one launch-like table: many seeded ranges of one buffer, empty and
// overlapping ones among them.  The yardstick is the bitwise loop below, itself pinned to the check
// value crc32("123456789") = 0xCBF43926 and to its own continuation property.
// `crc32z_host_check corrupt` flips one data bit after the yardstick ran: exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../se3ds_amd/csrc/crc32c_core.h"

using namespace se3ds::crc32c;

constexpr int kF = kFieldsSeeded;

// zlib.crc32(p[0:n], seed)
static uint32_t bitwise(const uint8_t* p, size_t n, uint32_t seed) {
  uint32_t c = seed ^ 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return c ^ 0xffffffffu;
}

struct SerialPolicy {
  uint32_t mul[kLanes];
  template <class F>
  uint32_t xor_lanes(F f) const {
    uint32_t v = 0;
    for (int lane = 0; lane < kLanes; ++lane) v ^= f(lane);
    return v;
  }
  uint32_t lane_multiplier(int lane) const { return mul[lane]; }
  void emit(uint32_t* p, uint32_t v) const { *p ^= v; }
};

static uint32_t g_tables[kTableWords];
static Pow2 g_pow2;
static SerialPolicy g_policy;

// what se3ds_crc32z_multi launches: the prepare pass, then the block walk in runs of per_wave
static void run(const uint8_t* buf, int64_t buf_bytes, const std::vector<int64_t>& table, int64_t per_wave,
                std::vector<uint32_t>* crc) {
  const int n = (int)(table.size() / kF);
  std::vector<int64_t> prefix((size_t)n + 1);
  crc->assign((size_t)n, 0u);
  int64_t blocks = 0;
  for (int s = 0; s < n; ++s) {
    prefix[(size_t)s] = blocks;
    (*crc)[(size_t)s] = table[(size_t)s * kF + 1] > 0 ? kInit : (uint32_t)table[(size_t)s * kF + 2];
    blocks += block_count(table[(size_t)s * kF + 1]);
  }
  prefix[(size_t)n] = blocks;
  for (int64_t g = 0; g < blocks; g += per_wave)
    walk<SerialPolicy, kPolyZip, kF>(g_policy, buf, buf_bytes, table.data(), prefix.data(), n, g, g + per_wave,
                                     g_tables, g_pow2, crc->data());
}

static uint32_t g_rng = 12345u;
static uint8_t next_byte() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return (uint8_t)(g_rng >> 24);
}

int main(int argc, char** argv) {
  const bool corrupt = argc == 2 && strcmp(argv[1], "corrupt") == 0;
  if (argc > 2 || (argc == 2 && !corrupt)) {
    fprintf(stderr, "usage: %s [corrupt]\n", argv[0]);
    return 2;
  }
  for (int i = 0; i < kTableWords; ++i) g_tables[i] = table_entry<kPolyZip>(i);
  g_pow2 = make_pow2<kPolyZip>();
  for (int lane = 0; lane < kLanes; ++lane) g_policy.mul[lane] = lane_multiplier<kPolyZip>(lane, g_pow2);
  const uint8_t* digits = reinterpret_cast<const uint8_t*>("123456789");
  if (bitwise(digits, 9, 0) != 0xCBF43926u || bitwise(digits + 4, 5, bitwise(digits, 4, 0)) != 0xCBF43926u) {
    fprintf(stderr, "the yardstick misses the CRC-32 check value\n");
    return 2;
  }
  const uint32_t seeds[] = {0u, 0xffffffffu, 0x1badb002u};

  const int64_t B = kBlockBytes;
  std::vector<int64_t> lengths;
  for (int64_t l = 0; l <= 9; ++l) lengths.push_back(l);
  for (int64_t l : {15, 16, 17, 63, 64, 65, 255, 256, 257}) lengths.push_back(l);
  for (int64_t l : {B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 5}) lengths.push_back(l);
  const int64_t runs[] = {1, 2, 3, 64};
  int failures = 0, cases = 0;
  std::vector<uint32_t> crc;
  for (int fill = 0; fill < 4; ++fill) {
    for (int64_t len : lengths) {
      for (int64_t align = 0; align < 16; ++align) {
        const int64_t bytes = align + len;
        void* block = nullptr;   // exact size (one byte for the empty buffer), 16-byte aligned base
        if (posix_memalign(&block, 16, (size_t)(bytes ? bytes : 1)) != 0) return 2;
        uint8_t* buf = static_cast<uint8_t*>(block);
        for (int64_t i = 0; i < bytes; ++i) {
          const uint8_t r = next_byte();
          buf[i] = fill == 0 ? r : fill == 1 ? 0 : fill == 2 ? 0xff : (i - align < (len * 3) / 4 ? 0 : r);
        }
        uint32_t want[3];
        for (int k = 0; k < 3; ++k) want[k] = bitwise(buf + align, (size_t)len, seeds[k]);
        if (corrupt && len > 0) buf[align + len / 2] ^= 0x10;
        for (int k = 0; k < 3; ++k) {
          for (int64_t per_wave : runs) {
            run(buf, bytes, {align, len, (int64_t)seeds[k]}, per_wave, &crc);
            ++cases;
            if (crc[0] != want[k]) {
              fprintf(stderr, "fill %d length %lld alignment %lld seed %08x run %lld: %08x, expected %08x\n", fill,
                      (long long)len, (long long)align, seeds[k], (long long)per_wave, crc[0], want[k]);
              ++failures;
            }
          }
        }
        free(block);
      }
    }
  }

  // one table over one buffer: random ranges, empty ones, 8-byte ones, a long one and its halves
  {
    const int64_t bytes = 6 * B + 13;
    uint8_t* buf = static_cast<uint8_t*>(malloc((size_t)bytes));
    if (!buf) return 2;
    for (int64_t i = 0; i < bytes; ++i) buf[i] = next_byte();
    std::vector<int64_t> table;
    auto add = [&](int64_t off, int64_t len) {   // every third row unseeded
      g_rng = g_rng * 1664525u + 1013904223u;
      table.push_back(off), table.push_back(len), table.push_back(table.size() % 9 == 2 ? 0 : (int64_t)g_rng);
    };
    add(0, 0), add(bytes, 0), add(0, bytes), add(0, bytes / 2), add(bytes / 2, bytes - bytes / 2);
    for (int i = 0; i < 200; ++i) {
      g_rng = g_rng * 1664525u + 1013904223u;
      const int64_t len = (int64_t)(g_rng >> 8) % 2001;
      g_rng = g_rng * 1664525u + 1013904223u;
      add((int64_t)(g_rng >> 4) % (bytes - len + 1), len);
      add((int64_t)(g_rng >> 5) % (bytes - 7), 8);
      if (i % 50 == 0) add(i, 0);
    }
    add(bytes - (3 * B + 5), 3 * B + 5), add(bytes - 1, 1), add(0, 1);
    std::vector<uint32_t> want;
    for (size_t s = 0; s < table.size() / kF; ++s)
      want.push_back(bitwise(buf + table[s * kF], (size_t)table[s * kF + 1], (uint32_t)table[s * kF + 2]));
    if (corrupt) buf[bytes / 3] ^= 1;
    for (int64_t per_wave : {(int64_t)1, (int64_t)2, (int64_t)7, (int64_t)1000}) {
      run(buf, bytes, table, per_wave, &crc);
      for (size_t s = 0; s < want.size(); ++s) {
        ++cases;
        if (crc[s] != want[s]) {
          fprintf(stderr, "table row %zu (offset %lld, length %lld) run %lld: %08x, expected %08x\n", s,
                  (long long)table[s * kF], (long long)table[s * kF + 1], (long long)per_wave, crc[s], want[s]);
          ++failures;
        }
      }
    }
    // a device table that does not match its validated host copy must not be followed out of the buffer
    std::vector<int64_t> bad = {bytes - 4, 8, 1, -1, 4, 2, 0, bytes + 1, 3, 0, 3, 4};
    run(buf, bytes, bad, 2, &crc);
    ++cases;
    if (crc[3] != bitwise(buf, 3, 4)) {
      fprintf(stderr, "a good row beside skipped rows: %08x\n", crc[3]);
      ++failures;
    }
    free(buf);
  }

  if (failures) {
    fprintf(stderr, "%d of %d cases failed\n", failures, cases);
    return 1;
  }
  printf("crc32z_host_check: %d cases OK\n", cases);
  return 0;
}
