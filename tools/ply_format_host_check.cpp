// The text formatting of the point-cloud writer (se3ds_amd/csrc/ply_format_core.h) as a plain host
// program, for the sanitizers: the functions the kernels of ply.hip call, one value at a time.  Built
// and run by tests/test_ply_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/ply_format_host_check.cpp -o ply_format_host_check && ./ply_format_host_check
//
// For every fp32 bit pattern it formats, the digits and the decimal exponent must equal those of
// std::to_chars(double, scientific) of the widened value (the shortest round-trip digits, closest
// among the shortest), the text must read back through strtod to the same binary64, its length must be
// the record's and at most kMaxFloatChars, and it is written into a heap block of exactly that length,
// so a character too many is a sanitizer report.  Non-finite values must print nan / inf / -inf.
// Cases (each pattern with both signs unless it lists both itself):
//   * 2^k for k in [-149, 127] with both neighbouring patterns              277 x 3 x 2
//   * the subnormal patterns 1, 1 + 4099, ... below 2^23                    2047 x 2
//   * every bit pattern that is a multiple of 4099                          1047809
//   * strtof("1e<k>") for k in [-45, 38] with both neighbouring patterns    84 x 3 x 2
//   * int32: the edge values and every 10^k - 1, 10^k, both signs, against snprintf
//   * one line of the longest values: exactly kMaxLineBytes or less
//   * log10_pow2, log10_pow5 and pow5_bits against exact decimal powers for e in [0, 203]
// `ply_format_host_check corrupt` flips one table entry: exit status 1.
// `ply_format_host_check dump FILE` reads hexadecimal bit patterns from standard input, one per line,
// and writes `<pattern> <text>` lines to FILE (tests/test_ply_cpu.py compares them with Python's text).
// `ply_format_host_check exhaustive [FIRST LAST]` runs every pattern of [FIRST, LAST] (hexadecimal;
// default all 2^32): minutes, not part of the suite.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../se3ds_amd/csrc/ply_format_core.h"

using namespace se3ds::ply;

static Tables g_tables = make_tables();
static long long g_cases = 0;

static bool fail(uint32_t bits, const char* what, const std::string& got, const std::string& want) {
  fprintf(stderr, "%08x: %s: got '%s', expected '%s'\n", bits, what, got.c_str(), want.c_str());
  return false;
}

// formats `bits` into an exact-size heap block; false (and a message) on any difference
static bool check_float(uint32_t bits, std::string* text_out = nullptr) {
  const Record r = to_decimal(bits, g_tables.w);
  if (r.length < 3 || r.length > (uint32_t)kMaxFloatChars) return fail(bits, "length", std::to_string(r.length), "3..23");
  std::unique_ptr<char[]> block(new char[r.length]);
  const uint32_t n = write_float(r, block.get());
  const std::string text(block.get(), r.length);
  if (n != r.length) return fail(bits, "written", std::to_string(n), std::to_string(r.length));
  if (text_out) *text_out = text;
  float x;
  memcpy(&x, &bits, sizeof x);
  const double wide = (double)x;
  ++g_cases;
  if (x != x) return text == "nan" ? true : fail(bits, "text", text, "nan");
  if (x - x != 0.0f) {
    const char* want = x < 0 ? "-inf" : "inf";
    return text == want ? true : fail(bits, "text", text, want);
  }
  for (char c : text)
    if (!((c >= '0' && c <= '9') || c == '.' || c == '-' || c == '+' || c == 'e')) return fail(bits, "character", text, "0-9.e+-");
  // digits and exponent against the library's shortest scientific text
  char sci[64];
  const std::to_chars_result tc = std::to_chars(sci, sci + sizeof sci, std::fabs(wide), std::chars_format::scientific);
  std::string digits;
  const char* p = sci;
  for (; p < tc.ptr && *p != 'e'; ++p)
    if (*p != '.') digits.push_back(*p);
  const int exponent = atoi(std::string(p + 1, (const char*)tc.ptr).c_str());
  const std::string mine = std::to_string((unsigned long long)r.digits);
  if (mine != digits || (int)r.ndigits != (int)digits.size()) return fail(bits, "digits", mine, digits);
  if (wide != 0 && r.d != exponent) return fail(bits, "exponent", std::to_string(r.d), std::to_string(exponent));
  if (((r.cls & kNegative) != 0) != ((bits >> 31) != 0)) return fail(bits, "sign", text, "the value's");
  // the text reads back to the same binary64
  char* end = nullptr;
  const double back = strtod(text.c_str(), &end);
  if (*end != 0 || memcmp(&back, &wide, sizeof back) != 0) return fail(bits, "strtod", text, std::string(sci, tc.ptr));
  // layout: positional for -4 <= d < 16 (a point, no exponent), otherwise an exponent of two digits
  const bool has_e = text.find('e') != std::string::npos, has_point = text.find('.') != std::string::npos;
  const bool positional = r.d >= -4 && r.d < 16;
  if (positional ? (has_e || !has_point) : (!has_e || has_point != (r.ndigits > 1)))
    return fail(bits, "layout", text, positional ? "positional" : "scientific");
  return true;
}

static bool both_signs(uint32_t bits) { return check_float(bits & 0x7fffffffu) && check_float(bits | 0x80000000u); }

static bool check_int(int32_t v) {
  char want[16];
  snprintf(want, sizeof want, "%d", v);
  const uint32_t n = int_length(v);
  if (n > (uint32_t)kMaxIntChars) return fail((uint32_t)v, "int length", std::to_string(n), "<= 11");
  std::unique_ptr<char[]> block(new char[n]);
  const uint32_t w = write_int(v, block.get());
  ++g_cases;
  if (w != n || std::string(block.get(), n) != want) return fail((uint32_t)v, "int", std::string(block.get(), n), want);
  return true;
}

// digits of b^e in decimal, least significant first
static std::vector<int> decimal_power(int b, int e) {
  std::vector<int> d(1, 1);
  for (int k = 0; k < e; ++k) {
    int carry = 0;
    for (size_t i = 0; i < d.size(); ++i) {
      const int t = d[i] * b + carry;
      d[i] = t % 10;
      carry = t / 10;
    }
    while (carry) {
      d.push_back(carry % 10);
      carry /= 10;
    }
  }
  return d;
}

static bool check_logs() {
  std::vector<uint32_t> five(1, 1);   // 5^e in base 2^32, least significant first
  for (int e = 0; e <= -kMinE2; ++e) {
    if (log10_pow2(e) != (int)decimal_power(2, e).size() - 1 || log10_pow5(e) != (int)decimal_power(5, e).size() - 1) {
      fprintf(stderr, "log10 of a power: e = %d\n", e);
      return false;
    }
    int bits = 32 * ((int)five.size() - 1);
    for (uint32_t top = five.back(); top; top >>= 1) ++bits;
    if (pow5_bits(e) != bits) {
      fprintf(stderr, "bits of 5^%d: %d, expected %d\n", e, pow5_bits(e), bits);
      return false;
    }
    uint64_t carry = 0;
    for (uint32_t& limb : five) {
      const uint64_t t = (uint64_t)limb * 5u + carry;
      limb = (uint32_t)t;
      carry = t >> 32;
    }
    if (carry) five.push_back((uint32_t)carry);
    ++g_cases;
  }
  return true;
}

static bool check_line() {
  // -0.00012345679 style values are 23 characters: the neighbour below 1e-4 with a minus sign
  const float tiny = -9.999999e-05f;
  uint32_t bits;
  memcpy(&bits, &tiny, sizeof bits);
  uint32_t longest = 0, longest_bits = bits;
  for (uint32_t b = bits - 64; b <= bits + 64; ++b) {
    const Record r = to_decimal(b, g_tables.w);
    if (r.length > longest) longest = r.length, longest_bits = b;
  }
  const Record r = to_decimal(longest_bits, g_tables.w);
  const Record xyz[3] = {r, r, r};
  const int32_t rgb[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  const uint32_t n = line_length(xyz, rgb);
  if (n > (uint32_t)kMaxLineBytes) return fail(longest_bits, "line length", std::to_string(n), "<= kMaxLineBytes");
  std::unique_ptr<char[]> block(new char[n]);
  const uint32_t w = write_line(xyz, rgb, block.get());
  ++g_cases;
  if (w != n || block[n - 1] != '\n' || block[n - 2] != ' ') return fail(longest_bits, "line", std::string(block.get(), n), "x y z r g b \\n");
  if (longest != (uint32_t)kMaxFloatChars || n != (uint32_t)kMaxLineBytes)   // the bound is attained
    return fail(longest_bits, "bound", std::to_string(longest) + "/" + std::to_string(n), "23/109");
  return true;
}

static bool sweep() {
  for (int k = kMinBinaryExponent; k <= kMaxBinaryExponent; ++k) {
    const uint32_t bits = k < -126 ? 1u << (k + 149) : (uint32_t)(k + 127) << 23;
    for (uint32_t b = bits - 1; b <= bits + 1; ++b)
      if (!both_signs(b)) return false;
  }
  for (uint32_t b = 1; b < (1u << 23); b += 4099)
    if (!both_signs(b)) return false;
  for (uint64_t b = 0; b <= 0xffffffffull; b += 4099)
    if (!check_float((uint32_t)b)) return false;
  for (int k = -45; k <= 38; ++k) {
    char text[16];
    snprintf(text, sizeof text, "1e%d", k);
    const float f = strtof(text, nullptr);
    uint32_t bits;
    memcpy(&bits, &f, sizeof bits);
    for (uint32_t b = bits - 1; b <= bits + 1; ++b)
      if (!both_signs(b)) return false;
  }
  const int32_t edges[] = {INT32_MIN, INT32_MIN + 1, -256, -255, -1, 0, 1, 9, 10, 99, 100, 255, 256, INT32_MAX - 1, INT32_MAX};
  for (int32_t v : edges)
    if (!check_int(v)) return false;
  for (int64_t p = 10; p <= 1000000000; p *= 10)
    for (int64_t v : {p - 1, p, 1 - p, -p})
      if (!check_int((int32_t)v)) return false;
  return check_line() && check_logs();
}

int main(int argc, char** argv) {
  const std::string mode = argc >= 2 ? argv[1] : "";
  if (mode == "corrupt" && argc == 2) {
    g_tables.w[2 * 18 + 1] ^= (uint64_t)1 << 40;   // 5^18: the entry 1.0f and its binade use
    if (sweep()) {
      fprintf(stderr, "a corrupted table went unnoticed\n");
      return 3;
    }
    return 1;
  }
  if (mode == "dump" && argc == 3) {
    FILE* out = fopen(argv[2], "w");
    if (!out) return 2;
    char line[64];
    while (fgets(line, sizeof line, stdin)) {
      const uint32_t bits = (uint32_t)strtoul(line, nullptr, 16);
      std::string text;
      if (!check_float(bits, &text)) return 1;
      fprintf(out, "%08x %s\n", bits, text.c_str());
    }
    return fclose(out) == 0 ? 0 : 2;
  }
  if (mode == "exhaustive" && (argc == 2 || argc == 4)) {
    const uint64_t first = argc == 4 ? strtoull(argv[2], nullptr, 16) : 0, last = argc == 4 ? strtoull(argv[3], nullptr, 16) : 0xffffffffull;
    for (uint64_t b = first; b <= last && b <= 0xffffffffull; ++b)
      if (!check_float((uint32_t)b)) return 1;
    printf("ply_format_host_check: %lld cases OK\n", g_cases);
    return 0;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: %s [corrupt | dump FILE | exhaustive [FIRST LAST]]\n", argv[0]);
    return 2;
  }
  if (!sweep()) return 1;
  printf("ply_format_host_check: %lld cases OK\n", g_cases);
  return 0;
}
