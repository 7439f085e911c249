// Text of one point-cloud line `x y z r g b \n` as SE3DSModel.write_memory_as_pointcloud writes it
// (reference models/models.py:154-178): three fp32 coordinates and three integer colours, each
// followed by one space, then a newline.  One text for two builds: the kernels of ply.hip and a plain
// C++ program (tools/ply_format_host_check.cpp) under the host sanitizers.  Everything is
// `__host__ __device__`; compiled without HIP it is ordinary C++17.  Integer arithmetic only.
//
// Floats.  The host loop prints '{}'.format(np.float32(x)): NumPy widens the scalar to a Python float
// and prints repr of that binary64, so np.float32(0.1) is 0.10000000149011612, not 0.1.  The rules:
//   * digits: the shortest decimal string (1..17 digits) that reads back as the same binary64, the
//     closest to the value among the shortest;
//   * d = decimal exponent of the first digit.  -4 <= d < 16: positional (0.0001, 123.25, an integer
//     ends in `.0`); otherwise d[.ddd]e+XX / e-XX with at least two exponent digits;
//   * -0.0 keeps its sign; every NaN is `nan`; infinities are `inf` and `-inf`.
//
// Digits come from the Ryu formulation (Adams, PLDI 2018): with the binary64 m2 * 2^(e2+2) and its
// rounding interval [4 m2 - 1 - mmShift, 4 m2 + 2] * 2^e2, one 64 x 128-bit multiply-shift against a
// table of powers of 5 (e2 < 0) or of their reciprocals (e2 >= 0) gives floor(. / 10^q) of the value
// and of both interval ends; digits are then removed while the ends still differ.
//
// Range.  Only widened fp32 values are formatted: the exponent of the leading bit lies in
// [kMinBinaryExponent, kMaxBinaryExponent] = [-149, 127] (fp32 subnormals are binary64 normals), so
// e2 is in [-203, 73], the 5^i table needs i <= 63 and the 5^-q table q <= 20.  The tables are sized
// for exactly that and the static_asserts below walk every e2 of the range; to_decimal takes fp32
// bits, so nothing outside the range can be asked of it.  d lies in [-45, 38]: two exponent digits.
//
// Tables.  make_tables() computes them at compile time with exact integer arithmetic (192-bit
// products and a long division written below): pow5[i] = the top kPow5Bits bits of 5^i,
// inv[q] = floor(2^(bits(5^q) - 1 + kPow5InvBits) / 5^q) + 1.
//
// Line bound.  A float is at most 23 characters: sign, then either `0.` + 3 zeros + 17 digits
// (d = -4; 22), 17 digits and a point (18), 16 digits + `.0` (d = 15, 18) or 17 digits, a point and
// `e-XX` (22).  An integer is at most 11 (`-2147483648`).  With one space after each value and the
// newline: kMaxLineBytes = 3 * 24 + 3 * 12 + 1 = 109.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef SE3DS_HD
#if defined(__HIPCC__)
#define SE3DS_HD __host__ __device__ inline
#else
#define SE3DS_HD inline
#endif
#endif

namespace se3ds {
namespace ply {

typedef unsigned __int128 u128;

constexpr int kMinBinaryExponent = -149, kMaxBinaryExponent = 127;   // of the leading bit
constexpr int kPow5Bits = 125, kPow5InvBits = 125;
constexpr int kPow5Count = 64, kPow5InvCount = 21;
constexpr int kTableWords = 2 * (kPow5Count + kPow5InvCount);   // uint64: pow5 (lo, hi) pairs, then inv
constexpr int kMaxDigits = 17;
constexpr int kMaxFloatChars = 23, kMaxIntChars = 11;
constexpr int kMaxLineBytes = 3 * (kMaxFloatChars + 1) + 3 * (kMaxIntChars + 1) + 1;
constexpr int kChunkPoints = 256;                        // points (lines) of one workgroup of ply.hip
constexpr int64_t kMaxPoints = (int64_t)1 << 24;         // per call
constexpr int kRecordBytes = 16;                          // sizeof(Record)
constexpr int kBinaryRecordBytes = 15;                    // binary body: float x, y, z; uchar red, green, blue

constexpr int kFinite = 0, kNan = 1, kInf = 2, kNegative = 0x80;   // Record::cls

// one formatted float before its characters are placed: value = digits * 10^(d - ndigits + 1)
struct Record {
  uint64_t digits;    // 1..17 decimal digits as an integer (0 for a zero)
  int16_t d;          // decimal exponent of the first digit
  uint8_t ndigits;
  uint8_t cls;        // kFinite / kNan / kInf, | kNegative
  uint32_t length;    // characters of the text
};
static_assert(sizeof(Record) == kRecordBytes, "a record is one 16-byte store");

struct Tables {
  uint64_t w[kTableWords];
};

// ---- exact integers for the table generator (compile time; 192 bits hold 5^63 < 2^147)
struct Big {
  uint64_t w[3];
};
constexpr Big big_pow5(int i) {
  Big b = {{1, 0, 0}};
  for (int k = 0; k < i; ++k) {
    uint64_t carry = 0;
    for (int l = 0; l < 3; ++l) {
      const u128 t = (u128)b.w[l] * 5u + carry;
      b.w[l] = (uint64_t)t;
      carry = (uint64_t)(t >> 64);
    }
  }
  return b;
}
constexpr int big_bits(const Big& b) {
  for (int l = 2; l >= 0; --l)
    for (int bit = 63; bit >= 0; --bit)
      if ((b.w[l] >> bit) & 1u) return 64 * l + bit + 1;
  return 0;
}
constexpr bool big_bit(const Big& b, int at) { return at >= 0 && at < 192 && ((b.w[at / 64] >> (at % 64)) & 1u); }
// bits [from, from + 128) of b, bit by bit; from may be negative (a left shift)
constexpr void big_window(const Big& b, int from, uint64_t* lo, uint64_t* hi) {
  uint64_t l = 0, h = 0;
  for (int k = 0; k < 64; ++k) {
    if (big_bit(b, from + k)) l |= (uint64_t)1 << k;
    if (big_bit(b, from + 64 + k)) h |= (uint64_t)1 << k;
  }
  *lo = l;
  *hi = h;
}
// floor(2^k / v) + 1 for v < 2^64, k < 192, as (lo, hi): the quotient is below 2^128 here
constexpr void pow2_over(int k, uint64_t v, uint64_t* lo, uint64_t* hi) {
  uint64_t q[3] = {0, 0, 0};
  u128 rem = 0;
  for (int l = 2; l >= 0; --l) {
    const uint64_t limb = (k / 64 == l) ? (uint64_t)1 << (k % 64) : 0;
    const u128 cur = (rem << 64) | limb;
    q[l] = (uint64_t)(cur / v);
    rem = cur % v;
  }
  const u128 r = (((u128)q[1] << 64) | q[0]) + 1u;
  *lo = (uint64_t)r;
  *hi = (uint64_t)(r >> 64);
}

// floor(log10(2^e)), floor(log10(5^e)) and bits(5^e) = ceil(log2(5^e)) (1 for e = 0) by fixed-point
// multiplication.  pow5_bits is compared with the exact powers below; the host check compares all three
// with exact decimal powers for every exponent of the range.
SE3DS_HD constexpr int log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }
SE3DS_HD constexpr int log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }
SE3DS_HD constexpr int pow5_bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }

constexpr Tables make_tables() {
  Tables t = {};
  for (int i = 0; i < kPow5Count; ++i) {
    const Big p = big_pow5(i);
    big_window(p, big_bits(p) - kPow5Bits, &t.w[2 * i], &t.w[2 * i + 1]);
  }
  for (int q = 0; q < kPow5InvCount; ++q) {
    const Big p = big_pow5(q);   // 5^20 < 2^47: one limb
    pow2_over(big_bits(p) - 1 + kPow5InvBits, p.w[0], &t.w[2 * (kPow5Count + q)], &t.w[2 * (kPow5Count + q) + 1]);
  }
  return t;
}

// the decimal exponent q and the table index of every e2 of the range stay inside the tables, the
// shifts of mul_shift stay in [64, 128), and pow5_bits is exact for every table entry
constexpr int kMinE2 = kMinBinaryExponent - 52 - 2, kMaxE2 = kMaxBinaryExponent - 52 - 2;
constexpr bool range_ok() {
  for (int i = 0; i < kPow5Count; ++i)
    if (pow5_bits(i) != big_bits(big_pow5(i))) return false;
  for (int e2 = kMinE2; e2 <= kMaxE2; ++e2) {
    if (e2 >= 0) {
      const int q = log10_pow2(e2) - (e2 > 3);
      if (q < 0 || q >= kPow5InvCount) return false;
      const int shift = -e2 + q + kPow5InvBits + pow5_bits(q) - 1;
      if (shift < 64 || shift >= 128) return false;
    } else {
      const int q = log10_pow5(-e2) - (-e2 > 1);
      const int i = -e2 - q;
      if (q < 0 || i < 0 || i >= kPow5Count) return false;
      const int shift = q - (pow5_bits(i) - kPow5Bits);
      if (shift < 64 || shift >= 128) return false;
    }
  }
  return true;
}
static_assert(range_ok(), "the tables do not cover the widened fp32 range");

// (m * mul) >> j for m < 2^56, mul < 2^126 given as (lo, hi), 64 <= j < 128; the result fits 64 bits
SE3DS_HD uint64_t mul_shift(uint64_t m, const uint64_t* mul, int j) {
  const u128 b0 = (u128)m * mul[0];
  const u128 b2 = (u128)m * mul[1];
  return (uint64_t)(((b0 >> 64) + b2) >> (j - 64));
}

SE3DS_HD bool multiple_of_pow5(uint64_t v, int p) {
  int count = 0;
  while (v != 0 && v % 5u == 0) {
    v /= 5u;
    ++count;
  }
  return count >= p;
}
SE3DS_HD bool multiple_of_pow2(uint64_t v, int p) { return p < 64 && (v & (((uint64_t)1 << p) - 1u)) == 0; }

SE3DS_HD int decimal_length(uint64_t v) {   // v < 10^17
  int n = 1;
  uint64_t p = 10;
  while (n < kMaxDigits && v >= p) {
    p *= 10u;
    ++n;
  }
  return n;
}

SE3DS_HD int leading_bit(uint32_t v) {   // v != 0
  int p = 0;
  for (int s = 16; s > 0; s >>= 1)
    if (v >> (p + s)) p += s;
  return p;
}

// characters of a finite record
SE3DS_HD uint32_t float_length(int d, int nd, bool negative) {
  uint32_t n = negative ? 1u : 0u;
  if (d >= -4 && d < 16) {
    if (d < 0) return n + 2u + (uint32_t)(-d - 1) + (uint32_t)nd;   // 0. zeros digits
    if (d >= nd - 1) return n + (uint32_t)(d + 1) + 2u;            // digits zeros .0
    return n + (uint32_t)nd + 1u;                                  // digits . digits
  }
  const int a = d < 0 ? -d : d;
  return n + (uint32_t)nd + (nd > 1 ? 1u : 0u) + 2u + (a >= 100 ? 3u : 2u);
}

// fp32 bits -> record.  tables: make_tables().w, in any memory
SE3DS_HD Record to_decimal(uint32_t f, const uint64_t* tables) {
  Record r;
  r.digits = 0;
  r.d = 0;
  r.ndigits = 1;
  const bool negative = (f >> 31) != 0;
  const uint32_t fe = (f >> 23) & 0xffu, fm = f & 0x7fffffu;
  if (fe == 0xffu) {
    r.cls = fm ? (uint8_t)kNan : (uint8_t)(kInf | (negative ? kNegative : 0));
    r.length = fm ? 3u : (negative ? 4u : 3u);
    return r;
  }
  r.cls = (uint8_t)(kFinite | (negative ? kNegative : 0));
  if (fe == 0 && fm == 0) {
    r.length = float_length(0, 1, negative);   // 0.0
    return r;
  }
  // widen: value = m2 * 2^(e2 + 2), 2^52 <= m2 < 2^53
  uint64_t m2;
  int e2;
  if (fe == 0) {
    const int p = leading_bit(fm);
    m2 = (uint64_t)fm << (52 - p);
    e2 = (p - 149) - 52 - 2;
  } else {
    m2 = ((uint64_t)1 << 52) | ((uint64_t)fm << 29);
    e2 = ((int)fe - 127) - 52 - 2;
  }
  const bool accept = (m2 & 1u) == 0;                       // round-to-even accepts the interval's ends
  const uint32_t mm_shift = (m2 & (((uint64_t)1 << 52) - 1u)) != 0 ? 1u : 0u;   // the lower gap is half at 2^k
  const uint64_t mv = 4u * m2;
  uint64_t vr, vp, vm;
  int e10;
  bool vm_zeros = false, vr_zeros = false;
  if (e2 >= 0) {
    const int q = log10_pow2(e2) - (e2 > 3);
    e10 = q;
    const int j = -e2 + q + kPow5InvBits + pow5_bits(q) - 1;
    const uint64_t* mul = tables + 2 * (kPow5Count + q);
    vr = mul_shift(mv, mul, j);
    vp = mul_shift(mv + 2u, mul, j);
    vm = mul_shift(mv - 1u - mm_shift, mul, j);
    if (q <= 21) {
      if (mv % 5u == 0) vr_zeros = multiple_of_pow5(mv, q);
      else if (accept) vm_zeros = multiple_of_pow5(mv - 1u - mm_shift, q);
      else vp -= multiple_of_pow5(mv + 2u, q) ? 1u : 0u;
    }
  } else {
    const int q = log10_pow5(-e2) - (-e2 > 1);
    e10 = q + e2;
    const int i = -e2 - q;
    const int j = q - (pow5_bits(i) - kPow5Bits);
    const uint64_t* mul = tables + 2 * i;
    vr = mul_shift(mv, mul, j);
    vp = mul_shift(mv + 2u, mul, j);
    vm = mul_shift(mv - 1u - mm_shift, mul, j);
    if (q <= 1) {
      vr_zeros = true;   // mv = 4 m2 has two trailing zero bits
      if (accept) vm_zeros = mm_shift == 1u;
      else --vp;
    } else if (q < 63) {
      vr_zeros = multiple_of_pow2(mv, q);
    }
  }
  int removed = 0;
  uint32_t last = 0;
  while (vp / 10u > vm / 10u) {
    vm_zeros = vm_zeros && vm % 10u == 0;
    vr_zeros = vr_zeros && last == 0;
    last = (uint32_t)(vr % 10u);
    vr /= 10u;
    vp /= 10u;
    vm /= 10u;
    ++removed;
  }
  if (vm_zeros) {
    while (vm % 10u == 0) {
      vr_zeros = vr_zeros && last == 0;
      last = (uint32_t)(vr % 10u);
      vr /= 10u;
      vp /= 10u;
      vm /= 10u;
      ++removed;
    }
  }
  if (vr_zeros && last == 5u && vr % 2u == 0) last = 4u;   // exactly half: to even
  const uint64_t out = vr + (((vr == vm && (!accept || !vm_zeros)) || last >= 5u) ? 1u : 0u);
  const int nd = decimal_length(out);
  r.digits = out;
  r.ndigits = (uint8_t)nd;
  r.d = (int16_t)(e10 + removed + nd - 1);
  r.length = float_length(r.d, nd, negative);
  return r;
}

// places digits v (nd of them) from the last to the first; digit j goes to at[j + (j >= point)]
SE3DS_HD void place_digits(uint64_t v, int nd, int point, char* at) {
  uint32_t lo = (uint32_t)(v % 1000000000u), hi = (uint32_t)(v / 1000000000u);   // hi < 10^8
  int j = nd - 1;
  for (int k = 0; k < 9 && j >= 0; ++k, --j) {
    at[j + (j >= point ? 1 : 0)] = (char)('0' + lo % 10u);
    lo /= 10u;
  }
  for (; j >= 0; --j) {
    at[j + (j >= point ? 1 : 0)] = (char)('0' + hi % 10u);
    hi /= 10u;
  }
}

// writes the text of r at out (r.length characters) and returns r.length
SE3DS_HD uint32_t write_float(const Record& r, char* out) {
  const int kind = r.cls & ~kNegative;
  char* p = out;
  if (kind == kNan) {
    p[0] = 'n'; p[1] = 'a'; p[2] = 'n';
    return 3u;
  }
  if (r.cls & kNegative) *p++ = '-';
  if (kind == kInf) {
    p[0] = 'i'; p[1] = 'n'; p[2] = 'f';
    return r.length;
  }
  const int d = r.d, nd = r.ndigits;
  if (d >= -4 && d < 16) {
    if (d < 0) {
      *p++ = '0';
      *p++ = '.';
      for (int k = 0; k < -d - 1; ++k) *p++ = '0';
      place_digits(r.digits, nd, nd, p);
    } else if (d >= nd - 1) {
      place_digits(r.digits, nd, nd, p);
      p += nd;
      for (int k = 0; k < d + 1 - nd; ++k) *p++ = '0';
      p[0] = '.';
      p[1] = '0';
    } else {
      place_digits(r.digits, nd, d + 1, p);
      p[d + 1] = '.';
    }
    return r.length;
  }
  place_digits(r.digits, nd, 1, p);
  if (nd > 1) p[1] = '.';
  p += nd + (nd > 1 ? 1 : 0);
  *p++ = 'e';
  *p++ = d < 0 ? '-' : '+';
  uint32_t a = (uint32_t)(d < 0 ? -d : d);
  if (a >= 100u) {
    *p++ = (char)('0' + a / 100u);
    a %= 100u;
  }
  p[0] = (char)('0' + a / 10u);
  p[1] = (char)('0' + a % 10u);
  return r.length;
}

// int32 as decimal text, the full range
SE3DS_HD uint32_t int_length(int32_t v) {
  uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  uint32_t n = v < 0 ? 2u : 1u;
  while (a >= 10u) {
    a /= 10u;
    ++n;
  }
  return n;
}
SE3DS_HD uint32_t write_int(int32_t v, char* out) {
  const uint32_t n = int_length(v);
  uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  if (v < 0) out[0] = '-';
  for (uint32_t k = n; k-- > (v < 0 ? 1u : 0u);) {
    out[k] = (char)('0' + a % 10u);
    a /= 10u;
  }
  return n;
}

// one line: at most kMaxLineBytes
SE3DS_HD uint32_t line_length(const Record* xyz, const int32_t* rgb) {
  uint32_t n = 1u;
  for (int k = 0; k < 3; ++k) n += xyz[k].length + 1u + int_length(rgb[k]) + 1u;
  return n;
}
SE3DS_HD uint32_t write_line(const Record* xyz, const int32_t* rgb, char* out) {
  char* p = out;
  for (int k = 0; k < 3; ++k) {
    p += write_float(xyz[k], p);
    *p++ = ' ';
  }
  for (int k = 0; k < 3; ++k) {
    p += write_int(rgb[k], p);
    *p++ = ' ';
  }
  *p++ = '\n';
  return (uint32_t)(p - out);
}

SE3DS_HD bool points_ok(int64_t m) { return m >= 0 && m <= kMaxPoints; }

}  // namespace ply
}  // namespace se3ds
