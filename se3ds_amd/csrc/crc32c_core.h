// Segmented CRC-32C (Castagnoli, reflected polynomial 0x82F63B78, init and final xor 0xffffffff; RFC
// 3720 B.4, tensorflow/core/lib/hash/crc32c.h) core.  One text for two builds: the kernels of
// crc32c.hip and a plain C++ program (tools/crc32c_host_check.cpp) that walks the same blocks, slices
// and combine order serially under the host sanitizers.  Everything is `__host__ __device__`;
// compiled without HIP it is ordinary C++.
//
// Arithmetic.  A CRC register is a polynomial over GF(2) modulo P, reflected: bit 31 is x^0, bit 0
// is x^31.  With a zero initial register the register after a message is linear in the message, so
//     raw(A || B) = raw(A) * x^(8 |B|)  ^  raw(B)   (mod P),
// and zero bytes in front of a message do not change it.  The initial 0xffffffff is the same as
// inverting the first four message bytes: the one slice that starts at the segment's first byte
// starts from 0xffffffff instead of 0; the final xor is a constant.
//
// Layout.  A segment of L bytes is cut FROM ITS END into blocks of kBlockBytes and every block into
// kLanes slices of kSliceBytes, so that the distance from the end of any slice to the end of the
// segment is (kLanes - 1 - lane) slices + m blocks -- a per-lane constant times a power of one
// constant -- and all raggedness sits at the segment's head, where a slice merely starts later.
// A lane runs the slicing-by-4 table CRC over its slice (bytes up to 4-byte alignment, words up to
// 16-byte alignment, 16-byte loads, words, bytes: every load lies inside the slice), carries it over
// consecutive blocks (acc = acc * x^(8 kBlockBytes) ^ raw), and multiplies by its lane constant; the
// xor over the lanes times x^(8 kBlockBytes m) is the run's share of the segment's CRC.  Shares
// combine by xor, which is exact and commutative: the result does not depend on their order.
//
// Two polynomials.  Everything that depends on P takes it as a template parameter whose default is
// Castagnoli, so the CRC-32C callers read as before.  The zip / zlib CRC-32 (kPolyZip, reflected
// 0xEDB88320) is the other instantiation; its table rows have a third field, a seed: the slice that
// starts at the range's first byte starts from ~seed, which continues zlib.crc32(prefix) over the
// range, and an empty range keeps its seed.
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
namespace crc32c {

constexpr uint32_t kPoly = 0x82F63B78u;
constexpr uint32_t kPolyZip = 0xEDB88320u;   // ISO 3309 / zlib / zip
constexpr uint32_t kOne = 0x80000000u;   // x^0
constexpr uint32_t kInit = 0xffffffffu;  // initial register and final xor
constexpr int kFields = 2;               // int64 per table row: byte offset, length
constexpr int kFieldsSeeded = 3;         // ... and the CRC of what precedes the range (0 .. 2^32 - 1)
constexpr int kLanes = 64;
constexpr int kSliceShift = 8;
constexpr int kSliceBytes = 1 << kSliceShift;
constexpr int kBlockShift = 14;
constexpr int kBlockBytes = 1 << kBlockShift;   // the work-splitting granule
constexpr int kTableWords = 4 * 256;            // slicing-by-4
static_assert(kBlockBytes == kLanes * kSliceBytes, "a block is one slice per lane");

template <uint32_t kP = kPoly>
SE3DS_HD constexpr uint32_t times_x(uint32_t a) { return (a >> 1) ^ (kP & (0u - (a & 1u))); }

// a * b mod P, 32 steps
template <uint32_t kP = kPoly>
SE3DS_HD constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = times_x<kP>(b);
  }
  return p;
}

// Word i of the slicing tables: table k = i >> 8 holds the register after byte i & 255 and k zero
// bytes.  Table 0 is the byte table.
template <uint32_t kP = kPoly>
SE3DS_HD constexpr uint32_t table_entry(int i) {
  uint32_t c = (uint32_t)(i & 255);
  for (int s = 8 * ((i >> 8) + 1); s > 0; --s) c = times_x<kP>(c);
  return c;
}

// v[k] = x^(8 * 2^k): the kernels take it by value as an argument.
struct Pow2 {
  uint32_t v[64];
};
template <uint32_t kP = kPoly>
SE3DS_HD constexpr Pow2 make_pow2() {
  Pow2 t{};
  t.v[0] = kOne >> 8;
  for (int k = 1; k < 64; ++k) t.v[k] = gf_mul<kP>(t.v[k - 1], t.v[k - 1]);
  return t;
}

// x^(8 n * 2^shift), n * 2^shift < 2^64: square-and-multiply over the set bits of n
template <uint32_t kP = kPoly>
SE3DS_HD uint32_t xpow8(uint64_t n, int shift, const Pow2& t) {
  uint32_t r = kOne;
  for (int k = shift; n != 0 && k < 64; ++k, n >>= 1)
    if (n & 1u) r = r == kOne ? t.v[k] : gf_mul<kP>(r, t.v[k]);
  return r;
}

// what the partial of `lane` is multiplied by: the slices behind it in its block
template <uint32_t kP = kPoly>
SE3DS_HD uint32_t lane_multiplier(int lane, const Pow2& t) {
  return xpow8<kP>((uint64_t)(kLanes - 1 - lane), kSliceShift, t);
}

SE3DS_HD int64_t block_count(int64_t len) {
  return len > 0 ? (int64_t)(((uint64_t)len + (uint64_t)(kBlockBytes - 1)) >> kBlockShift) : 0;
}

SE3DS_HD uint32_t step_byte(uint32_t c, uint8_t b, const uint32_t* t) { return t[(c ^ b) & 255u] ^ (c >> 8); }

SE3DS_HD uint32_t step_word(uint32_t c, uint32_t w, const uint32_t* t) {
  c ^= w;   // little-endian: the first byte is the low one
  return t[768 + (c & 255u)] ^ t[512 + ((c >> 8) & 255u)] ^ t[256 + ((c >> 16) & 255u)] ^ t[c >> 24];
}

struct Quad {
  uint32_t w[4];
};
SE3DS_HD uint32_t load_word(const uint8_t* p) {
  uint32_t w;
  memcpy(&w, __builtin_assume_aligned(p, 4), 4);
  return w;
}
SE3DS_HD Quad load_quad(const uint8_t* p) {
  Quad q;
  memcpy(&q, __builtin_assume_aligned(p, 16), 16);
  return q;
}

// The register after the n bytes at p, from register c.  Reads [p, p + n) and nothing else.
SE3DS_HD uint32_t slice_crc(const uint8_t* p, uint32_t n, uint32_t c, const uint32_t* t) {
  while (n != 0 && (reinterpret_cast<uintptr_t>(p) & 3u) != 0) {
    c = step_byte(c, *p, t);
    ++p, --n;
  }
  while (n >= 4 && (reinterpret_cast<uintptr_t>(p) & 15u) != 0) {
    c = step_word(c, load_word(p), t);
    p += 4, n -= 4;
  }
  while (n >= 128) {   // one 128-byte line in flight per lane before the first lookup
    Quad q[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) q[i] = load_quad(p + 16 * i);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 4; ++j) c = step_word(c, q[i].w[j], t);
    p += 128, n -= 128;
  }
  while (n >= 16) {
    const Quad q = load_quad(p);
    for (int j = 0; j < 4; ++j) c = step_word(c, q.w[j], t);
    p += 16, n -= 16;
  }
  while (n >= 4) {
    c = step_word(c, load_word(p), t);
    p += 4, n -= 4;
  }
  while (n != 0) {
    c = step_byte(c, *p, t);
    ++p, --n;
  }
  return c;
}

// Slice of `lane` in block c of a segment of len bytes in nb blocks: [begin, begin + n), n = 0 in
// front of the segment.
SE3DS_HD void slice_bounds(int64_t len, int64_t nb, int64_t c, int lane, int64_t* begin, uint32_t* n) {
  const int64_t end = len - (int64_t)((uint64_t)(nb - 1 - c) << kBlockShift) -
                      ((int64_t)(kLanes - 1 - lane) << kSliceShift);
  if (end <= 0) {
    *begin = 0, *n = 0;
    return;
  }
  const int64_t b = end > kSliceBytes ? end - kSliceBytes : 0;
  *begin = b, *n = (uint32_t)(end - b);
}

// One lane's share of blocks [c_lo, c_hi) of a segment, positioned at the end of block c_hi - 1.
// init: the register in front of the segment's first byte.
template <uint32_t kP = kPoly>
SE3DS_HD uint32_t lane_partial(const uint8_t* seg, int64_t len, int64_t nb, int64_t c_lo, int64_t c_hi,
                               int lane, uint32_t lane_mul, uint32_t init, const uint32_t* t, const Pow2& pw) {
  uint32_t acc = 0;
  for (int64_t c = c_lo; c < c_hi; ++c) {
    int64_t begin;
    uint32_t n;
    slice_bounds(len, nb, c, lane, &begin, &n);
    if (c != c_lo) acc = gf_mul<kP>(acc, pw.v[kBlockShift]);
    if (n != 0) acc ^= slice_crc(seg + begin, n, begin == 0 ? init : 0u, t);
  }
  return gf_mul<kP>(acc, lane_mul);
}

// Blocks [g0, g1) of the concatenated work of all segments.  prefix[s] = number of blocks in front
// of segment s, prefix[n] = all.  Policy: xor_lanes(f) = xor of f(lane) over the lanes,
// lane_multiplier(lane), emit(p, v): *p ^= v once.  The table is not trusted: a row that leaves
// [0, buf_bytes) or disagrees with prefix is skipped.  kF = kFieldsSeeded: the row's third field
// is its seed.
template <class Policy, uint32_t kP = kPoly, int kF = kFields>
SE3DS_HD void walk(const Policy& policy, const uint8_t* buf, int64_t buf_bytes, const int64_t* table,
                   const int64_t* prefix, int n, int64_t g0, int64_t g1, const uint32_t* t, const Pow2& pw,
                   uint32_t* crc) {
  if (g1 > prefix[n]) g1 = prefix[n];
  if (g0 < 0 || g0 >= g1) return;
  int lo = 0, hi = n;   // prefix[lo] <= g0 < prefix[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (prefix[mid] <= g0) lo = mid; else hi = mid;
  }
  int s = lo;
  int64_t g = g0;
  while (g < g1 && s < n) {
    const int64_t first = prefix[s], next = prefix[s + 1];
    if (next <= g) {   // an empty segment
      ++s;
      continue;
    }
    const int64_t off = table[(int64_t)s * kF], len = table[(int64_t)s * kF + 1];
    const int64_t nb = next - first;
    if (first <= g && off >= 0 && len > 0 && len <= buf_bytes && off <= buf_bytes - len &&
        block_count(len) == nb) {
      const int64_t c_lo = g - first, c_hi = g1 - first < nb ? g1 - first : nb;
      const uint8_t* seg = buf + off;
      const uint32_t init = kF == kFieldsSeeded ? ~(uint32_t)table[(int64_t)s * kF + (kF - 1)] : kInit;
      uint32_t v = policy.xor_lanes([&](int lane) {
        return lane_partial<kP>(seg, len, nb, c_lo, c_hi, lane, policy.lane_multiplier(lane), init, t, pw);
      });
      if (nb != c_hi) v = gf_mul<kP>(v, xpow8<kP>((uint64_t)(nb - c_hi), kBlockShift, pw));
      policy.emit(crc + s, v);
    }
    g = next < g1 ? next : g1;
    ++s;
  }
}

}  // namespace crc32c
}  // namespace se3ds
