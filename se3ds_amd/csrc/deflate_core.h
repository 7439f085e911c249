// PNG filtering (ISO/IEC 15948 section 9) and a deflate (RFC 1951) encoder core for one strip of
// scan lines, written from the two specifications.  One encoder for two builds, as inflate_core.h:
// the 64-lane kernel of png_encode.hip and a plain C++ program (tools/deflate_host_check.cpp) that
// runs the same code under the host sanitizers.  Compiled without HIP it is ordinary C++.
//
// A strip is at most 65535 filtered bytes (filter-type byte + residuals per scan line), so it always
// fits one stored block.  It becomes one dynamic-Huffman block over literals and runs -- a run is a
// match of distance 1, length 3..258, taken greedily -- or, when that would not be smaller, one
// stored block; then an empty stored block, which ends the strip on a byte boundary and carries
// BFINAL for the last strip of an image.  Strips are independent: concatenated they are one deflate
// stream.
//
// The lanes of a policy work in lock step.  What has width is strided over the lanes: the filters
// and their cost sums, the Adler-32 partial sums, the sort of the used symbols by frequency, the
// search for the end of a run, the copy of a stored block.  The token scan is serial in its
// symbols, so every lane walks it with the same state (wave-uniform control flow) and lane 0
// stores; the Huffman merge and the length limit (286 symbols against tens of KiB of data) run in
// lane 0 alone.  With HostPolicy (one lane) all of it is the serial twin, bit for bit.
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
namespace deflate {

constexpr uint32_t kMaxStripBytes = 65535;   // one stored block
constexpr uint32_t kDataBytes = 65536;       // the strip buffer
constexpr uint32_t kStripOverhead = 10;      // stored header + the empty stored block behind it
constexpr uint32_t kAdlerMod = 65521;
constexpr int kSymbols = 286;
constexpr int kMaxBits = 15;
constexpr uint32_t kEndOfBlock = 256;
constexpr uint32_t kMaxRun = 258;
constexpr uint32_t kFilterAdaptive = 5;      // filter modes 0..4 are the PNG filter types

// rows of a full strip of an image with row_bytes bytes per row (row_bytes <= 65534)
SE3DS_HD uint32_t strip_rows(uint32_t row_bytes) {
  const uint32_t r = kMaxStripBytes / (1u + row_bytes);
  return r < 1u ? 1u : r;
}

// Adler-32 of a concatenation from the sums of its parts (RFC 1950: s1 = 1 + sum of the bytes,
// s2 = sum of the running s1): (a1, a2) over the first part, (b1, b2) over len_b further bytes.
SE3DS_HD void adler_combine(uint32_t a1, uint32_t a2, uint32_t b1, uint32_t b2, uint64_t len_b,
                            uint32_t* s1, uint32_t* s2) {
  const uint64_t rem = len_b % kAdlerMod;
  *s1 = (uint32_t)((a1 + b1 + kAdlerMod - 1u) % kAdlerMod);
  *s2 = (uint32_t)((a2 + b2 + rem * ((a1 + kAdlerMod - 1u) % kAdlerMod)) % kAdlerMod);
}

// The encoder's working memory: LDS in the kernel, an ordinary object on the host.
struct Shared {
  alignas(16) uint8_t data[kDataBytes];   // the strip's filtered bytes
  uint32_t freq[kSymbols];
  uint32_t weight[2 * kSymbols];          // tree nodes: the sorted leaves, then the merges
  uint16_t parent[2 * kSymbols];
  uint16_t depth[2 * kSymbols];
  uint16_t sorted[kSymbols];              // used symbols by (frequency, symbol), ascending
  uint16_t code[kSymbols];                // bit-reversed canonical code words
  uint16_t num[kMaxBits + 1];             // symbols per code length
  uint8_t len[kSymbols];
  uint32_t nlit;                          // literal/length code lengths in the header
  uint32_t body_bits;                     // sum of frequency x code length
};

struct HostPolicy {
  static constexpr int kLanes = 1;
  int lane() const { return 0; }
  void sync() const {}
  uint32_t sum(uint32_t v) const { return v; }
  uint32_t min(uint32_t v) const { return v; }
};

SE3DS_HD uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  int pa = p - (int)a, pb = p - (int)b, pc = p - (int)c;
  pa = pa < 0 ? -pa : pa;
  pb = pb < 0 ? -pb : pb;
  pc = pc < 0 ? -pc : pc;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// |int8(v)| of a residual byte
SE3DS_HD uint32_t cost(uint32_t v) { return v < 128u ? v : 256u - v; }

template <class Policy>
class Encoder {
 public:
  // out: the strip's slot, 4-byte aligned, room for kStripOverhead + the strip's filtered bytes.
  SE3DS_HD Encoder(const Policy& policy, Shared& shared, uint8_t* out) : p_(policy), s_(shared), out_(out) {}

  // Rows [row0, row0 + rows) of a dense image (height x row_bytes bytes, bpp bytes per pixel) ->
  // s_.data, rows x (1 + row_bytes) <= kMaxStripBytes bytes.  mode 0..4: that filter type on every
  // row; kFilterAdaptive: per row the type with the smallest sum of |int8(residual)|, ties to the
  // lowest type.  The row above row0 is read from the image.  Returns the byte count.
  // swap16: the image holds 16-bit samples in host (little-endian) order and bpp is 2; what is
  // filtered is the big-endian byte sequence PNG stores: file byte x of a row is memory byte x ^ 1
  // (row_bytes is even, so x ^ 1 stays inside the row).
  SE3DS_HD uint32_t filter(const uint8_t* image, uint32_t row_bytes, uint32_t bpp, uint32_t mode,
                           uint32_t row0, uint32_t rows, bool swap16 = false) {
    const uint32_t flip = swap16 ? 1u : 0u;
    const uint32_t lane = (uint32_t)p_.lane();
    const uint32_t pitch = 1u + row_bytes;
    p_.sync();   // the lanes are done with the previous strip
    for (uint32_t r = 0; r < rows; ++r) {
      const uint8_t* cur = image + (uint64_t)(row0 + r) * row_bytes;
      const uint8_t* up = row0 + r > 0 ? cur - row_bytes : nullptr;
      uint32_t type = mode;
      if (mode == kFilterAdaptive) {
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t x = lane; x < row_bytes; x += Policy::kLanes) {
          uint32_t res[5];
          residuals(cur, up, x, bpp, flip, res);
          for (int t = 0; t < 5; ++t) sum[t] += cost(res[t]);   // < 2^32: 65534 x 128
        }
        type = 0;
        uint32_t best = p_.sum(sum[0]);
        for (uint32_t t = 1; t < 5; ++t) {
          const uint32_t v = p_.sum(sum[t]);
          if (v < best) {
            best = v;
            type = t;
          }
        }
      }
      uint8_t* dst = s_.data + r * pitch;
      if (lane == 0) dst[0] = (uint8_t)type;
      for (uint32_t x = lane; x < row_bytes; x += Policy::kLanes) {
        uint32_t res[5];
        residuals(cur, up, x, bpp, flip, res);
        dst[1 + x] = (uint8_t)res[type];
      }
    }
    p_.sync();
    return rows * pitch;
  }

  // s_.data[0, n), n <= kMaxStripBytes -> out: the strip's blocks.  Returns the byte count, at most
  // kStripOverhead + n; s1() / s2() are the Adler-32 sums of the n bytes.
  SE3DS_HD uint32_t compress(uint32_t n, bool final_strip) {
    const uint32_t lane = (uint32_t)p_.lane();
    p_.sync();
    adler(n);
    for (uint32_t i = lane; i < (uint32_t)kSymbols; i += Policy::kLanes) {
      s_.freq[i] = 0;
      s_.len[i] = 0;
    }
    p_.sync();
    extra_bits_ = 0;
    scan<false>(n);
    if (lane == 0) {
      s_.freq[kEndOfBlock] = 1;
      if (n == 0) s_.freq[0] = 1;   // a second symbol: a one-symbol code would be incomplete
    }
    p_.sync();
    build_code();
    const uint32_t header_bits = 3 + 5 + 5 + 4 + 19 * 3 + 4 * (s_.nlit + 1);
    const uint64_t bits = (uint64_t)header_bits + s_.body_bits + extra_bits_ + 3;
    const uint64_t coded = (bits + 7) / 8 + 4;
    acc_ = 0;
    cnt_ = 0;
    pos_ = 0;
    if (coded < (uint64_t)kStripOverhead + n) {
      header();
      scan<true>(n);
      put(s_.code[kEndOfBlock], s_.len[kEndOfBlock]);
    } else {
      put(0, 3);   // BFINAL 0, BTYPE 00
      align();
      put(n, 16);
      put(~n & 0xffffu, 16);
      flush_bytes();
      for (uint32_t i = lane; i < n; i += Policy::kLanes) out_[pos_ + i] = s_.data[i];
      pos_ += n;
    }
    put(final_strip ? 1u : 0u, 3);   // the empty stored block
    align();
    put(0, 16);
    put(0xffffu, 16);
    flush_bytes();
    return pos_;
  }

  SE3DS_HD uint32_t s1() const { return s1_; }
  SE3DS_HD uint32_t s2() const { return s2_; }

 private:
  // the five residuals of byte x of a row: a = the byte one pixel to the left, b = the byte above,
  // c = the byte above-left, all 0 outside the image.  x counts file bytes; flip (0 or 1) is xor-ed
  // into every memory index (filter(): swap16)
  SE3DS_HD static void residuals(const uint8_t* cur, const uint8_t* up, uint32_t x, uint32_t bpp,
                                 uint32_t flip, uint32_t (&res)[5]) {
    const uint32_t v = cur[x ^ flip];
    const uint32_t a = x >= bpp ? cur[(x - bpp) ^ flip] : 0u;
    const uint32_t b = up ? up[x ^ flip] : 0u;
    const uint32_t c = (up && x >= bpp) ? up[(x - bpp) ^ flip] : 0u;
    res[0] = v;
    res[1] = (v - a) & 0xffu;
    res[2] = (v - b) & 0xffu;
    res[3] = (v - ((a + b) >> 1)) & 0xffu;
    res[4] = (v - paeth(a, b, c)) & 0xffu;
  }

  SE3DS_HD void adler(uint32_t n) {
    // per lane: the byte sum (< 2^24) and the sum weighted by the distance to the end, kept mod
    // 65521; no term exceeds 65535 x 255 < 2^24
    uint32_t sa = 0, sb = 0;
    for (uint32_t q = (uint32_t)p_.lane(); q < n; q += Policy::kLanes) {
      const uint32_t v = s_.data[q];
      sa += v;
      sb = (sb + (n - q) * v) % kAdlerMod;
    }
    sa = p_.sum(sa);
    sb = p_.sum(sb);
    s1_ = (1u + sa) % kAdlerMod;
    s2_ = (n + sb) % kAdlerMod;
  }

  // bytes from position i on that equal v, at most kMaxRun and not past n; data[i] == v
  SE3DS_HD uint32_t run_length(uint32_t i, uint32_t n, uint32_t v) const {
    const uint32_t limit = n - i < kMaxRun ? n - i : kMaxRun;
    for (uint32_t base = 0; base < limit; base += Policy::kLanes) {
      const uint32_t k = base + (uint32_t)p_.lane();
      uint32_t miss = (k < limit && s_.data[i + k] == v) ? 0xffffffffu : k;
      miss = p_.min(miss);
      if (miss != 0xffffffffu) return miss < limit ? miss : limit;
    }
    return limit;
  }

  // RFC 1951 3.2.5 as arithmetic: 8 codes without extra bits, then 4 codes per extra bit, 285 = 258
  SE3DS_HD static void length_symbol(uint32_t len, uint32_t* sym, uint32_t* ebits, uint32_t* extra) {
    const uint32_t x = len - 3;
    if (x < 8) {
      *sym = 257 + x;
      *ebits = 0;
      *extra = 0;
    } else if (len == kMaxRun) {
      *sym = 285;
      *ebits = 0;
      *extra = 0;
    } else {
      uint32_t e = 1;
      while ((x >> (e + 3)) != 0) ++e;   // floor(log2 x) - 2
      *sym = 257 + 4 * e + 4 + ((x >> e) - 4);
      *ebits = e;
      *extra = x & ((1u << e) - 1u);
    }
  }

  // The token walk: a literal, or -- when the byte repeats the one before it at least three times
  // over -- a match of distance 1.  EMIT false: frequencies and extra bits; true: the code words.
  template <bool EMIT>
  SE3DS_HD void scan(uint32_t n) {
    const bool first = p_.lane() == 0;
    uint32_t i = 0;
    while (i < n) {
      const uint32_t v = s_.data[i];
      if (i > 0 && v == s_.data[i - 1]) {
        const uint32_t len = run_length(i, n, v);
        if (len >= 3) {
          uint32_t sym, ebits, extra;
          length_symbol(len, &sym, &ebits, &extra);
          if (EMIT) {
            // code word, extra bits, then the one-bit distance code 0
            const uint32_t l = s_.len[sym];
            put((uint32_t)s_.code[sym] | (extra << l), l + ebits + 1);
          } else {
            if (first) ++s_.freq[sym];
            extra_bits_ += ebits + 1;
          }
          i += len;
          continue;
        }
      }
      if (EMIT) {
        put(s_.code[v], s_.len[v]);
      } else if (first) {
        ++s_.freq[v];
      }
      ++i;
    }
  }

  // freq -> len, code, nlit, body_bits
  SE3DS_HD void build_code() {
    const uint32_t lane = (uint32_t)p_.lane();
    uint32_t used = 0;
    for (uint32_t i = lane; i < (uint32_t)kSymbols; i += Policy::kLanes) {
      const uint32_t f = s_.freq[i];
      if (f == 0) continue;
      ++used;
      uint32_t rank = 0;
      for (uint32_t j = 0; j < (uint32_t)kSymbols; ++j) {
        const uint32_t g = s_.freq[j];
        rank += (g != 0 && (g < f || (g == f && j < i))) ? 1u : 0u;
      }
      s_.sorted[rank] = (uint16_t)i;
    }
    used = p_.sum(used);   // >= 2
    p_.sync();
    if (lane == 0) limited_lengths(used);
    p_.sync();
  }

  // One lane: the Huffman merge over the sorted leaves (two queues), the depths, the limit to
  // kMaxBits by the Kraft sum, the canonical code words.
  SE3DS_HD void limited_lengths(uint32_t m) {
    for (uint32_t k = 0; k < m; ++k) s_.weight[k] = s_.freq[s_.sorted[k]];
    uint32_t leaf = 0, inner = m, next = m;
    while (next < 2 * m - 1) {
      uint32_t pick[2];
      for (int t = 0; t < 2; ++t) {
        if (leaf < m && (inner >= next || s_.weight[leaf] <= s_.weight[inner])) pick[t] = leaf++;
        else pick[t] = inner++;
      }
      s_.weight[next] = s_.weight[pick[0]] + s_.weight[pick[1]];
      s_.parent[pick[0]] = (uint16_t)next;
      s_.parent[pick[1]] = (uint16_t)next;
      ++next;
    }
    const uint32_t root = 2 * m - 2;
    s_.depth[root] = 0;
    for (uint32_t k = root; k-- > 0;) s_.depth[k] = (uint16_t)(s_.depth[s_.parent[k]] + 1);
    for (int l = 0; l <= kMaxBits; ++l) s_.num[l] = 0;
    for (uint32_t k = 0; k < m; ++k) {
      const uint32_t d = s_.depth[k];
      ++s_.num[d > (uint32_t)kMaxBits ? (uint32_t)kMaxBits : d];
    }
    // Cutting the deep leaves to kMaxBits over-subscribes the code.  Each round takes one leaf
    // from the longest length and lengthens one shorter leaf, whose sibling place the first takes:
    // the Kraft sum, in units of 2^-kMaxBits, drops by one until it is 2^kMaxBits again.
    uint32_t total = 0;
    for (int l = 1; l <= kMaxBits; ++l) total += (uint32_t)s_.num[l] << (kMaxBits - l);
    while (total > (1u << kMaxBits)) {
      --s_.num[kMaxBits];
      for (int l = kMaxBits - 1; l > 0; --l) {
        if (s_.num[l]) {
          --s_.num[l];
          s_.num[l + 1] = (uint16_t)(s_.num[l + 1] + 2);
          break;
        }
      }
      --total;
    }
    // the shortest lengths to the most frequent symbols
    uint32_t j = m;
    for (int l = 1; l <= kMaxBits; ++l)
      for (uint32_t c = s_.num[l]; c > 0; --c) s_.len[s_.sorted[--j]] = (uint8_t)l;
    // canonical code words (RFC 1951 3.2.2), stored bit-reversed: Huffman codes go out from their
    // most significant bit
    uint32_t next_code[kMaxBits + 1];
    uint32_t code = 0;
    for (int l = 1; l <= kMaxBits; ++l) {
      next_code[l] = code;
      code = (code + s_.num[l]) << 1;
    }
    uint32_t nlit = 257, body = 0;
    for (uint32_t i = 0; i < (uint32_t)kSymbols; ++i) {
      const uint32_t l = s_.len[i];
      if (l == 0) continue;
      uint32_t c = next_code[l]++, rev = 0;
      for (uint32_t b = 0; b < l; ++b) {
        rev = (rev << 1) | (c & 1u);
        c >>= 1;
      }
      s_.code[i] = (uint16_t)rev;
      body += s_.freq[i] * l;
      if (i + 1 > nlit) nlit = i + 1;
    }
    s_.nlit = nlit;
    s_.body_bits = body;
  }

  // The dynamic block's header with the fixed code-length code: symbols 0..15 at 4 bits (symbol s
  // is the code word s), 16 / 17 / 18 unused; one distance code, 0, at length 1.
  SE3DS_HD void header() {
    put(0, 1);   // BFINAL: the empty stored block behind the strip carries it
    put(2, 2);   // BTYPE 10
    put(s_.nlit - 257, 5);
    put(0, 5);    // HDIST: 1 code
    put(15, 4);   // HCLEN: all 19 code-length code lengths, in the order 16 17 18 0 8 7 ...
    put(0, 9);    // 16, 17, 18
    for (int i = 0; i < 16; ++i) put(4, 3);
    for (uint32_t i = 0; i < s_.nlit; ++i) put(rev4(s_.len[i]), 4);
    put(rev4(1), 4);   // the distance code
  }

  SE3DS_HD static uint32_t rev4(uint32_t v) {
    return ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1) | ((v & 8u) >> 3);
  }

  // ------------------------------------------------------------------------------ bit writer
  SE3DS_HD void put(uint32_t bits, uint32_t n) {   // n <= 32, bits < 2^n
    acc_ |= (uint64_t)bits << cnt_;
    cnt_ += n;
    if (cnt_ >= 32) {
      if (p_.lane() == 0) {
        const uint32_t w = (uint32_t)acc_;
        if ((pos_ & 3u) == 0) {
          memcpy(__builtin_assume_aligned(out_ + pos_, 4), &w, 4);
        } else {
          for (uint32_t k = 0; k < 4; ++k) out_[pos_ + k] = (uint8_t)(w >> (8 * k));
        }
      }
      pos_ += 4;
      acc_ >>= 32;
      cnt_ -= 32;
    }
  }

  SE3DS_HD void align() { cnt_ = (cnt_ + 7u) & ~7u; }

  SE3DS_HD void flush_bytes() {   // after align(): whole bytes only
    while (cnt_ >= 8) {
      if (p_.lane() == 0) out_[pos_] = (uint8_t)acc_;
      ++pos_;
      acc_ >>= 8;
      cnt_ -= 8;
    }
  }

  const Policy& p_;
  Shared& s_;
  uint8_t* out_;
  uint64_t acc_ = 0;
  uint32_t cnt_ = 0, pos_ = 0;
  uint32_t extra_bits_ = 0;
  uint32_t s1_ = 1, s2_ = 0;
};

}  // namespace deflate
}  // namespace se3ds
