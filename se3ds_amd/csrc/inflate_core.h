// zlib (RFC 1950) / deflate (RFC 1951) decoder core, written from the two specifications.  One
// decoder for two builds: the 64-lane kernel of inflate.hip and a plain C++ program
// (tools/inflate_host_check.cpp) that runs the same code under the host sanitizers.  Everything is
// `__host__ __device__`; compiled without HIP it is ordinary C++.
//
// A stream is decoded by `Policy::kLanes` lanes in lock step: every lane holds the same bit-reader
// state and decodes the same symbol (control flow is uniform), and the work with data parallelism
// in it is strided over the lanes -- the input chunk fetch, the table build, the match copy, the
// ring flush with its Adler-32 partial sums and filter-type check, the zero fill after a failure.
// The policy supplies the lane index, the lane count, the barrier and the two reductions.  With
// HostPolicy (one lane, no barrier, identity reductions) the strided loops become the serial twin.
//
// Memory safety does not depend on the stream: the compressed length and the expected inflated
// length come from the caller's table; past the end the bit reader yields zeros and the stream ends
// as TRUNCATED; every ring index is masked; an output byte beyond the expected length is TOO_LONG
// before it is written; a match may not reach before the first output byte.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SE3DS_HD __host__ __device__ inline
#else
#define SE3DS_HD inline
#endif

namespace se3ds {
namespace inflate {

// One int32 per stream: the code in the low 8 bits.  BAD_FILTER alone carries a detail above it:
// bits 8-15 the offending filter-type byte, bits 16-30 its row (saturating at 32767).
enum class Status : int32_t {
  OK = 0,
  TRUNCATED = 1,          // the input ended inside the stream or its trailer
  BAD_HEADER = 2,         // zlib header: CM != 8, CINFO > 7, FCHECK wrong or FDICT set
  BAD_BLOCK_TYPE = 3,     // BTYPE 3
  BAD_STORED_LENGTH = 4,  // LEN != ~NLEN
  BAD_COUNTS = 5,         // HLIT > 286 or HDIST > 30 symbols
  OVER_SUBSCRIBED = 6,    // a set of code lengths that no prefix code has
  INCOMPLETE = 7,         // an incomplete set other than the two RFC 1951 3.2.7 allows for distances
  BAD_REPEAT = 8,         // repeat code without a previous length, or past HLIT + HDIST
  NO_END_OF_BLOCK = 9,    // symbol 256 has no code
  BAD_CODE = 10,          // bits that are no code word; literal/length 286, 287; distance 30, 31
  BAD_DISTANCE = 11,      // a distance beyond the bytes produced so far
  TOO_LONG = 12,          // more bytes than the geometry holds
  TOO_SHORT = 13,         // fewer
  BAD_ADLER = 14,         // the trailer does not match the inflated bytes
  BAD_FILTER = 15,        // a scan line starts with a filter type above 4
};

constexpr uint32_t kRingBytes = 65536;   // the 32 KiB window + one flush granule + a match, rounded up
constexpr uint32_t kRingMask = kRingBytes - 1;
constexpr uint32_t kGranule = 16384;     // flush unit; bounds the terms of the Adler-32 sums
constexpr uint32_t kInChunk = 1024;      // compressed bytes staged at a time
constexpr int kFastBits = 10;            // codes up to this length decode with one table read
constexpr int kMaxSymbols = 320;         // 286 + 30 code lengths of a dynamic header, rounded up
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kMaxStreamBytes = 0x7fffffffu;   // compressed and inflated lengths fit in 31 bits

// A canonical prefix code: count / first code / offset into `sorted` per length (RFC 1951 3.2.2),
// and a direct table over the next kFastBits input bits: (symbol << 4) | length, 0 = not that short.
struct Table {
  uint16_t fast[1 << kFastBits];
  uint16_t sorted[kMaxSymbols];
  uint16_t count[16];
  uint16_t first[16];
  uint16_t offs[16];
};

// The decoder's working memory: LDS in the kernel, an ordinary object on the host.
struct Shared {
  alignas(16) uint8_t ring[kRingBytes];
  alignas(16) uint8_t in[kInChunk];
  uint8_t lens[kMaxSymbols];
  Table clen, lit, dist, fixed_lit, fixed_dist;
};

struct HostPolicy {
  static constexpr int kLanes = 1;
  int lane() const { return 0; }
  void sync() const {}
  uint32_t sum(uint32_t v) const { return v; }
  uint32_t min(uint32_t v) const { return v; }
};

template <class Policy>
class Inflater {
 public:
  // in: in_len compressed bytes (zlib framing).  out: room for `expected` bytes = rows of `pitch`
  // bytes (filter-type byte + filtered bytes).  All three sizes <= kMaxStreamBytes, pitch >= 1.
  SE3DS_HD Inflater(const Policy& policy, Shared& shared, const uint8_t* in, uint32_t in_len, uint8_t* out,
                    uint32_t expected, uint32_t pitch)
      : p_(policy), s_(shared), in_(in), in_len_(in_len), out_(out), expected_(expected), pitch_(pitch) {}

  // Decodes the stream; every lane returns the same status word.
  SE3DS_HD int32_t run() {
    Status st = decode_stream();
    if (st != Status::OK) zero_fill(flushed_);
    int32_t word = (int32_t)st;
    if (st == Status::BAD_FILTER) word |= (int32_t)bad_filter_;
    return word;
  }

 private:
  enum class Kind { CodeLengths, LitLen, Dist };

  // ------------------------------------------------------------------------------ bit reader
  SE3DS_HD void fetch(uint32_t base) {
    p_.sync();   // the lanes are done with the previous chunk
    for (uint32_t i = (uint32_t)p_.lane(); i < kInChunk; i += Policy::kLanes) {
      const uint32_t q = base + i;   // <= 2^31 + 8 + kInChunk: no wrap
      s_.in[i] = q < in_len_ ? in_[q] : (uint8_t)0;
    }
    chunk_base_ = base;
    p_.sync();
  }

  SE3DS_HD uint32_t next_byte() {
    uint32_t off = in_pos_ - chunk_base_;   // wraps to a huge value when in_pos_ was rewound below the chunk
    if (off >= kInChunk) {
      fetch(in_pos_);
      off = 0;
    }
    ++in_pos_;   // counts on past the end: ran_out() compares it with in_len_
    return s_.in[off];
  }

  SE3DS_HD void refill() {   // at least 57 bits: one length / distance pair needs 48
    while (bitcnt_ <= 56) {
      bitbuf_ |= (uint64_t)next_byte() << bitcnt_;
      bitcnt_ += 8;
    }
  }

  SE3DS_HD void drop(uint32_t n) {
    bitbuf_ >>= n;
    bitcnt_ -= n;
  }

  SE3DS_HD uint32_t bits(uint32_t n) {   // n <= 32, after a refill()
    const uint32_t v = (uint32_t)(bitbuf_ & ((1ull << n) - 1));
    drop(n);
    return v;
  }

  // bytes of the stream touched by the bits consumed so far; beyond in_len_ they were made up
  SE3DS_HD bool ran_out() const { return in_pos_ - (bitcnt_ >> 3) > in_len_; }

  // real (not made up) bits waiting in the buffer
  SE3DS_HD uint32_t real_bits() const {
    const uint32_t phantom = in_pos_ > in_len_ ? (in_pos_ - in_len_) * 8 : 0;
    return bitcnt_ > phantom ? bitcnt_ - phantom : 0;
  }

  SE3DS_HD Status fail(Status st) const { return ran_out() ? Status::TRUNCATED : st; }

  // ------------------------------------------------------------------------------ tables
  // lens[0, n) -> t.  Cooperative: a lane per code length counts and sorts, then every lane decodes
  // its share of the 2^kFastBits possible inputs canonically.
  SE3DS_HD Status build(Table& t, const uint8_t* lens, int n, Kind kind) {
    const int lane = p_.lane();
    p_.sync();   // lens is written
    for (int l = lane; l < 16; l += Policy::kLanes) {
      uint32_t c = 0;
      if (l > 0)
        for (int i = 0; i < n; ++i) c += lens[i] == l;
      t.count[l] = (uint16_t)c;
    }
    p_.sync();
    int left = 1;   // code words still free at this length
    uint32_t code = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
      const uint32_t c = t.count[l];
      left = 2 * left - (int)c;
      if (left < 0) return Status::OVER_SUBSCRIBED;
      if (lane == 0) {
        t.first[l] = (uint16_t)code;
        t.offs[l] = (uint16_t)index;
      }
      code = (code + c) << 1;
      index += c;
    }
    if (left > 0) {
      const bool allowed = kind == Kind::Dist && (index == 0 || (index == 1 && t.count[1] == 1));
      if (!allowed) return Status::INCOMPLETE;
    }
    p_.sync();
    for (int l = 1 + lane; l < 16; l += Policy::kLanes) {
      uint32_t k = t.offs[l];
      for (int i = 0; i < n; ++i)
        if (lens[i] == l) t.sorted[k++] = (uint16_t)i;
    }
    p_.sync();
    for (uint32_t idx = (uint32_t)lane; idx < (1u << kFastBits); idx += Policy::kLanes) {
      uint32_t entry = 0, c = 0;
      for (int l = 1; l <= kFastBits; ++l) {
        c = (c << 1) | ((idx >> (l - 1)) & 1u);
        const uint32_t first = t.first[l];
        if (c >= first && c - first < t.count[l]) {
          entry = ((uint32_t)t.sorted[t.offs[l] + (c - first)] << 4) | (uint32_t)l;
          break;
        }
      }
      t.fast[idx] = (uint16_t)entry;
    }
    p_.sync();
    return Status::OK;
  }

  // The next symbol, or -1 when the next bits are no code word.  After a refill().
  SE3DS_HD int decode(const Table& t) {
    const uint32_t e = t.fast[(uint32_t)bitbuf_ & ((1u << kFastBits) - 1)];
    if (e & 15u) {
      drop(e & 15u);
      return (int)(e >> 4);
    }
    uint32_t c = 0;
    for (int l = 1; l < 16; ++l) {
      c = (c << 1) | ((uint32_t)(bitbuf_ >> (l - 1)) & 1u);
      const uint32_t first = t.first[l];
      if (c >= first && c - first < t.count[l]) {
        drop((uint32_t)l);
        return (int)t.sorted[t.offs[l] + (c - first)];
      }
    }
    return -1;
  }

  // A failed decode() is a truncation when fewer real bits were left than the longest code has.
  SE3DS_HD Status bad_code() const {
    return (ran_out() || real_bits() < 15) ? Status::TRUNCATED : Status::BAD_CODE;
  }

  SE3DS_HD Status build_fixed() {
    if (fixed_ready_) return Status::OK;
    for (int i = p_.lane(); i < 288; i += Policy::kLanes)
      s_.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    Status st = build(s_.fixed_lit, s_.lens, 288, Kind::LitLen);
    if (st != Status::OK) return st;
    p_.sync();
    for (int i = p_.lane(); i < 32; i += Policy::kLanes) s_.lens[i] = 5;
    st = build(s_.fixed_dist, s_.lens, 32, Kind::Dist);
    fixed_ready_ = st == Status::OK;
    return st;
  }

  SE3DS_HD Status build_dynamic() {
    static constexpr uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int lane = p_.lane();
    refill();
    const int nlit = (int)bits(5) + 257, ndist = (int)bits(5) + 1, nclen = (int)bits(4) + 4;
    if (ran_out()) return Status::TRUNCATED;
    if (nlit > 286 || ndist > 30) return Status::BAD_COUNTS;
    p_.sync();
    for (int i = lane; i < 19; i += Policy::kLanes) s_.lens[i] = 0;
    p_.sync();
    for (int i = 0; i < nclen; ++i) {
      refill();
      const uint32_t v = bits(3);
      if (lane == 0) s_.lens[kOrder[i]] = (uint8_t)v;
    }
    if (ran_out()) return Status::TRUNCATED;
    Status st = build(s_.clen, s_.lens, 19, Kind::CodeLengths);
    if (st != Status::OK) return st;
    const int total = nlit + ndist;
    int i = 0;
    uint32_t prev = 0;
    while (i < total) {
      refill();
      const int sym = decode(s_.clen);
      if (sym < 0) return bad_code();
      uint32_t value = 0;
      int run = 1;
      if (sym < 16) {
        value = (uint32_t)sym;
      } else if (sym == 16) {
        if (i == 0) return fail(Status::BAD_REPEAT);
        value = prev;
        run = 3 + (int)bits(2);
      } else if (sym == 17) {
        run = 3 + (int)bits(3);
      } else {
        run = 11 + (int)bits(7);
      }
      if (ran_out()) return Status::TRUNCATED;
      if (run > total - i) return Status::BAD_REPEAT;
      for (int k = lane; k < run; k += Policy::kLanes) s_.lens[i + k] = (uint8_t)value;
      i += run;
      prev = value;
    }
    p_.sync();
    if (s_.lens[256] == 0) return Status::NO_END_OF_BLOCK;
    st = build(s_.lit, s_.lens, nlit, Kind::LitLen);
    if (st != Status::OK) return st;
    return build(s_.dist, s_.lens + nlit, ndist, Kind::Dist);
  }

  // ------------------------------------------------------------------------------ output
  // Ring bytes [a, b) -> out, with the Adler-32 update and the filter-type check.  a is a multiple
  // of kGranule, b - a <= kGranule.
  SE3DS_HD void flush(uint32_t a, uint32_t b) {
    p_.sync();
    const uint32_t lane = (uint32_t)p_.lane();
    // this lane's byte sum (< 2^23) and its sum weighted by the distance to b, kept mod 65521: with
    // b - a <= kGranule no term exceeds 2^27, whatever the number of lanes
    uint32_t sa = 0, sb = 0;
    const bool aligned = (reinterpret_cast<uintptr_t>(out_) & 15u) == 0;
    const uint32_t n16 = aligned ? (b - a) >> 4 : 0;
    for (uint32_t c = lane; c < n16; c += Policy::kLanes) {
      const uint32_t q = a + (c << 4);
      uint8_t v[16];
      memcpy(v, &s_.ring[q & kRingMask], 16);
      memcpy(__builtin_assume_aligned(out_ + q, 16), v, 16);
      uint32_t a16 = 0, b16 = 0;
      for (uint32_t j = 0; j < 16; ++j) {
        a16 += v[j];
        b16 += (16 - j) * v[j];
      }
      sa += a16;
      sb = (sb + (b - q - 16) * a16 + b16) % kAdlerMod;
    }
    for (uint32_t q = a + (n16 << 4) + lane; q < b; q += Policy::kLanes) {
      const uint32_t v = s_.ring[q & kRingMask];
      out_[q] = (uint8_t)v;
      sa += v;
      sb = (sb + (b - q) * v) % kAdlerMod;
    }
    // the scan lines that start inside [a, b)
    uint32_t worst = 0xffffffffu;
    for (uint64_t r = (a + (uint64_t)pitch_ - 1) / pitch_ + lane; r * pitch_ < b; r += Policy::kLanes)
      if (s_.ring[(uint32_t)(r * pitch_) & kRingMask] > 4 && (uint32_t)r < worst) worst = (uint32_t)r;
    worst = p_.min(worst);
    if (worst != 0xffffffffu && bad_filter_ == 0) {
      const uint32_t v = s_.ring[(uint32_t)((uint64_t)worst * pitch_) & kRingMask];
      bad_filter_ = (v << 8) | ((worst > 32767u ? 32767u : worst) << 16);
    }
    sa = p_.sum(sa);
    sb = p_.sum(sb);
    const uint32_t n = b - a;
    s2_ = (s2_ + (n * s1_) % kAdlerMod + sb) % kAdlerMod;
    s1_ = (s1_ + sa) % kAdlerMod;
  }

  SE3DS_HD void flush_full_granules() {
    while (pos_ - flushed_ >= kGranule) {
      flush(flushed_, flushed_ + kGranule);
      flushed_ += kGranule;
    }
  }

  SE3DS_HD void zero_fill(uint32_t from) {
    for (uint32_t q = from + (uint32_t)p_.lane(); q < expected_; q += Policy::kLanes) out_[q] = 0;
  }

  // ------------------------------------------------------------------------------ blocks
  SE3DS_HD Status stored_block() {
    drop(bitcnt_ & 7u);
    refill();
    const uint32_t len = bits(16), nlen = bits(16);
    if (ran_out()) return Status::TRUNCATED;
    if (len != (~nlen & 0xffffu)) return Status::BAD_STORED_LENGTH;
    in_pos_ -= bitcnt_ >> 3;   // whole unread bytes go back; not past in_len_, nothing ran out
    bitbuf_ = 0;
    bitcnt_ = 0;
    if (len > in_len_ - in_pos_) return Status::TRUNCATED;
    if (len > expected_ - pos_) return Status::TOO_LONG;
    uint32_t left = len;
    while (left > 0) {
      const uint32_t room = kGranule - (pos_ - flushed_);   // >= 1
      const uint32_t n = left < room ? left : room;
      for (uint32_t i = (uint32_t)p_.lane(); i < n; i += Policy::kLanes)
        s_.ring[(pos_ + i) & kRingMask] = in_[in_pos_ + i];
      pos_ += n;
      in_pos_ += n;
      left -= n;
      flush_full_granules();
    }
    return Status::OK;
  }

  SE3DS_HD Status coded_block(const Table& lit, const Table& dist) {
    const uint32_t lane = (uint32_t)p_.lane();
    for (;;) {
      refill();
      const int sym = decode(lit);
      if (sym < 0) return bad_code();
      if (sym < 256) {
        if (ran_out()) return Status::TRUNCATED;
        if (pos_ >= expected_) return Status::TOO_LONG;
        if (lane == 0) s_.ring[pos_ & kRingMask] = (uint8_t)sym;
        ++pos_;
        flush_full_granules();
        continue;
      }
      if (sym == 256) return ran_out() ? Status::TRUNCATED : Status::OK;
      if (sym > 285) return fail(Status::BAD_CODE);
      // RFC 1951 3.2.5 as arithmetic: 8 codes without extra bits, then 4 codes per extra bit
      const uint32_t lc = (uint32_t)sym - 257;
      uint32_t len;
      if (lc < 8) {
        len = 3 + lc;
      } else if (lc == 28) {
        len = 258;
      } else {
        const uint32_t e = (lc - 4) >> 2;
        len = 3 + ((4 + (lc & 3)) << e) + bits(e);
      }
      const int dsym = decode(dist);
      if (dsym < 0) return bad_code();
      if (dsym > 29) return fail(Status::BAD_CODE);
      const uint32_t dc = (uint32_t)dsym;
      uint32_t d;
      if (dc < 4) {
        d = 1 + dc;
      } else {
        const uint32_t e = (dc - 2) >> 1;
        d = 1 + ((2 + (dc & 1)) << e) + bits(e);
      }
      if (ran_out()) return Status::TRUNCATED;
      if (d > pos_) return Status::BAD_DISTANCE;
      if (len > expected_ - pos_) return Status::TOO_LONG;
      // byte i of the match is byte i mod d of the d bytes before pos_: every source byte is older
      // than the match, so an overlapping match (d < len) needs no ordering between the lanes
      p_.sync();
      const uint32_t src = pos_ - d;
      if (d >= len) {
        for (uint32_t i = lane; i < len; i += Policy::kLanes)
          s_.ring[(pos_ + i) & kRingMask] = s_.ring[(src + i) & kRingMask];
      } else {
        for (uint32_t i = lane; i < len; i += Policy::kLanes)
          s_.ring[(pos_ + i) & kRingMask] = s_.ring[(src + i % d) & kRingMask];
      }
      pos_ += len;
      flush_full_granules();
    }
  }

  SE3DS_HD Status decode_stream() {
    fetch(0);
    refill();
    const uint32_t cmf = bits(8), flg = bits(8);
    if (ran_out()) return Status::TRUNCATED;
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20u))
      return Status::BAD_HEADER;
    uint32_t last = 0;
    while (!last) {
      refill();
      last = bits(1);
      const uint32_t type = bits(2);
      if (ran_out()) return Status::TRUNCATED;
      Status st;
      if (type == 0) {
        st = stored_block();
      } else if (type == 1) {
        st = build_fixed();
        if (st == Status::OK) st = coded_block(s_.fixed_lit, s_.fixed_dist);
      } else if (type == 2) {
        st = build_dynamic();
        if (st == Status::OK) st = coded_block(s_.lit, s_.dist);
      } else {
        st = Status::BAD_BLOCK_TYPE;
      }
      if (st != Status::OK) return st;
    }
    if (pos_ > flushed_) flush(flushed_, pos_);
    flushed_ = pos_;
    drop(bitcnt_ & 7u);
    refill();
    const uint32_t b0 = bits(8), b1 = bits(8), b2 = bits(8), b3 = bits(8);
    if (ran_out()) return Status::TRUNCATED;
    if (((b0 << 24) | (b1 << 16) | (b2 << 8) | b3) != ((s2_ << 16) | s1_)) return Status::BAD_ADLER;
    if (pos_ != expected_) return Status::TOO_SHORT;
    if (bad_filter_) return Status::BAD_FILTER;
    return Status::OK;
  }

  const Policy& p_;
  Shared& s_;
  const uint8_t* in_;
  const uint32_t in_len_;
  uint8_t* out_;
  const uint32_t expected_, pitch_;
  uint64_t bitbuf_ = 0;
  uint32_t bitcnt_ = 0, in_pos_ = 0, chunk_base_ = 0;
  uint32_t pos_ = 0, flushed_ = 0;   // bytes produced / bytes written to out_
  uint32_t s1_ = 1, s2_ = 0;         // Adler-32 of out_[0, flushed_)
  uint32_t bad_filter_ = 0;          // the detail bits of the first bad filter type seen, 0 = none
  bool fixed_ready_ = false;
};

}  // namespace inflate
}  // namespace se3ds
