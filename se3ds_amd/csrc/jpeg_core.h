// Baseline JPEG (ITU-T T.81, sequential DCT, Huffman, 8 bit) decoder core, written from the
// recommendation.  One core for two builds: the kernels of jpeg.hip and a plain C++ program
// (tools/jpeg_host_check.cpp) that runs the same code under the host sanitizers.  Everything is
// `__host__ __device__`; compiled without HIP it is ordinary C++.
//
// Entropy decode.  An entropy segment (a restart interval, or the whole scan) is one serial Huffman
// stream, but JPEG's prefix codes re-synchronise: a decoder that starts at a wrong bit, or in a wrong
// place of the block structure, usually falls into step with the true one after a few symbols.  So a
// segment is decoded by LANES lanes speculatively and the result is then proven consistent:
//
//   The segment is walked in windows of LANES x CHUNK raw bytes, staged in `Shared::win`.  Lane i owns
//   chunk i and decodes every symbol (code word + extra bits) that STARTS in it.  A decoder state is
//   (bit position in the raw bytes, block slot within the MCU, zig-zag index k); `FF 00` stuffing is
//   skipped inline, so positions count raw bytes, and a position never rests on a stuffed 00.
//   round 0    lane 0 enters with the true state carried over from the window before; lane i > 0
//              guesses (chunk start, slot 0, k 0).  A lane records its exit state, the blocks it
//              completed and the sum of the DC differences per component (the summary).
//   round r    lane i > 0 takes the exit state its predecessor had after round r - 1 (two buffers);
//              if that is not the entry it last used it decodes its chunk again.
//   stop       when a round >= 1 changed no exit state: then summary_i = f_i(exit_{i-1}) for every
//              lane and lane 0's entry is true, so every summary is true by induction.  After round r
//              lanes 0..r hold true summaries, so at most (active lanes + 1) rounds run; the loop
//              carries that bound.  Lanes whose chunk begins at or behind the segment's end take no
//              part.
//   write      an exclusive scan of (blocks, DC sums) over the lanes plus the window's carry gives
//              each lane its first block and its DC predictors; it decodes its chunk once more from
//              its true entry and writes de-zig-zagged int16 coefficients, DC accumulated.  A block
//              that straddles chunks is written by several lanes: the caller zeroes the coefficients
//              first.  Only this pass reports errors, and it stops at the segment's block count.
//
// Memory safety does not depend on the stream.  A lane starts a symbol only in front of its chunk's
// end, a fetch reads the 16 bytes from the aligned word its position lies in (a symbol spans at most 5
// data bytes = 10 raw bytes), a position moves at most 8 raw bytes past a symbol's start, and the
// window is staged with kSlack bytes behind it, zero past the segment's end.  Bits that are no code word count as 16 bits, a run
// is clamped at coefficient 63, a DC category at 11.  Coefficients are written only for block
// indices below the segment's count.
//
// The later phases are per-element functions: `idct_block` (dequantise + the 8 x 8 "slow integer"
// inverse DCT with 13-bit constants, saturating) and `pixel` (fancy h2v1 / h2v2 upsampling, colour
// conversion, crop).  All arithmetic is uint32 / wrapping: no signed overflow.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SE3DS_HD __host__ __device__ inline
#else
#define SE3DS_HD inline
#endif

namespace se3ds {
namespace jpeg {

// One int32 per segment: the code in the low 8 bits, the rounds of all its windows (saturating) in
// bits 8-30.
enum class Status : int32_t {
  OK = 0,
  TRUNCATED = 1,   // the bits ran out before the last block
  BAD_CODE = 2,    // bits that are no code word
  BAD_RUN = 3,     // a run or ZRL past coefficient 63
  BAD_DC = 4,      // DC category above 11
  TOO_LONG = 5,    // entropy bytes behind the segment's last block
};

constexpr int kLanes = 256;        // lanes (= chunks) per window in the kernel
constexpr int kChunkBytes = 128;   // raw bytes per chunk in the kernel
constexpr int kSlack = 28;         // staged behind the window: what a fetch behind the last symbol reads
constexpr int kLookBits = 9;       // code words up to this length decode with one table read
constexpr int kScanGroup = 16;     // lanes per group of the two-level scan
constexpr int kImageFields = 200;  // int64 per image row
constexpr int kSegmentFields = 5;  // int64 per segment row: image, byte offset, length, first MCU, MCUs
constexpr int64_t kMaxSegmentBytes = 1 << 28;   // bit positions fit in 31 bits
constexpr uint32_t kMaxRounds = (1u << 23) - 1;

// One row of the image table, kImageFields int64 wide.
struct Image {
  int64_t width, height;
  int64_t ncomp;              // 1 or 3
  int64_t h0, v0;             // sampling of component 0 (1 or 2 each); the others are 1 x 1
  int64_t dst;                // device pointer: height x width x out_channels uint8, dense
  int64_t out_channels;       // 1 or 3
  int64_t coef_off;           // workspace offset of the coefficients: int16 [blocks][64], scan order
  int64_t plane_off;          // workspace offset of the padded component planes
  int64_t seg_first, seg_count;
  int64_t mcus_x, mcus_y;
  int64_t tables;             // bit c: DC table of component c; bit 4 + c: its AC table
  int64_t reserved[2];
  uint16_t quant[3][64];      // per component, natural (row-major) order
  uint8_t huff[4][272];       // DC 0, DC 1, AC 0, AC 1: 16 counts (BITS), then the values (HUFFVAL)
};
static_assert(sizeof(Image) == kImageFields * 8, "image row");

SE3DS_HD int slots_of(const Image& im) { return im.ncomp == 1 ? 1 : (int)(im.h0 * im.v0) + 2; }
SE3DS_HD int64_t blocks_of(const Image& im) { return im.mcus_x * im.mcus_y * slots_of(im); }
SE3DS_HD int comp_h(const Image& im, int c) { return c == 0 ? (int)im.h0 : 1; }
SE3DS_HD int comp_v(const Image& im, int c) { return c == 0 ? (int)im.v0 : 1; }
SE3DS_HD int64_t plane_w(const Image& im, int c) { return im.mcus_x * comp_h(im, c) * 8; }
SE3DS_HD int64_t plane_h(const Image& im, int c) { return im.mcus_y * comp_v(im, c) * 8; }
SE3DS_HD int64_t coef_bytes(const Image& im) { return blocks_of(im) * 128; }
SE3DS_HD int64_t plane_bytes(const Image& im) {
  int64_t n = 0;
  for (int c = 0; c < (int)im.ncomp; ++c) n += plane_w(im, c) * plane_h(im, c);
  return n;
}

// A canonical prefix code (T.81 Annex C): per length the first code, the count and the offset into
// the values, and a direct table over the next kLookBits bits: (length << 8) | value, 0 = longer.
struct Huff {
  uint16_t look[1 << kLookBits];
  uint32_t first[17];
  uint32_t limit[17];   // (first + count) << (16 - length): 16 bits below it hold a code this short
  uint32_t delta[17];   // offs - first: index of a code's value = code + delta
  uint16_t count[17];
  uint16_t offs[17];
  uint8_t vals[256];
};

struct State {
  uint32_t pos;   // bit position in the segment's raw bytes
  uint32_t sk;    // (slot << 8) | k
};
SE3DS_HD bool same(State a, State b) { return a.pos == b.pos && a.sk == b.sk; }

// The decoder's working memory: LDS in the kernel, an ordinary object on the host.
template <int LANES, int CHUNK>
struct Shared {
  static_assert(CHUNK >= 16 && CHUNK % 4 == 0, "a symbol must not span a whole chunk");
  static constexpr uint32_t kWindow = (uint32_t)LANES * CHUNK;
  static constexpr uint32_t kStaged = kWindow + kSlack + 4;   // + 4: the source's misalignment
  alignas(16) uint8_t win[kStaged];
  Huff huff[4];
  State exit[2][LANES];
  State used[LANES];
  uint32_t blocks[LANES];   // the summary; after the scan the exclusive prefix, carry included
  uint32_t dc[3][LANES];
  uint32_t err[LANES];
  uint32_t group[(LANES + kScanGroup - 1) / kScanGroup][4];   // the scan's group totals, then offsets
  State carry;
  uint32_t carry_blocks, carry_dc[3], rounds, status, done;
};

// ---- the policies' contract: each(f) runs f(lane) for every lane and then synchronises; any(f)
// does the same and returns the OR of the results to every lane.  The kernel's policy is in
// jpeg.hip; this one simulates the lanes one after the other.
template <int LANES>
struct HostPolicy {
  template <class F> void each(F f) const {
    for (int lane = 0; lane < LANES; ++lane) f(lane);
  }
  template <class F> bool any(F f) const {
    bool r = false;
    for (int lane = 0; lane < LANES; ++lane) r = f(lane) || r;
    return r;
  }
};

SE3DS_HD uint32_t load32(const void* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
SE3DS_HD void store32(void* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// Canonical code of table t from the image's counts: the serial part, one lane per table.
SE3DS_HD void huff_prepare(Huff& h, const uint8_t* spec) {
  uint32_t code = 0, at = 0;
  h.first[0] = h.limit[0] = h.delta[0] = 0;
  h.count[0] = 0;
  h.offs[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const uint32_t n = spec[l - 1];
    h.first[l] = code;
    h.limit[l] = (code + n) << (16 - l);
    h.delta[l] = at - code;
    h.count[l] = (uint16_t)n;
    h.offs[l] = (uint16_t)at;
    code = (code + n) << 1;
    at += n;
  }
}

// The code word at the top of `bits16` among lengths lo..hi: (length << 8) | value, 0 = none.
SE3DS_HD uint32_t huff_search(const Huff& h, uint32_t bits16, int lo, int hi) {
  for (int l = lo; l <= hi; ++l) {
    const uint32_t d = (bits16 >> (16 - l)) - h.first[l];
    if (d < h.count[l]) return ((uint32_t)l << 8) | h.vals[(h.offs[l] + d) & 255u];
  }
  return 0;
}

// A code longer than kLookBits: its length is the first whose limit lies above the bits.  No loop
// with an exit: in a wave some lane takes this path at almost every symbol, so it is kept to
// independent reads.
SE3DS_HD uint32_t huff_long(const Huff& h, uint32_t bits16) {
  uint32_t l = kLookBits + 1;
  for (int j = kLookBits + 1; j < 16; ++j) l += bits16 >= h.limit[j] ? 1u : 0u;
  if (bits16 >= h.limit[16]) return 0;
  return (l << 8) | h.vals[((bits16 >> (16 - l)) + h.delta[l]) & 255u];
}

SE3DS_HD uint32_t huff_decode(const Huff& h, uint32_t bits16) {
  const uint32_t e = h.look[bits16 >> (16 - kLookBits)];
  return e ? e : huff_long(h, bits16);
}

SE3DS_HD int32_t extend(uint32_t v, uint32_t t) {   // T.81 F.2.2.1 EXTEND
  if (t == 0) return 0;
  return v >= (1u << (t - 1)) ? (int32_t)v : (int32_t)v - (int32_t)((1u << t) - 1);
}

template <int LANES, int CHUNK>
struct Decoder {
  using Sh = Shared<LANES, CHUNK>;
  Sh& sh;
  const Image& im;
  const uint8_t* src;   // the segment's raw bytes
  uint32_t len;         // their count, <= kMaxSegmentBytes
  int16_t* coef;        // the segment's first block
  uint32_t total;       // its block count
  int nslots, ny;
  uint32_t mis;         // src & 3: win[r - w0 + mis] is raw byte r
  uint32_t tables;      // Image::tables

  SE3DS_HD Decoder(Sh& s, const Image& image, const uint8_t* bytes, uint32_t n, int16_t* out,
                   uint32_t blocks)
      : sh(s), im(image), src(bytes), len(n), coef(out), total(blocks) {
    nslots = slots_of(im);
    ny = nslots == 1 ? 1 : nslots - 2;
    mis = (uint32_t)(reinterpret_cast<uintptr_t>(bytes) & 3u);
    tables = (uint32_t)im.tables;
  }

  // ---- phases (each takes the lane index)
  SE3DS_HD void tables_serial(int lane) {
    for (int t = lane; t < 4; t += LANES) {
      huff_prepare(sh.huff[t], im.huff[t]);
      for (int i = 0; i < 256; ++i) sh.huff[t].vals[i] = im.huff[t][16 + i];
    }
    if (lane == 0) {
      sh.carry.pos = 0;
      sh.carry.sk = 0;
      sh.carry_blocks = 0;
      sh.carry_dc[0] = sh.carry_dc[1] = sh.carry_dc[2] = 0;
      sh.rounds = 0;
      sh.status = 0;
      sh.done = 0;
    }
  }
  SE3DS_HD void tables_look(int lane) {
    for (int i = lane; i < 4 << kLookBits; i += LANES) {
      Huff& h = sh.huff[i >> kLookBits];
      const uint32_t x = (uint32_t)i & ((1u << kLookBits) - 1);
      h.look[x] = (uint16_t)huff_search(h, x << (16 - kLookBits), 1, kLookBits);
    }
  }

  // Raw bytes [w0 - mis, w0 - mis + kStaged) of the segment into win, zero outside [0, len).
  SE3DS_HD void stage(int lane, uint32_t w0) {
    for (uint32_t j = (uint32_t)lane; j < Sh::kStaged / 4; j += LANES) {
      const int64_t r0 = (int64_t)w0 + 4 * (int64_t)j - (int64_t)mis;
      uint32_t v = 0;
      if (r0 >= 0 && r0 + 4 <= (int64_t)len) {
        v = load32(src + r0);
      } else {
        for (int b = 0; b < 4; ++b) {
          const int64_t r = r0 + b;
          if (r >= 0 && r < (int64_t)len) v |= (uint32_t)src[r] << (8 * b);
        }
      }
      store32(sh.win + 4 * j, v);
    }
  }

  // 32 bits from bit `pos` on, stuffing skipped; bias = mis - w0.  *ends: nibble j = the raw bytes
  // that j data bytes take.  The bits come from at most 5 data bytes = 10 raw bytes: four aligned
  // words are read at once and the stuffed zeros are squeezed out in registers -- in a wave some lane
  // meets an FF at most symbols, so that path must not go back to memory byte by byte.
  SE3DS_HD uint32_t peek32(uint32_t pos, uint32_t bias, uint32_t* ends) const {
    const uint32_t idx = (pos >> 3) + bias, o = (idx & 3u) * 8;
    const uint8_t* at = sh.win + (idx & ~3u);
    const uint64_t a = ((uint64_t)__builtin_bswap32(load32(at)) << 32) | __builtin_bswap32(load32(at + 4));
    const uint64_t b = ((uint64_t)__builtin_bswap32(load32(at + 8)) << 32) | __builtin_bswap32(load32(at + 12));
    uint64_t x0 = o ? (a << o) | (b >> (64 - o)) : a, x1 = b << o;   // raw bytes idx .. idx + 15 - o / 8
    const uint64_t y = ~x0 | 0x0000000000FFFFFFull;   // a zero byte among the top five <=> an FF there
    if (((y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull) == 0) {
      *ends = 0x543210u;
      return (uint32_t)((x0 << (pos & 7u)) >> 32);
    }
    uint64_t acc = 0;
    uint32_t cum = 0, e = 0;
    for (int j = 1; j <= 5; ++j) {
      const uint32_t top = (uint32_t)(x0 >> 48);   // two raw bytes
      acc = (acc << 8) | (top >> 8);
      const uint32_t s = top == 0xFF00u ? 16u : 8u;
      cum += s >> 3;
      e |= cum << (4 * j);
      x0 = (x0 << s) | (x1 >> (64 - s));
      x1 <<= s;
    }
    *ends = e;
    return (uint32_t)(acc >> (8 - (pos & 7u)));
  }
  // The position `n` bits behind `pos`, given peek32's *ends for pos.
  SE3DS_HD uint32_t advance(uint32_t pos, uint32_t n, uint32_t ends) const {
    const uint32_t bit = (pos & 7u) + n;
    return (((pos >> 3) + ((ends >> (4 * (bit >> 3))) & 15u)) << 3) + (bit & 7u);
  }

  // `pos` rounded up to the next whole data byte, stuffing skipped: where bytes behind the padding
  // of the last block's byte would begin.
  SE3DS_HD uint32_t padded(uint32_t pos, uint32_t bias) const {
    if ((pos & 7u) == 0) return pos;
    uint32_t ends;
    peek32(pos, bias, &ends);
    return advance(pos, 8 - (pos & 7u), ends);
  }

  struct Result {
    State exit;
    uint32_t blocks;
    uint32_t dc[3];
    uint32_t err;
  };

  // Decodes the symbols that start in [st.pos, lim).  WRITE: coefficients go out, from block `blk`
  // with predictors `pred`, and the first error stops the lane.
  template <bool WRITE>
  SE3DS_HD Result decode_chunk(State st, uint32_t lim, uint32_t w0, uint32_t blk,
                               const uint32_t* pred) const {
    static constexpr uint8_t kNatural[64] = {
        0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const uint32_t bias = mis - w0, end = len * 8;
    Result r;
    r.blocks = 0;
    r.err = 0;
    r.dc[0] = r.dc[1] = r.dc[2] = 0;
    uint32_t p[3] = {0, 0, 0};
    if (WRITE) {
      p[0] = pred[0];
      p[1] = pred[1];
      p[2] = pred[2];
    }
    uint32_t pos = st.pos, slot = st.sk >> 8, k = st.sk & 255u;
    if (WRITE && blk >= total) {
      // a lane that enters behind the last block: the last symbol may have ended inside its first
      // byte, and the padding of that byte is no error (the same rule as behind the last block below)
      if (pos < lim && padded(pos, bias) < end) r.err = (uint32_t)Status::TOO_LONG;
      r.exit = st;
      return r;
    }
    // every symbol takes at least one bit: CHUNK * 8 symbols at the most
    for (int it = 0; it < CHUNK * 8 && pos < lim; ++it) {
      const uint32_t comp = slot < (uint32_t)ny ? 0u : slot - (uint32_t)ny + 1u;
      uint32_t ends;
      const uint32_t bits = peek32(pos, bias, &ends);
      uint32_t err = 0, used;
      if (k == 0) {
        uint32_t e = huff_decode(sh.huff[(tables >> comp) & 1u], bits >> 16);
        if (!e) {
          err = (uint32_t)Status::BAD_CODE;
          e = 16u << 8;
        }
        uint32_t l = e >> 8, t = e & 255u;
        if (t > 11) {
          err = err ? err : (uint32_t)Status::BAD_DC;
          t = 11;
        }
        const uint32_t raw = t ? (bits << l) >> (32 - t) : 0u;
        const uint32_t v = (uint32_t)extend(raw, t);
        // (selects, not indexed arrays: the sums stay in registers)
        r.dc[0] += comp == 0 ? v : 0u;
        r.dc[1] += comp == 1 ? v : 0u;
        r.dc[2] += comp == 2 ? v : 0u;
        used = l + t;
        if (WRITE && !err) {
          p[0] += comp == 0 ? v : 0u;
          p[1] += comp == 1 ? v : 0u;
          p[2] += comp == 2 ? v : 0u;
          coef[(int64_t)blk * 64] = (int16_t)(uint16_t)(comp == 0 ? p[0] : comp == 1 ? p[1] : p[2]);
        }
        k = 1;
      } else {
        uint32_t e = huff_decode(sh.huff[2u + ((tables >> (4u + comp)) & 1u)], bits >> 16);
        if (!e) {
          err = (uint32_t)Status::BAD_CODE;
          e = 16u << 8;
        }
        const uint32_t l = e >> 8, run = (e >> 4) & 15u, s = e & 15u;
        used = l + s;
        if (s == 0) {
          if (run == 15) {
            k += 16;
            if (k > 64) {
              err = err ? err : (uint32_t)Status::BAD_RUN;
              k = 64;
            }
          } else {
            k = 64;   // EOB
          }
        } else {
          k += run;
          if (k > 63) {
            err = err ? err : (uint32_t)Status::BAD_RUN;
            k = 63;
          }
          const int32_t v = extend((bits << l) >> (32 - s), s);
          if (WRITE && !err) coef[(int64_t)blk * 64 + kNatural[k]] = (int16_t)v;
          k += 1;
        }
      }
      pos = advance(pos, used, ends);
      if (WRITE) {
        if (!err && pos > end) err = (uint32_t)Status::TRUNCATED;
        if (err) {
          r.err = err;
          break;
        }
      }
      if (k >= 64) {
        k = 0;
        slot = slot + 1 == (uint32_t)nslots ? 0u : slot + 1;
        r.blocks += 1;
        if (WRITE) {
          blk += 1;
          if (blk == total) {
            // the last block: what may follow is the padding of its byte, nothing more
            if (padded(pos, bias) < end) r.err = (uint32_t)Status::TOO_LONG;
            break;
          }
        }
      }
    }
    r.exit.pos = pos;
    r.exit.sk = (slot << 8) | k;
    return r;
  }

  SE3DS_HD uint32_t active(uint32_t w0) const {
    const uint32_t left = len - w0, n = (left + CHUNK - 1) / CHUNK;
    return n < (uint32_t)LANES ? n : (uint32_t)LANES;
  }
  SE3DS_HD uint32_t chunk_lim(int lane, uint32_t w0) const {
    const uint32_t e = (w0 + (uint32_t)(lane + 1) * CHUNK) * 8, end = len * 8;
    return e < end ? e : end;
  }
  SE3DS_HD void keep(int lane, const Result& r, int buffer) {
    sh.exit[buffer][lane] = r.exit;
    sh.blocks[lane] = r.blocks;
    sh.dc[0][lane] = r.dc[0];
    sh.dc[1][lane] = r.dc[1];
    sh.dc[2][lane] = r.dc[2];
  }

  SE3DS_HD void round0(int lane, uint32_t w0) {
    if ((uint32_t)lane >= active(w0)) return;
    State entry;
    if (lane == 0) {
      entry = sh.carry;
    } else {
      entry.pos = (w0 + (uint32_t)lane * CHUNK) * 8;
      entry.sk = 0;
    }
    sh.used[lane] = entry;
    keep(lane, decode_chunk<false>(entry, chunk_lim(lane, w0), w0, 0, nullptr), 0);
  }

  // -> whether this lane's exit state changed
  SE3DS_HD bool round_n(int lane, uint32_t w0, uint32_t r) {
    if ((uint32_t)lane >= active(w0)) return false;
    const int cur = (int)(r & 1u), prev = cur ^ 1;
    const State before = sh.exit[prev][lane];
    if (lane == 0) {
      sh.exit[cur][0] = before;
      return false;
    }
    const State entry = sh.exit[prev][lane - 1];
    if (same(entry, sh.used[lane])) {
      sh.exit[cur][lane] = before;
      return false;
    }
    sh.used[lane] = entry;
    keep(lane, decode_chunk<false>(entry, chunk_lim(lane, w0), w0, 0, nullptr), cur);
    return !same(sh.exit[cur][lane], before);
  }

  // The exclusive scan of the summaries in three steps: a lane per group of kScanGroup lanes scans
  // its group in place and leaves the group's totals; lane 0 scans the totals, carry included, and
  // moves the carry on; every lane adds its group's offset.  `final` = the buffer that holds the
  // proven exit states.
  SE3DS_HD void scan_groups(int lane, uint32_t w0) {
    const uint32_t n = active(w0), from = (uint32_t)lane * kScanGroup;
    if (from >= n) return;
    const uint32_t to = from + kScanGroup < n ? from + kScanGroup : n;
    uint32_t b = 0, d0 = 0, d1 = 0, d2 = 0;
    for (uint32_t i = from; i < to; ++i) {
      const uint32_t nb = sh.blocks[i], e0 = sh.dc[0][i], e1 = sh.dc[1][i], e2 = sh.dc[2][i];
      sh.blocks[i] = b;
      sh.dc[0][i] = d0;
      sh.dc[1][i] = d1;
      sh.dc[2][i] = d2;
      b += nb;
      d0 += e0;
      d1 += e1;
      d2 += e2;
    }
    sh.group[lane][0] = b;
    sh.group[lane][1] = d0;
    sh.group[lane][2] = d1;
    sh.group[lane][3] = d2;
  }
  SE3DS_HD void scan_totals(int lane, uint32_t w0, int final, uint32_t rounds) {
    if (lane != 0) return;
    const uint32_t n = active(w0), groups = (n + kScanGroup - 1) / kScanGroup;
    uint32_t t[4] = {sh.carry_blocks, sh.carry_dc[0], sh.carry_dc[1], sh.carry_dc[2]};
    for (uint32_t g = 0; g < groups; ++g)
      for (int j = 0; j < 4; ++j) {
        const uint32_t v = sh.group[g][j];
        sh.group[g][j] = t[j];
        t[j] += v;
      }
    sh.carry_blocks = t[0];
    sh.carry_dc[0] = t[1];
    sh.carry_dc[1] = t[2];
    sh.carry_dc[2] = t[3];
    sh.carry = sh.exit[final][n - 1];
    const uint32_t sum = sh.rounds + rounds;
    sh.rounds = sum > kMaxRounds ? kMaxRounds : sum;
  }
  SE3DS_HD void scan_offsets(int lane, uint32_t w0) {
    if ((uint32_t)lane >= active(w0)) return;
    const uint32_t* g = sh.group[lane / kScanGroup];
    sh.blocks[lane] += g[0];
    sh.dc[0][lane] += g[1];
    sh.dc[1][lane] += g[2];
    sh.dc[2][lane] += g[3];
  }

  SE3DS_HD bool write(int lane, uint32_t w0) {
    sh.err[lane] = 0;
    if ((uint32_t)lane >= active(w0)) return false;
    const uint32_t pred[3] = {sh.dc[0][lane], sh.dc[1][lane], sh.dc[2][lane]};
    const Result r = decode_chunk<true>(sh.used[lane], chunk_lim(lane, w0), w0, sh.blocks[lane], pred);
    sh.err[lane] = r.err;
    return r.err != 0;
  }

  SE3DS_HD void first_error(int lane) {
    if (lane != 0) return;
    for (int i = 0; i < LANES; ++i)
      if (sh.err[i]) {
        sh.status = sh.err[i];
        return;
      }
  }

  // The whole segment -> its status word.  Control flow outside the phases depends only on values
  // every lane reads behind a synchronisation, so it is uniform over the workgroup.
  template <class Policy>
  SE3DS_HD int32_t run(const Policy& policy) {
    policy.each([&](int lane) { tables_serial(lane); });
    policy.each([&](int lane) { tables_look(lane); });
    const uint32_t windows = (len + Sh::kWindow - 1) / Sh::kWindow;
    bool failed = false;
    for (uint32_t w = 0; w < windows && !failed && sh.carry_blocks < total; ++w) {
      const uint32_t w0 = w * Sh::kWindow;
      policy.each([&](int lane) { stage(lane, w0); });
      policy.each([&](int lane) { round0(lane, w0); });
      const uint32_t n = active(w0);
      uint32_t r = 1;
      bool changed = true;
      for (; r <= n && changed; ++r)
        changed = policy.any([&](int lane) { return round_n(lane, w0, r); });
      // r - 1 rounds >= 1 ran; the last of them wrote buffer (r - 1) & 1
      policy.each([&](int lane) { scan_groups(lane, w0); });
      policy.each([&](int lane) { scan_totals(lane, w0, (int)((r - 1) & 1u), r); });
      policy.each([&](int lane) { scan_offsets(lane, w0); });
      failed = policy.any([&](int lane) { return write(lane, w0); });
      if (failed) policy.each([&](int lane) { first_error(lane); });
    }
    uint32_t code = sh.status;
    if (!failed && sh.carry_blocks < total) code = (uint32_t)Status::TRUNCATED;
    return (int32_t)(code | (sh.rounds << 8));
  }
};

// ---- inverse transform: T.81 A.3.3 by the factorisation of Loeffler, Ligtenberg and Moschytz in
// 13-bit fixed point ("slow integer"): the constants are round(c * 8192).
SE3DS_HD void idct_1d(const uint32_t* in, uint32_t* out, int shift) {
  const uint32_t z1a = (in[2] + in[6]) * 4433u;
  const uint32_t e2 = z1a - in[6] * 15137u, e3 = z1a + in[2] * 6270u;
  const uint32_t e0 = (in[0] + in[4]) * 8192u, e1 = (in[0] - in[4]) * 8192u;
  const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  uint32_t o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
  uint32_t z1 = o0 + o3, z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  o0 *= 2446u;
  o1 *= 16819u;
  o2 *= 25172u;
  o3 *= 12299u;
  z1 = 0u - z1 * 7373u;
  z2 = 0u - z2 * 20995u;
  z3 = z5 - z3 * 16069u;
  z4 = z5 - z4 * 3196u;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  const uint32_t v[8] = {t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3};
  const uint32_t half = 1u << (shift - 1);
  for (int i = 0; i < 8; ++i) {
    // arithmetic shift of the two's-complement value, without a signed operand
    const uint32_t x = v[i] + half;
    out[i] = (x >> shift) | ((x & 0x80000000u) ? ~(0xFFFFFFFFu >> shift) : 0u);
  }
}

// coef: int16 [64] natural order; quant: its table; out: 8 rows of 8 samples, `pitch` apart.
SE3DS_HD void idct_block(const int16_t* coef, const uint16_t* quant, uint8_t* out, int64_t pitch) {
  uint32_t ws[64];
  for (int c = 0; c < 8; ++c) {
    uint32_t in[8], col[8];
    for (int r = 0; r < 8; ++r)
      in[r] = (uint32_t)(int32_t)coef[r * 8 + c] * (uint32_t)quant[r * 8 + c];
    idct_1d(in, col, 11);
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = col[r];
  }
  for (int r = 0; r < 8; ++r) {
    uint32_t row[8];
    idct_1d(ws + r * 8, row, 18);
    for (int c = 0; c < 8; ++c) {
      const uint32_t v = row[c] + 128u;
      out[r * pitch + c] = (v & 0x80000000u) ? 0 : v > 255u ? 255 : (uint8_t)v;
    }
  }
}

// ---- upsampling, colour, crop: output pixel (x, y) of the image whose planes start at `planes`.
SE3DS_HD uint32_t chroma_sample(const Image& im, const uint8_t* p, int64_t pw, int64_t x, int64_t y) {
  const int64_t dw = (im.width + im.h0 - 1) / im.h0, dh = (im.height + im.v0 - 1) / im.v0;
  if (im.h0 == 1) return p[y * pw + x];   // (v0 is 1 too: 4:4:4)
  const int64_t c = x >> 1;
  if (dw <= 2) return p[(im.v0 == 2 ? y >> 1 : y) * pw + c];   // replicated, not filtered
  if (im.v0 == 1) {
    const uint8_t* q = p + y * pw;
    if (x == 0 || x == 2 * dw - 1) return q[c];
    return (x & 1) ? (3u * q[c] + q[c + 1] + 2u) >> 2 : (3u * q[c] + q[c - 1] + 1u) >> 2;
  }
  const int64_t cy = y >> 1;
  int64_t fy = (y & 1) ? cy + 1 : cy - 1;
  fy = fy < 0 ? 0 : fy > dh - 1 ? dh - 1 : fy;
  const uint8_t *near = p + cy * pw, *far = p + fy * pw;
  const uint32_t here = 3u * near[c] + far[c];
  if (x & 1) {
    if (c == dw - 1) return (4u * here + 7u) >> 4;
    return (3u * here + 3u * near[c + 1] + far[c + 1] + 7u) >> 4;
  }
  if (c == 0) return (4u * here + 8u) >> 4;
  return (3u * here + 3u * near[c - 1] + far[c - 1] + 8u) >> 4;
}

SE3DS_HD uint8_t clamp_u8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : (uint8_t)v; }

SE3DS_HD void pixel(const Image& im, const uint8_t* planes, uint8_t* dst, int64_t x, int64_t y) {
  const int64_t pw0 = plane_w(im, 0);
  const int32_t lum = planes[y * pw0 + x];
  uint8_t* o = dst + (y * im.width + x) * im.out_channels;
  if (im.out_channels == 1) {
    o[0] = (uint8_t)lum;
    return;
  }
  if (im.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)lum;
    return;
  }
  const int64_t pw1 = plane_w(im, 1);
  const uint8_t* pb = planes + pw0 * plane_h(im, 0);
  const uint8_t* pr = pb + pw1 * plane_h(im, 1);
  const int32_t cb = (int32_t)chroma_sample(im, pb, pw1, x, y) - 128;
  const int32_t cr = (int32_t)chroma_sample(im, pr, pw1, x, y) - 128;
  // |products| < 2^24: no overflow; the shifts are arithmetic (floor), written as a division-free
  // offset so that no negative value is shifted
  const int32_t bias = 1 << 24;
  o[0] = clamp_u8(lum + (((91881 * cr + 32768 + bias) >> 16) - (bias >> 16)));
  o[1] = clamp_u8(lum + (((-22554 * cb - 46802 * cr + 32768 + bias) >> 16) - (bias >> 16)));
  o[2] = clamp_u8(lum + (((116130 * cb + 32768 + bias) >> 16) - (bias >> 16)));
}

}  // namespace jpeg
}  // namespace se3ds
