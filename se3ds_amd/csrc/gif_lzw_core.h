// The part of the GIF encoder that the device (csrc/gif.hip) and the host share: the strip
// geometry, the LZW step over an open-addressed hash of (prefix, byte) -> code, the LSB-first bit
// writer, and the bound on what one strip can emit.  Plain C++ that also compiles as HIP device
// code; tools/gif_host_check.cpp runs it under the sanitizers.  The format is DESIGN.md 3.18.
//
// A strip is coded by one wave.  The walk is serial, so every lane carries the same state and takes
// the same branches; what differs per lane is named by the Wave policy: which staged pixel and which
// output word a lane holds, and who writes the table.  The host policy is a wave of one lane.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3DS_HD __host__ __device__
#else
#define SE3DS_HD
#endif

namespace se3ds {
namespace gif {

constexpr int kClear = 256, kEnd = 257, kFirstFree = 258, kMaxCodes = 4096;
constexpr int kStripPixels = 16384;        // a strip is the whole rows that reach this many pixels
constexpr int kTableSlots = 8192;          // 32 KiB of LDS; at most 3838 entries live: under half full
constexpr uint32_t kEmptySlot = 0xffffffffu;   // no entry packs to this: a code exceeds its prefix

SE3DS_HD inline int64_t strip_rows(int64_t width) {
  const int64_t rows = (kStripPixels + width - 1) / width;
  return rows < 1 ? 1 : rows;
}

// The most bits a strip of `pixels` pixels emits.  Every pixel closes at most one code and a code
// is at most 12 bits: 12 * pixels, the strip's last prefix included.  A clear inside the walk is
// emitted in place of a table entry once the table holds 4096 - 258 = 3838 of them, and every
// entry costs a pixel: at most pixels / 3838 clears of 12 bits.  The framing is the frame's
// leading clear (9 bits) and the closing clear or end code (at most 12): counted as two full codes.
SE3DS_HD inline int64_t strip_bits_bound(int64_t pixels) {
  return 12 * (pixels + pixels / (kMaxCodes - kFirstFree) + 2);
}
// The strip's slot: the bound in whole 32-bit words, and one word more so that the packer may read
// the byte behind the last one it needs.
SE3DS_HD inline int64_t strip_slot_bytes(int64_t pixels) {
  return 4 * ((strip_bits_bound(pixels) + 31) / 32 + 1);
}

SE3DS_HD inline uint32_t table_hash(uint32_t key) { return (key * 0x9e3779b1u) >> 19; }   // 13 bits

// A wave of one lane: the host.
struct HostWave {
  static constexpr int kLanes = 1;
  SE3DS_HD int lane() const { return 0; }
  SE3DS_HD bool leader() const { return true; }
  SE3DS_HD uint32_t pick(uint32_t mine, int) const { return mine; }   // lane j's value, for all
  SE3DS_HD uint32_t uniform(uint32_t v) const { return v; }           // a value all lanes agree on
  SE3DS_HD void sync() const {}                                       // the lanes' table writes are seen
};

template <typename Wave>
SE3DS_HD inline void table_clear(const Wave& w, uint32_t* table) {
  for (int i = w.lane(); i < kTableSlots; i += Wave::kLanes) table[i] = kEmptySlot;
  w.sync();
}

// Codes go out LSB first into 32-bit words; lane (word index mod lanes) keeps a word until the wave
// holds one each, then all store theirs side by side.
template <typename Wave>
struct BitWriter {
  uint32_t* out;
  uint64_t acc;
  uint32_t mine, bits, words;

  SE3DS_HD void begin(uint32_t* dst) { out = dst; acc = 0; mine = 0; bits = 0; words = 0; }
  SE3DS_HD void word(const Wave& w, uint32_t v) {
    if ((int)(words % Wave::kLanes) == w.lane()) mine = v;
    ++words;
    if (words % Wave::kLanes == 0) out[words - Wave::kLanes + w.lane()] = mine;
  }
  SE3DS_HD void emit(const Wave& w, uint32_t code, uint32_t width) {
    acc |= (uint64_t)code << bits;
    bits += width;
    if (bits >= 32) {
      word(w, (uint32_t)acc);
      acc >>= 32;
      bits -= 32;
    }
  }
  // -> the strip's length in bits; the last word is zero-padded
  SE3DS_HD uint64_t finish(const Wave& w) {
    const uint64_t total = (uint64_t)words * 32 + bits;
    if (bits) word(w, (uint32_t)acc);
    const uint32_t tail = words % Wave::kLanes;
    if ((uint32_t)w.lane() < tail) out[words - tail + w.lane()] = mine;
    return total;
  }
};

// One strip: `pixels` palette indices at px -> its code stream at out (strip_slot_bytes(pixels)
// bytes), returns the length in bits.  table: kTableSlots words, in any state.  first / last: the
// strip opens / closes its frame.
template <typename Wave>
SE3DS_HD inline uint64_t lzw_strip(const Wave& w, const uint8_t* px, int64_t pixels, bool first, bool last,
                                   uint32_t* table, uint32_t* out) {
  BitWriter<Wave> bw;
  bw.begin(out);
  table_clear(w, table);
  uint32_t width = 9, next = kFirstFree, prefix = 0;
  if (first) bw.emit(w, kClear, 9);
  uint32_t ahead = w.lane() < pixels ? px[w.lane()] : 0;
  for (int64_t base = 0; base < pixels; base += Wave::kLanes) {
    const int64_t left = pixels - base;
    const int count = left < Wave::kLanes ? (int)left : Wave::kLanes;
    const uint32_t staged = ahead;   // the next 64 pixels are on their way while these are walked
    const int64_t then = base + Wave::kLanes + w.lane();
    ahead = then < pixels ? px[then] : 0;
    for (int j = 0; j < count; ++j) {
      const uint32_t c = w.pick(staged, j);
      if (base == 0 && j == 0) {
        prefix = c;
        continue;
      }
      const uint32_t key = prefix << 8 | c;
      uint32_t slot = table_hash(key), entry;
      for (;;) {
        entry = w.uniform(table[slot]);
        if (entry == kEmptySlot || (entry >> 12) == key) break;
        slot = (slot + 1) & (kTableSlots - 1);
      }
      if (entry != kEmptySlot) {
        prefix = entry & 0xfffu;
        continue;
      }
      bw.emit(w, prefix, width);
      if (next < (uint32_t)kMaxCodes) {
        if (w.leader()) table[slot] = key << 12 | next;
        if (next == (1u << width) && width < 12) ++width;
        ++next;
      } else {
        bw.emit(w, kClear, width);
        table_clear(w, table);
        width = 9;
        next = kFirstFree;
      }
      prefix = c;
    }
  }
  bw.emit(w, prefix, width);
  if (next < (uint32_t)kMaxCodes) {   // the decoder adds one more entry behind this code
    if (next == (1u << width) && width < 12) ++width;
    ++next;
  }
  bw.emit(w, last ? kEnd : kClear, width);
  return bw.finish(w);
}

}  // namespace gif
}  // namespace se3ds
