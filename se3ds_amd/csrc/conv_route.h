// Which kernel a convolution call launches (conv.hip), decided ONCE and returned as a value: the
// route id se3ds_debug_conv_route_name reports, its family, the channels per workgroup, and the rows
// of column sums its epilogue emits -- so that the launch, the two statistics-row queries and the
// weight gradients' workspace sizes are read off the same choice.  Host arithmetic only, one text for
// two builds: conv.hip and a plain C++17 program (tools/conv_route_host_check.cpp) under the host
// sanitizers.  It reads no environment variable: conv.hip reads the switches per call and passes
// their values in (ConvSwitches).
//
// Precedence of conv_route (first gate that holds):
//   thin s2 dgrad > thin Cin fwd > thin Cout dgrad > thin Cout fwd      bf16, SE3DS_NO_THIN unset
//   > halo (3x3 stride 1) > 256-pixel macro tile > 128 x 128 LDS-DMA    operands 16-byte streamable
//   > gather                                                           everything else
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>

#include "../../include/se3ds_hip.h"

namespace se3ds {

// Test hook (se3ds_debug_last_conv_route): every dispatcher of the convolution family names the
// kernel instantiation it is about to launch -- one entry per template instantiation that differs in
// tile shape, MFMA shape (m16 = 16x16x32, m32 = 32x32x16), dtype, mode or fused-BN flag.  Host only:
// a thread_local ring of the calling thread's last launches, no device work.
#define SE3DS_CONV_ROUTES(X)                                                                      \
  X(thin_s2_dgrad) X(thin_cin_fwd) X(thin_cout_dgrad) X(thin_cout_fwd)                             \
  X(halo256_fwd_m16) X(halo256_dgrad_m16) X(halo256_dgrad_bn_m16)                                  \
  X(halo256_fwd_m32) X(halo256_dgrad_m32) X(halo256_dgrad_bn_m32)                                  \
  X(halo128_fwd_m16) X(halo128_dgrad_m16) X(halo128_dgrad_bn_m16)                                  \
  X(halo128_fwd_m32) X(halo128_dgrad_m32) X(halo128_dgrad_bn_m32)                                  \
  X(big256_fwd_m16) X(big256_dgrad_m16) X(big256_dgrad_bn_m16)                                     \
  X(big256_fwd_m32) X(big256_dgrad_m32) X(big256_dgrad_bn_m32)                                     \
  X(big128_fwd_m16) X(big128_dgrad_m16) X(big128_dgrad_bn_m16)                                     \
  X(big128_fwd_m32) X(big128_dgrad_m32) X(big128_dgrad_bn_m32)                                     \
  X(glds_f32_fwd) X(glds_f32_dgrad)                                                                \
  X(glds_bf16_fwd_m16) X(glds_bf16_dgrad_m16) X(glds_bf16_dgrad_bn_m16)                            \
  X(glds_bf16_fwd_m32) X(glds_bf16_dgrad_m32) X(glds_bf16_dgrad_bn_m32)                            \
  X(igemm_f32_fwd) X(igemm_f32_dgrad) X(igemm_bf16_fwd) X(igemm_bf16_dgrad)                        \
  X(wgrad_taps3_m16) X(wgrad_taps3_m32) X(wgrad_taps_wrap) X(thin_cin_wgrad)                       \
  X(wgrad_glds_f32) X(wgrad_glds_bf16) X(wgrad_f32) X(wgrad_bf16)                                  \
  X(wgrad_reduce_vec) X(wgrad_reduce_scalar) X(wgrad_reduce_multi)                                 \
  X(thin_cout_wgrad_t2) X(thin_cout_wgrad_t3) X(thin_cout_wgrad_t4) X(thin_cout_wgrad_t5)          \
  X(pad_channels8) X(wgrad_taps_thin) X(wgrad_swap_fixup)                                          \
  X(weight_prep_f32) X(weight_prep_bf16) X(weight_prep_vec) X(weight_prep_multi)
enum ConvRoute {
#define SE3DS_ROUTE_ENUM(name) kRoute_##name,
  SE3DS_CONV_ROUTES(SE3DS_ROUTE_ENUM)
#undef SE3DS_ROUTE_ENUM
  kConvRouteCount
};
// the forward / data-gradient kernels (one parameter struct, IgemmParams) come first
constexpr int kIgemmRouteCount = kRoute_igemm_bf16_dgrad + 1;

namespace {

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

// ------------------------------------------------------------------ tile sizes the gates and grids read
constexpr int BM = 128;     // pixels per tile
constexpr int BN = 128;     // output channels per tile
constexpr int WG_BL = 32;   // weight gradient: reduction pixels per step
constexpr int kThinCols = 32;                       // pixel columns per tile of every thin kernel but the s2 one
constexpr int kThinDRows = 8, kThinDCinMax = 256;   // thin Cout data gradient
constexpr int kThinSRows = 8, kThinSCols = 64;      // thin 4x4 stride-2 data gradient
constexpr int kThinKMax = 256, kThinCinMax = 8;     // thin Cin forward / weight gradient
constexpr int kThinWRows = 8, kThinWSlabs = 256;    // thin Cin weight gradient: one partial slab per workgroup
constexpr int kThinQRows = 8, kThinQSlabs = 256;    // thin Cout weight gradient: 8 x 32 pixel tiles, one 8-wave workgroup per CU
constexpr int kThinFRows = 16;                      // thin Cin forward
constexpr int kThinRows = 4;                        // thin Cout forward

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ forward and data gradient
// The switches, as conv.hip reads them from the environment per call (tests flip them in-process).
struct ConvSwitches {
  bool thin;            // SE3DS_NO_THIN unset: the thin-layer kernels are taken where they apply
  int big_tile;         // SE3DS_BIG_TILE: -1 unset = cost model, 0 = never, 1 = whenever the shape allows
  int halo_tile;        // SE3DS_HALO_TILE: -1 unset = heuristic, 0 = never, 1 = whenever the shape allows, 128 / 256 = that width
  bool m16;             // SE3DS_HALO_M16 not 0: v_mfma_f32_16x16x32_bf16 in the LDS-DMA kernels and the tap-fused weight gradient
  int fused_bn_stats;   // SE3DS_FUSED_BN_STATS: 0 = never, 1 = only the halo-resident 3x3 kernel, 2 (default) = every LDS-DMA kernel
};

enum ConvMask { kMaskNone = 0, kMaskBinary = 1, kMaskFractional = 2 };
struct ConvCall {
  int mode, dtype;
  int n, h, w, cin, ho, wo, cout, kh, kw, stride, pad_t, pad_l, wrap_w;
  ConvMask mask;   // the input mask (forward) or the gradient's row scale (data gradient: fractional)
  bool row_a, bias, act, stats, addend, bn_x;   // the argument is present (act: not 0)
  bool pitched;    // o_pitch or bias_mod given: the 2x2 transposed convolution's interleaved rows
};

enum class ConvFamily { ThinS2Dgrad, ThinCinFwd, ThinCoutDgrad, ThinCoutFwd, Halo, Big, Glds, Gather };
struct ConvChoice {
  ConvRoute route;
  ConvFamily family;
  int channels;         // output channels per workgroup of the halo / macro-tile kernels (128 / 256), else 0
  bool glds;            // the operands stream through the LDS-DMA path (also what fills IgemmParams for the gather)
  int64_t stats_rows;   // rows of the [rows][2][channels] column sums the route's epilogue emits (one per
                        // 64-pixel wave tile); 0: it emits none (fp32, gather, thin, ragged channel tiles,
                        // a strided data gradient)
};

// Output channels per workgroup of the halo-resident 3x3 kernel (256 / 128) or 0 for the next family.
// Measured (tools/conv_bench.py): the 256-channel tile runs one workgroup per CU at ~1.25x the
// per-CU rate of two resident 128 x 128 tiles, so it wins unless its coarser grid leaves CUs
// idle in the last round; the 128-channel variant does not beat the 128 x 128 kernel and is
// only taken when forced (tests).
inline int halo_tile_channels(int n, int oh, int ow, int oc, int forced) {
  if (forced == 0) return 0;
  if ((oc % 128) != 0) return 0;
  if (forced == 128 || (oc % 256) != 0) return 128;
  if (forced == 256) return 256;
  // 256 channels per workgroup unless that leaves a large part of the chip without work
  const int64_t tiles = (int64_t)n * cdiv(oh, 8) * cdiv(ow, 32);
  const int64_t items256 = tiles * (oc / 256);
  const double eff256 = (double)items256 / (double)(cdiv(items256, (int64_t)256) * 256);
  const int64_t items128 = items256 * 2;
  const double eff128 = 0.85 * (double)items128 / (double)(cdiv(items128, (int64_t)256) * 256);
  return eff256 >= eff128 ? 256 : 128;
}

// Output channels per 256-pixel macro tile (256 / 128) or 0 for the 128 x 128 kernel; stride: of the
// data gradient's parity classes (1 for the forward pass).
inline int big_tile_channels(int n, int oh, int ow, int oc, int stride, int g_big_tile) {
  if (g_big_tile == 0) return 0;
  const int co = (oc % 256) == 0 ? 256 : ((oc % 128) == 0 ? 128 : 0);
  if (!co) return 0;
  if (g_big_tile == 1) return co;
  int64_t m = 0;   // pixel rows over all parity classes
  const int s = stride;
  for (int py = 0; py < s; ++py)
    for (int px = 0; px < s; ++px)
      m += (int64_t)n * ((oh - py + s - 1) / s) * ((ow - px + s - 1) / s);
  const double kCusD = 256.0;
  const double big_items = (double)cdiv(m, (int64_t)256) * (oc / co);
  const double small_items = (double)cdiv(m, (int64_t)128) * cdiv(oc, 128);
  if (co != 256) return 0;
  const double gain = 1.25;
  // time in units of one 128 x 128 tile on a CU that holds two of them
  const double t_small = std::ceil(small_items / (2 * kCusD)) * 2.0;
  const double t_big = std::ceil(big_items / kCusD) * (co == 256 ? 4.0 : 2.0) / gain;
  return t_big < t_small ? co : 0;
}

// The six variants of an LDS-DMA family follow each other in SE3DS_CONV_ROUTES: forward, data
// gradient, data gradient with fused batch-norm statistics, at m16 and then at m32.
inline ConvRoute lds_dma_variant(ConvRoute fwd_m16, bool fwd, bool bn, bool m16) {
  return (ConvRoute)(fwd_m16 + (m16 ? 0 : 3) + (fwd ? 0 : (bn ? 2 : 1)));
}
static_assert(kRoute_halo256_dgrad_m16 == kRoute_halo256_fwd_m16 + 1 && kRoute_halo256_dgrad_bn_m32 == kRoute_halo256_fwd_m16 + 5 &&
              kRoute_halo128_dgrad_m16 == kRoute_halo128_fwd_m16 + 1 && kRoute_halo128_dgrad_bn_m32 == kRoute_halo128_fwd_m16 + 5 &&
              kRoute_big256_dgrad_m16 == kRoute_big256_fwd_m16 + 1 && kRoute_big256_dgrad_bn_m32 == kRoute_big256_fwd_m16 + 5 &&
              kRoute_big128_dgrad_m16 == kRoute_big128_fwd_m16 + 1 && kRoute_big128_dgrad_bn_m32 == kRoute_big128_fwd_m16 + 5 &&
              kRoute_glds_bf16_dgrad_m16 == kRoute_glds_bf16_fwd_m16 + 1 && kRoute_glds_bf16_dgrad_bn_m32 == kRoute_glds_bf16_fwd_m16 + 5 &&
              kRoute_halo256_fwd_m32 == kRoute_halo256_fwd_m16 + 3 && kRoute_glds_bf16_fwd_m32 == kRoute_glds_bf16_fwd_m16 + 3,
              "lds_dma_variant counts on the order of SE3DS_CONV_ROUTES");

// Every gate, once, in the order the kernels take precedence.  `c` is a call that passed
// conv_common's shape validation (stride 1 or 2, a known dtype).
inline ConvChoice conv_route(const ConvCall& c, const ConvSwitches& sw) {
  const bool fwd = c.mode == MODE_FWD, bf16 = c.dtype == SE3DS_BF16;
  const bool k3s1 = c.kh == 3 && c.kw == 3 && c.stride == 1;
  const int bk = bf16 ? 32 : 16;                       // elements per K step
  const int sc = fwd ? c.cin : c.cout;                 // channels of the streamed operand ...
  const int oc = fwd ? c.cout : c.cin;                 // ... and of the result,
  const int oh = fwd ? c.ho : c.h, ow = fwd ? c.wo : c.w;   // whose pixels the tiles cover
  ConvChoice ch = {kRoute_igemm_f32_fwd, ConvFamily::Gather, 0, false, 0};
  ch.glds = (sc % (2 * bk)) == 0 && c.mask != kMaskFractional;
  if (!fwd && bf16 && c.kh == 4 && c.kw == 4 && c.stride == 2 && c.cin <= 4 && c.cout == 128 &&
      c.mask == kMaskNone && !c.row_a && !c.bias && !c.act && !c.wrap_w &&
      (c.pad_t == 0 || c.pad_t == 2) && (c.pad_l == 0 || c.pad_l == 2) && sw.thin) {
    ch.route = kRoute_thin_s2_dgrad; ch.family = ConvFamily::ThinS2Dgrad;
    return ch;
  }
  if (fwd && bf16 && c.cin <= kThinCinMax && (c.cout % 128) == 0 && c.kh * c.kw * c.cin <= kThinKMax &&
      c.kh <= 7 && c.kw <= 7 && !c.stats && !c.addend && !c.pitched && sw.thin) {
    ch.route = kRoute_thin_cin_fwd; ch.family = ConvFamily::ThinCinFwd;
    return ch;
  }
  if (!fwd && bf16 && k3s1 && c.cout <= 4 && (c.cin % 64) == 0 && c.cin <= kThinDCinMax &&
      c.mask == kMaskNone && !c.row_a && sw.thin) {
    ch.route = kRoute_thin_cout_dgrad; ch.family = ConvFamily::ThinCoutDgrad;
    return ch;
  }
  if (fwd && bf16 && k3s1 && c.cout <= 4 && (c.cin % 64) == 0 && c.cin <= 128 && c.mask == kMaskNone &&
      !c.row_a && !c.stats && !c.addend && sw.thin) {
    ch.route = kRoute_thin_cout_fwd; ch.family = ConvFamily::ThinCoutFwd;
    return ch;
  }
  // the fused batch-norm backward statistics ride on a data gradient that was given stats and bn_x
  const bool bn = !fwd && c.stats && c.bn_x;
  // rows: stride 1 only for the data gradient -- one parity class, the same tile geometry as a
  // forward pass over the gradient's pixels
  const bool rows = fwd || c.stride == 1;
  const int64_t m = (int64_t)c.n * oh * ow;
  if (ch.glds && bf16 && k3s1) {
    ch.channels = halo_tile_channels(c.n, oh, ow, oc, sw.halo_tile);
    if (ch.channels) {
      ch.family = ConvFamily::Halo;
      ch.route = lds_dma_variant(ch.channels == 256 ? kRoute_halo256_fwd_m16 : kRoute_halo128_fwd_m16, fwd, bn, sw.m16);
      ch.stats_rows = (int64_t)c.n * cdiv(oh, 8) * cdiv(ow, 32) * 4;
      return ch;
    }
  }
  if (ch.glds && bf16) {
    ch.channels = big_tile_channels(c.n, oh, ow, oc, fwd ? 1 : c.stride, sw.big_tile);
    if (ch.channels) {
      ch.family = ConvFamily::Big;
      ch.route = lds_dma_variant(ch.channels == 256 ? kRoute_big256_fwd_m16 : kRoute_big128_fwd_m16, fwd, bn, sw.m16);
      ch.stats_rows = rows ? cdiv(m, (int64_t)256) * 4 : 0;
      return ch;
    }
  }
  if (ch.glds) {
    ch.family = ConvFamily::Glds;
    if (!bf16) {
      ch.route = fwd ? kRoute_glds_f32_fwd : kRoute_glds_f32_dgrad;
      return ch;
    }
    // (the 16x16x32 epilogue has no ragged channel tiles, and neither have the column sums)
    const bool whole = (oc % BN) == 0;
    ch.route = lds_dma_variant(kRoute_glds_bf16_fwd_m16, fwd, bn, whole && sw.m16);
    ch.stats_rows = whole && rows ? cdiv(m, (int64_t)BM) * (BM / 64) : 0;
    return ch;
  }
  ch.route = bf16 ? (fwd ? kRoute_igemm_bf16_fwd : kRoute_igemm_bf16_dgrad)
                  : (fwd ? kRoute_igemm_f32_fwd : kRoute_igemm_f32_dgrad);
  return ch;
}

// se3ds_conv2d_fwd_stats_rows and se3ds_conv2d_dgrad_bnstats_rows: the stats_rows of the statistics
// call they describe (the gates read neither the other side's size nor the padding).  What is not
// routing stays here: the SE3DS_FUSED_BN_STATS level -- the caller's wish to use fewer of the fused
// epilogues than there are -- and the backward statistics' 16-byte channel groups.
inline int64_t conv_fwd_stats_rows(int dtype, int n, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                                   bool has_mask, bool mask_binary, const ConvSwitches& sw) {
  if (stride < 1 || stride > 2 || sw.fused_bn_stats == 0) return 0;
  ConvCall c = {};
  c.mode = MODE_FWD; c.dtype = dtype; c.n = n; c.h = ho; c.w = wo; c.cin = cin; c.ho = ho; c.wo = wo;
  c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride;
  c.mask = !has_mask ? kMaskNone : (mask_binary ? kMaskBinary : kMaskFractional);
  c.stats = true;
  const ConvChoice ch = conv_route(c, sw);
  return sw.fused_bn_stats == 1 && ch.family != ConvFamily::Halo ? 0 : ch.stats_rows;
}
inline int64_t conv_dgrad_bnstats_rows(int dtype, int n, int h, int w, int cin, int cout, int kh, int kw, int stride,
                                       bool has_row_scale, const ConvSwitches& sw) {
  if (stride < 1 || stride > 2 || (cin % 8) != 0) return 0;
  ConvCall c = {};
  c.mode = MODE_DGRAD; c.dtype = dtype; c.n = n; c.h = h; c.w = w; c.cin = cin; c.ho = h; c.wo = w;
  c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride;
  c.mask = has_row_scale ? kMaskFractional : kMaskNone;
  c.stats = c.bn_x = true;
  return conv_route(c, sw).stats_rows;
}

// ------------------------------------------------------------------ weight gradient
struct WgradChoice {
  ConvRoute route;
  int splits;             // partial slabs the kernel writes and the split reduce sums
  int slabs;              // partial slabs the workspace holds for this route (>= splits)
  int steps;              // tap-fused kernels: 64-pixel steps in all ...
  int steps_per_split;    // ... and per split
  int64_t row_tiles;      // generic kernels: grid.x
  int linear_k;           // ... K = (tap, ci) linearised (Cin <= 16)
  int64_t l_per_split;    // ... reduction pixels per split
  size_t lead_bytes;      // swapped form: bytes in front of the partial slabs (the padded dy copy of
                          // the taps-thin route, the transposed result of the generic one)
};
constexpr WgradChoice kNoWgrad = {kConvRouteCount, 0, 0, 0, 0, 0, 0, 0, 0};
// fp32 partial slabs of `nel` weights each, and the tail every weight-gradient workspace has
inline size_t wgrad_slab_bytes(int slabs, int64_t nel) { return sizeof(float) * (size_t)slabs * (size_t)nel + 16; }

inline int wgrad_splits(int64_t L, int64_t tiles, int64_t nel) {
  // Work items = tiles x splits, equal cost; ~512 run concurrently (2 per CU).  Cost model
  // (microseconds): rounds of items x steps per item x time per 64-pixel step, plus the write +
  // read of the fp32 partial slabs by the deterministic reduce.  Pick the cheapest split count.
  const double kStepUs = 2.15, kBytesPerUs = 3.0e6, kSlots = 512.0;
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= 256; ++s) {
    int64_t per = (L + s - 1) / s;
    if (s > 1 && per < 256) break;
    double steps = (double)((per + 63) / 64);
    double rounds = (double)((tiles * s + (int64_t)kSlots - 1) / (int64_t)kSlots);
    double cost = rounds * steps * kStepUs + (s > 1 ? 5.0 : 0.0) +
                  (double)s * (double)nel * 8.0 / kBytesPerUs * (s > 1 ? 1.0 : 0.5);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}

// CUs a weight-gradient launch may count on.  (With the two decoders on two streams a 128-item
// launch of one branch shares the chip with the other branch's; counting on 128 was measured
// 221.1 / 221.4 ms per step against 222.7 / 221.5 with 256 on one box in round 3 -- the launches of
// the two branches do not pair up reliably: all 256.)
constexpr int wgrad_slots() { return 256; }

// tap-fused 3x3 kernel: steps of 64 pixels, work items = (Cin/64) x (Cout/128) x splits on 256
// single-workgroup CUs.  Returns the split count (0: shape not eligible).
inline int wgrad_taps_splits(int n, int ho, int wo, int cin, int cout, int kh, int kw, int* steps) {
  if (kh != 3 || kw != 3 || (cin % 64) != 0 || (cout % 128) != 0) return 0;
  const int64_t total = (int64_t)n * cdiv(ho, 2) * cdiv(wo, 32);
  if (total > (1 << 30)) return 0;
  *steps = (int)total;
  const int64_t tiles = (int64_t)(cin / 64) * (cout / 128);
  // rounds of 256 items x steps per item (~1.3 us each) + partial-slab traffic of the reduce
  const double kStepUs = 1.3, kBytesPerUs = 3.0e6;
  const int64_t nel = (int64_t)9 * cin * cout;
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= 512 && s <= total; ++s) {
    const double per = (double)cdiv(total, (int64_t)s);
    if (s > 1 && per < 8) break;
    const double rounds = (double)cdiv(tiles * s, (int64_t)wgrad_slots());
    const double cost = rounds * (per * kStepUs + 4.0) +
                        (double)s * (double)nel * 8.0 / kBytesPerUs * (s > 1 ? 1.0 : 0.5);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}

// thin-Cout layers through the tap-fused kernel (padded dy copy): split count, 0 = not eligible
inline int wgrad_taps_thin_splits(int n, int h, int w, int cin, int cout, int k, int* steps) {
  if (k != 3 || cout > 8 || (cin % 64) != 0) return 0;
  const int64_t total = (int64_t)n * cdiv(h, 2) * cdiv(w, 32);
  if (total > (1 << 30)) return 0;
  *steps = (int)total;
  const int64_t tiles = cin / 64;
  int64_t sp = cdiv((int64_t)256, tiles);   // one round of the 256 CUs
  if (sp > total / 8) sp = total / 8;
  if (sp < 1) sp = 1;
  return (int)sp;
}

// The three candidates of se3ds_conv2d_wgrad by SHAPE alone (route = kConvRouteCount: not eligible);
// wgrad_route adds what a size query does not know -- dtype, stride, mask, row scale -- and
// wgrad_workspace_bytes takes the largest, so size and launch are made of the same pieces.
inline WgradChoice wgrad_taps(int n, int ho, int wo, int cin, int cout, int kh, int kw) {
  WgradChoice c = kNoWgrad;
  c.splits = c.slabs = wgrad_taps_splits(n, ho, wo, cin, cout, kh, kw, &c.steps);
  if (!c.splits) return c;
  c.route = kRoute_wgrad_taps3_m16;
  c.steps_per_split = (int)cdiv(c.steps, c.splits);
  return c;
}
inline WgradChoice wgrad_thin_cin(int n, int ho, int wo, int cin, int cout, int kh, int kw, const ConvSwitches& sw) {
  WgradChoice c = kNoWgrad;
  if (!(cin <= kThinCinMax && cout == 128 && kh * kw * cin <= kThinKMax && kh <= 7 && kw <= 7 && sw.thin)) return c;
  c.route = kRoute_thin_cin_wgrad;
  const int64_t blocks = (int64_t)n * cdiv(ho, kThinWRows) * cdiv(wo, kThinCols);
  c.splits = (int)(blocks > kThinWSlabs ? kThinWSlabs : blocks);   // one partial slab per persistent workgroup
  c.slabs = kThinWSlabs;
  return c;
}
inline WgradChoice wgrad_generic(int n, int ho, int wo, int cin, int cout, int kh, int kw) {
  WgradChoice c = kNoWgrad;
  c.route = kRoute_wgrad_bf16;
  c.linear_k = cin <= 16 ? 1 : 0;
  const int64_t L = (int64_t)n * ho * wo;
  c.row_tiles = c.linear_k ? cdiv((int64_t)kh * kw * cin, 128) : (int64_t)kh * kw * cdiv(cin, 128);
  c.splits = c.slabs = wgrad_splits(L, c.row_tiles * cdiv(cout, 128), (int64_t)kh * kw * cin * cout);
  c.l_per_split = cdiv(cdiv(L, c.splits), WG_BL) * WG_BL;
  return c;
}

inline WgradChoice wgrad_route(int dtype, int n, int ho, int wo, int cin, int cout, int kh, int kw, int stride,
                               int wrap_w, ConvMask mask, bool row_scale, const ConvSwitches& sw) {
  const bool bf16 = dtype == SE3DS_BF16;
  if (bf16 && stride == 1 && !row_scale && mask != kMaskFractional) {
    WgradChoice c = wgrad_taps(n, ho, wo, cin, cout, kh, kw);
    if (c.splits > 0) {
      c.route = wrap_w ? kRoute_wgrad_taps_wrap : (sw.m16 ? kRoute_wgrad_taps3_m16 : kRoute_wgrad_taps3_m32);
      return c;
    }
  }
  if (bf16 && stride <= 2) {
    const WgradChoice c = wgrad_thin_cin(n, ho, wo, cin, cout, kh, kw, sw);
    if (c.route == kRoute_thin_cin_wgrad) return c;
  }
  WgradChoice c = wgrad_generic(n, ho, wo, cin, cout, kh, kw);
  const int epc = bf16 ? 8 : 4;   // elements per 16-byte chunk
  const bool glds = !c.linear_k && mask != kMaskFractional && !row_scale && (cin % epc) == 0 && (cout % epc) == 0;
  if (glds) c.l_per_split = cdiv(cdiv((int64_t)n * ho * wo, c.splits), 64) * 64;
  c.route = glds ? (bf16 ? kRoute_wgrad_glds_bf16 : kRoute_wgrad_glds_f32) : (bf16 ? kRoute_wgrad_bf16 : kRoute_wgrad_f32);
  return c;
}
inline size_t wgrad_workspace_bytes(int n, int ho, int wo, int cin, int cout, int kh, int kw, const ConvSwitches& sw) {
  const int64_t nel = (int64_t)kh * kw * cin * cout;
  size_t bytes = 0;
  for (const WgradChoice& c : {wgrad_taps(n, ho, wo, cin, cout, kh, kw), wgrad_thin_cin(n, ho, wo, cin, cout, kh, kw, sw),
                               wgrad_generic(n, ho, wo, cin, cout, kh, kw)}) {
    const size_t b = wgrad_slab_bytes(c.slabs, nel);
    bytes = b > bytes ? b : bytes;
  }
  return bytes;
}

// se3ds_conv2d_wgrad_swapped (k x k, stride 1, few output channels).  The generic route is
// se3ds_conv2d_wgrad of the swapped problem into lead_bytes of the workspace, then the fix-up.
inline WgradChoice wgrad_swapped_thin_cout(int n, int h, int w, int cin, int cout, int k) {
  WgradChoice c = kNoWgrad;
  if (!(k == 3 && cout <= 4)) return c;
  // column tiles per wave: 9 * Cin / 32 tiles dealt to 8 waves
  const int64_t tiles_per_wave = cdiv(9 * (cin / 32), 8);
  c.route = tiles_per_wave == 2 ? kRoute_thin_cout_wgrad_t2 : tiles_per_wave == 3 ? kRoute_thin_cout_wgrad_t3
          : tiles_per_wave == 4 ? kRoute_thin_cout_wgrad_t4 : kRoute_thin_cout_wgrad_t5;
  const int64_t blocks = (int64_t)n * cdiv(h, kThinQRows) * cdiv(w, kThinCols);
  c.splits = (int)(blocks > kThinQSlabs ? kThinQSlabs : blocks);   // one partial slab per persistent workgroup
  c.slabs = kThinQSlabs;
  return c;
}
inline WgradChoice wgrad_swapped_taps_thin(int n, int h, int w, int cin, int cout, int k) {
  WgradChoice c = kNoWgrad;
  c.splits = c.slabs = wgrad_taps_thin_splits(n, h, w, cin, cout, k, &c.steps);
  if (!c.splits) return c;
  c.route = kRoute_wgrad_taps_thin;
  c.steps_per_split = (int)cdiv(c.steps, c.splits);
  c.lead_bytes = ((size_t)n * h * w * 16 + 255) / 256 * 256;   // dy padded to 8 channels
  return c;
}
inline WgradChoice wgrad_swapped_route(int dtype, int n, int h, int w, int cin, int cout, int k, const ConvSwitches& sw) {
  const bool bf16 = dtype == SE3DS_BF16;
  if (bf16 && (cin % 32) == 0 && cin <= 128 && sw.thin) {
    const WgradChoice c = wgrad_swapped_thin_cout(n, h, w, cin, cout, k);
    if (c.slabs) return c;
  }
  if (bf16) {
    const WgradChoice c = wgrad_swapped_taps_thin(n, h, w, cin, cout, k);
    if (c.splits > 0) return c;
  }
  WgradChoice c = kNoWgrad;
  c.route = kRoute_wgrad_swap_fixup;
  c.lead_bytes = (sizeof(float) * (size_t)k * k * cin * cout + 63) / 64 * 64;
  return c;
}
inline size_t wgrad_swapped_workspace_bytes(int n, int h, int w, int cin, int cout, int k, const ConvSwitches& sw) {
  const int64_t nel = (int64_t)k * k * cin * cout;
  const size_t a = wgrad_workspace_bytes(n, h, w, cout, cin, k, k, sw) + sizeof(float) * (size_t)nel + 64;
  const int sp = wgrad_swapped_taps_thin(n, h, w, cin, cout, k).slabs;
  const size_t b = sp ? (size_t)n * h * w * 16 + 256 + sizeof(float) * (size_t)sp * (size_t)nel + 64 : 0;
  const int q = wgrad_swapped_thin_cout(n, h, w, cin, cout, k).slabs;
  const size_t c = q ? sizeof(float) * (size_t)q * (size_t)nel + 64 : 0;
  const size_t ab = a > b ? a : b;
  return ab > c ? ab : c;
}

}  // namespace
}  // namespace se3ds
