// The routing of the convolution family (se3ds_amd/csrc/conv_route.h) as a plain host program, for the
// sanitizers: which kernel a forward / data-gradient / weight-gradient call launches, the rows of
// fused statistics it emits, the split counts and the workspace sizes.  Built and run by
// tests/test_conv_route_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -Werror
//       tools/conv_route_host_check.cpp -o conv_route_host_check && ./conv_route_host_check
//
// The yardstick (old_* below) is a literal transcription of the dispatchers conv.hip held before the
// header: conv_common's if-chain, fwd_stats_rows, the pre-filters of the two *_rows queries, the chains
// of se3ds_conv2d_wgrad and se3ds_conv2d_wgrad_swapped and the sums of their size queries, with the
// environment reads replaced by the values of OldSw.
//
// Sweep: mode fwd / dgrad x dtype fp32 / bf16 x k in {1, 2, 3, 4, 7} x stride in {1, 2} x
// cin in {3, 4, 8, 16, 32, 64, 96, 128, 192, 256, 512, 1024, 2048} x cout in {1, 3, 4, 8, 64, 128, 192,
// 256, 512, 1024, 2048} x (h, w) in {(8, 16), (32, 64), (33, 65), (129, 257), (512, 1024)} x
// n in {1, 8, 16} x mask none / binary / fractional; padding (k - 1) / 2, and 0 / 1 / 2 for the 4x4
// stride-2 layers (the thin stride-2 data gradient asks for 0 or 2).  Pruned: on every such shape the
// argument flags (row_a, bias, act, stats [+ bn_x], addend, pitched, wrap_w) go on ONE at a time under
// the default switches, and every switch takes each documented value ONE at a time with the
// statistics off and on -- a gate reads its flags and switches independently of each other, so pairs
// add nothing but the three rows at the end of kSwitchRows, without which no call reaches the forced
// 128-channel macro tile at m32.  The weight gradients: every shape x stride x mask x row scale x wrap x the two
// switches they read; the swapped form and the four size queries on every shape.
// Further: every route a dispatcher can choose occurs in the sweep (kLaunchedUnconditionally lists the
// others); stats_rows > 0 only on a bf16 LDS-DMA route; the production shapes of
// profiles/r06_shapes_b8.txt keep their routes and split counts (kPinned).
// `conv_route_host_check corrupt` gives the yardstick the macro tile BEFORE the halo kernel: exit 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../se3ds_amd/csrc/conv_route.h"

using namespace se3ds;

static long long g_cases = 0;
static bool g_corrupt = false;
static bool g_seen[kConvRouteCount];
static const char* const kNames[] = {
#define SE3DS_ROUTE_NAME(name) #name,
    SE3DS_CONV_ROUTES(SE3DS_ROUTE_NAME)
#undef SE3DS_ROUTE_NAME
    "none"};
// launched by every call of their entry point (or next to a chosen route), never chosen
static const ConvRoute kLaunchedUnconditionally[] = {
    kRoute_wgrad_reduce_vec, kRoute_wgrad_reduce_scalar, kRoute_wgrad_reduce_multi, kRoute_pad_channels8,
    kRoute_weight_prep_f32,  kRoute_weight_prep_bf16,    kRoute_weight_prep_vec,    kRoute_weight_prep_multi};

// ---------------------------------------------------------------- the yardstick (conv.hip before conv_route.h)
struct OldSw {
  bool no_thin;                 // SE3DS_NO_THIN is set
  int big, halo, m16, fused;    // atoi of SE3DS_BIG_TILE / _HALO_TILE (-1: unset), _HALO_M16 (unset: 1), _FUSED_BN_STATS (unset: 2)
};
struct OldParams { int N, oH, oW, oC, sC, stride; bool bn_x; };   // what the gates read of IgemmParams
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int kOldBM = 128, kOldBN = 128, kOldWgBl = 32;

static bool old_thin_on(const OldSw& e) { return !e.no_thin; }
static int old_halo_tile_channels(const OldParams& p, const OldSw& e) {
  const int mode = e.halo;
  if (mode == 0) return 0;
  if ((p.oC % 128) != 0) return 0;
  if (mode == 128 || (p.oC % 256) != 0) return 128;
  if (mode == 256) return 256;
  const int64_t tiles = (int64_t)p.N * ceil_div(p.oH, 8) * ceil_div(p.oW, 32);
  const int64_t items256 = tiles * (p.oC / 256);
  const double eff256 = (double)items256 / (double)(ceil_div(items256, (int64_t)256) * 256);
  const int64_t items128 = items256 * 2;
  const double eff128 = 0.85 * (double)items128 / (double)(ceil_div(items128, (int64_t)256) * 256);
  return eff256 >= eff128 ? 256 : 128;
}
static bool old_halo_m16(const OldSw& e) { return e.m16 != 0; }
static int old_big_tile_channels(const OldParams& p, int mode, const OldSw& e) {
  const int g_big_tile = e.big;
  if (g_big_tile == 0) return 0;
  const int co = (p.oC % 256) == 0 ? 256 : ((p.oC % 128) == 0 ? 128 : 0);
  if (!co) return 0;
  if (g_big_tile == 1) return co;
  int64_t m = 0;
  const int s = mode == MODE_FWD ? 1 : p.stride;
  for (int py = 0; py < s; ++py)
    for (int px = 0; px < s; ++px)
      m += (int64_t)p.N * ((p.oH - py + s - 1) / s) * ((p.oW - px + s - 1) / s);
  const double kCus = 256.0;
  const double big_items = (double)ceil_div(m, (int64_t)256) * (p.oC / co);
  const double small_items = (double)ceil_div(m, (int64_t)128) * ceil_div(p.oC, 128);
  if (co != 256) return 0;
  const double gain = 1.25;
  const double t_small = std::ceil(small_items / (2 * kCus)) * 2.0;
  const double t_big = std::ceil(big_items / kCus) * (co == 256 ? 4.0 : 2.0) / gain;
  return t_big < t_small ? co : 0;
}
static int64_t old_fwd_stats_rows(const OldParams& p, int dtype, int stride, int kh, int kw, bool glds, const OldSw& e,
                                  int mode = MODE_FWD) {
  if (!glds || dtype != SE3DS_BF16) return 0;
  if (mode == MODE_DGRAD && stride != 1) return 0;
  const int64_t M = (int64_t)p.N * p.oH * p.oW;
  if (stride == 1 && kh == 3 && kw == 3 && old_halo_tile_channels(p, e))
    return (int64_t)p.N * ceil_div(p.oH, 8) * ceil_div(p.oW, 32) * 4;
  if (old_big_tile_channels(p, mode, e)) return ceil_div(M, (int64_t)256) * 4;
  if ((p.oC % kOldBN) == 0) return ceil_div(M, (int64_t)kOldBM) * (kOldBM / 64);
  return 0;
}

struct OldConv {
  int status;           // SE3DS_OK: launched `route`
  int route, family, channels;
  bool glds;
  int64_t rows;         // fwd_stats_rows of the call, whether or not it passes stats
};
// conv_common from the first line after the shape validation; pointers as "is present"
static OldConv old_conv_common(int mode, int dtype, int n, int h, int wdt, int cin, int ho, int wo, int cout, int kh,
                               int kw, int stride, int pad_t, int pad_l, int wrap_w, bool src_mask, int mask_binary,
                               bool bias, bool row_a, int act, bool stats, bool addend, bool bn_x, bool bn_mean_rstd,
                               bool pitched, const OldSw& e) {
  OldConv r = {SE3DS_OK, -1, -1, 0, false, 0};
  OldParams p;
  p.N = n; p.stride = stride;
  const int bk = dtype == SE3DS_F32 ? 16 : 32;
  if (mode == MODE_FWD) { p.sC = cin; p.oH = ho; p.oW = wo; p.oC = cout; }
  else { p.sC = cout; p.oH = h; p.oW = wdt; p.oC = cin; }
  const bool glds = (p.sC % (2 * bk)) == 0 && (!src_mask || mask_binary);
  r.glds = glds;
  r.rows = old_fwd_stats_rows(p, dtype, stride, kh, kw, glds, e, mode);
  if (stats && !(r.rows > 0)) { r.status = SE3DS_E_UNSUPPORTED; return r; }
  if (stats && mode == MODE_DGRAD && (!bn_x || !bn_mean_rstd || (p.oC & 7) != 0)) { r.status = SE3DS_E_UNSUPPORTED; return r; }
  p.bn_x = mode == MODE_DGRAD && stats && bn_x;
  if (mode == MODE_DGRAD && dtype == SE3DS_BF16 && kh == 4 && kw == 4 && stride == 2 && cin <= 4 &&
      cout == 128 && !src_mask && !row_a && !bias && act == 0 &&
      !wrap_w && (pad_t == 0 || pad_t == 2) && (pad_l == 0 || pad_l == 2) &&
      old_thin_on(e)) { r.route = kRoute_thin_s2_dgrad; r.family = 0; return r; }
  if (mode == MODE_FWD && dtype == SE3DS_BF16 && cin <= 8 && (cout % 128) == 0 &&
      kh * kw * cin <= 256 && kh <= 7 && kw <= 7 && !stats && !addend &&
      !pitched && old_thin_on(e)) { r.route = kRoute_thin_cin_fwd; r.family = 1; return r; }
  if (mode == MODE_DGRAD && dtype == SE3DS_BF16 && kh == 3 && kw == 3 && stride == 1 && cout <= 4 &&
      (cin % 64) == 0 && cin <= 256 && !src_mask && !row_a &&
      old_thin_on(e)) { r.route = kRoute_thin_cout_dgrad; r.family = 2; return r; }
  if (mode == MODE_FWD && dtype == SE3DS_BF16 && kh == 3 && kw == 3 && stride == 1 && cout <= 4 &&
      (cin % 64) == 0 && cin <= 128 && !src_mask && !row_a &&
      !stats && !addend && old_thin_on(e)) { r.route = kRoute_thin_cout_fwd; r.family = 3; return r; }
  const bool halo_gate = glds && dtype == SE3DS_BF16 && stride == 1 && kh == 3 && kw == 3;
  const bool big_gate = glds && dtype == SE3DS_BF16;
  // (`corrupt`: the macro tile is asked first)
  for (int step = 0; step < 2; ++step) {
    const bool halo_turn = (step == 0) != g_corrupt;
    if (halo_turn && halo_gate) {
      const int co = old_halo_tile_channels(p, e);
      if (co) {
        r.family = 4; r.channels = co;
        if (co == 256 && old_halo_m16(e)) {
          if (mode == MODE_FWD) r.route = kRoute_halo256_fwd_m16;
          else if (p.bn_x) r.route = kRoute_halo256_dgrad_bn_m16;
          else r.route = kRoute_halo256_dgrad_m16;
        } else if (co == 256) {
          if (mode == MODE_FWD) r.route = kRoute_halo256_fwd_m32;
          else if (p.bn_x) r.route = kRoute_halo256_dgrad_bn_m32;
          else r.route = kRoute_halo256_dgrad_m32;
        } else {
          if (old_halo_m16(e)) {
            if (mode == MODE_FWD) r.route = kRoute_halo128_fwd_m16;
            else if (p.bn_x) r.route = kRoute_halo128_dgrad_bn_m16;
            else r.route = kRoute_halo128_dgrad_m16;
          } else if (mode == MODE_FWD) r.route = kRoute_halo128_fwd_m32;
          else if (p.bn_x) r.route = kRoute_halo128_dgrad_bn_m32;
          else r.route = kRoute_halo128_dgrad_m32;
        }
        return r;
      }
    }
    if (!halo_turn && big_gate) {
      const int co = old_big_tile_channels(p, mode, e);
      if (co) {
        r.family = 5; r.channels = co;
        if (co == 256 && old_halo_m16(e)) {
          if (mode == MODE_FWD) r.route = kRoute_big256_fwd_m16;
          else if (p.bn_x) r.route = kRoute_big256_dgrad_bn_m16;
          else r.route = kRoute_big256_dgrad_m16;
        } else if (co == 256) {
          if (mode == MODE_FWD) r.route = kRoute_big256_fwd_m32;
          else if (p.bn_x) r.route = kRoute_big256_dgrad_bn_m32;
          else r.route = kRoute_big256_dgrad_m32;
        } else if (old_halo_m16(e)) {
          if (mode == MODE_FWD) r.route = kRoute_big128_fwd_m16;
          else if (p.bn_x) r.route = kRoute_big128_dgrad_bn_m16;
          else r.route = kRoute_big128_dgrad_m16;
        } else {
          if (mode == MODE_FWD) r.route = kRoute_big128_fwd_m32;
          else if (p.bn_x) r.route = kRoute_big128_dgrad_bn_m32;
          else r.route = kRoute_big128_dgrad_m32;
        }
        return r;
      }
    }
  }
  if (glds) {
    r.family = 6;
    if (dtype == SE3DS_F32) {
      if (mode == MODE_FWD) r.route = kRoute_glds_f32_fwd;
      else r.route = kRoute_glds_f32_dgrad;
    } else {
      if ((p.oC % kOldBN) == 0 && old_halo_m16(e)) {
        if (mode == MODE_FWD) r.route = kRoute_glds_bf16_fwd_m16;
        else if (p.bn_x) r.route = kRoute_glds_bf16_dgrad_bn_m16;
        else r.route = kRoute_glds_bf16_dgrad_m16;
      } else if (mode == MODE_FWD) r.route = kRoute_glds_bf16_fwd_m32;
      else if (p.bn_x) r.route = kRoute_glds_bf16_dgrad_bn_m32;
      else r.route = kRoute_glds_bf16_dgrad_m32;
    }
    return r;
  }
  r.family = 7;
  if (dtype == SE3DS_F32) {
    if (mode == MODE_FWD) r.route = kRoute_igemm_f32_fwd;
    else r.route = kRoute_igemm_f32_dgrad;
  } else {
    if (mode == MODE_FWD) r.route = kRoute_igemm_bf16_fwd;
    else r.route = kRoute_igemm_bf16_dgrad;
  }
  return r;
}
static int64_t old_fwd_stats_rows_query(int dtype, int n, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                                        int has_in_mask, int in_mask_binary, const OldSw& e) {
  if (dtype != SE3DS_BF16 || stride < 1 || stride > 2 || (cin % 64) != 0 ||
      (has_in_mask && !in_mask_binary))
    return 0;
  const int lvl = e.fused;
  if (lvl == 0) return 0;
  OldParams p = {};
  p.N = n; p.oH = ho; p.oW = wo; p.oC = cout; p.stride = stride;
  if (lvl == 1 && !(stride == 1 && kh == 3 && kw == 3 && old_halo_tile_channels(p, e))) return 0;
  return old_fwd_stats_rows(p, dtype, stride, kh, kw, true, e);
}
static int64_t old_dgrad_bnstats_rows_query(int dtype, int n, int h, int w, int cin, int cout, int kh, int kw,
                                            int stride, int has_row_scale, const OldSw& e) {
  if (dtype != SE3DS_BF16 || stride != 1 || (cout % 64) != 0 || (cin % 8) != 0 || has_row_scale)
    return 0;
  OldParams p = {};
  p.N = n; p.oH = h; p.oW = w; p.oC = cin; p.stride = stride;
  return old_fwd_stats_rows(p, dtype, stride, kh, kw, true, e, MODE_DGRAD);
}

static int old_wgrad_splits(int64_t L, int64_t tiles, int64_t nel) {
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
static int old_wgrad_taps_splits(int n, int ho, int wo, int cin, int cout, int kh, int kw, int* steps) {
  if (kh != 3 || kw != 3 || (cin % 64) != 0 || (cout % 128) != 0) return 0;
  const int64_t total = (int64_t)n * ceil_div(ho, 2) * ceil_div(wo, 32);
  if (total > (1 << 30)) return 0;
  *steps = (int)total;
  const int64_t tiles = (int64_t)(cin / 64) * (cout / 128);
  const double kStepUs = 1.3, kBytesPerUs = 3.0e6;
  const int64_t nel = (int64_t)9 * cin * cout;
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= 512 && s <= total; ++s) {
    const double per = (double)ceil_div(total, (int64_t)s);
    if (s > 1 && per < 8) break;
    const double rounds = (double)ceil_div(tiles * s, (int64_t)256);
    const double cost = rounds * (per * kStepUs + 4.0) +
                        (double)s * (double)nel * 8.0 / kBytesPerUs * (s > 1 ? 1.0 : 0.5);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}
static bool old_thin_cin_wgrad_ok(int cin, int cout, int kh, int kw, const OldSw& e) {
  return cin <= 8 && cout == 128 && kh * kw * cin <= 256 && kh <= 7 && kw <= 7 &&
         old_thin_on(e);
}
static size_t old_wgrad_workspace_bytes(int n, int ho, int wo, int cin, int cout, int kh, int kw, const OldSw& e) {
  int tsteps = 0;
  const int tsplits = old_wgrad_taps_splits(n, ho, wo, cin, cout, kh, kw, &tsteps);
  const size_t taps_bytes = sizeof(float) * (size_t)tsplits * (size_t)kh * kw * cin * cout + 16;
  int64_t L = (int64_t)n * ho * wo;
  int64_t row_tiles = cin <= 16 ? ceil_div((int64_t)kh * kw * cin, 128)
                                : (int64_t)kh * kw * ceil_div(cin, 128);
  int64_t tiles = row_tiles * ceil_div(cout, 128);
  int splits = old_wgrad_splits(L, tiles, (int64_t)kh * kw * cin * cout);
  size_t bytes = sizeof(float) * (size_t)splits * (size_t)kh * kw * cin * cout + 16;
  if (old_thin_cin_wgrad_ok(cin, cout, kh, kw, e)) {
    const size_t thin = sizeof(float) * (size_t)256 * (size_t)kh * kw * cin * cout + 16;
    bytes = bytes > thin ? bytes : thin;
  }
  return bytes > taps_bytes ? bytes : taps_bytes;
}
// what a weight-gradient launch is made of: the kernel, grid.x and grid.z, the kernel's step /
// pixel counts, and the slabs the split reduce sums
struct OldWgrad {
  int route, reduce_splits, steps, steps_per_split, linear_k;
  int64_t row_tiles, l_per_split;
  size_t lead;
};
static OldWgrad old_wgrad(int dtype, int n, int ho, int wo, int cin, int cout, int kh, int kw, int stride, int wrap_w,
                          bool in_mask, int in_mask_binary, bool row_scale, const OldSw& e) {
  OldWgrad r = {-1, 0, 0, 0, 0, 0, 0, 0};
  if (dtype == SE3DS_BF16 && stride == 1 && !row_scale &&
      (!in_mask || in_mask_binary)) {
    int tsteps = 0;
    const int tsplits = old_wgrad_taps_splits(n, ho, wo, cin, cout, kh, kw, &tsteps);
    if (tsplits > 0) {
      r.steps = tsteps;
      r.steps_per_split = (int)ceil_div(tsteps, tsplits);
      if (!wrap_w) r.route = old_halo_m16(e) ? kRoute_wgrad_taps3_m16 : kRoute_wgrad_taps3_m32;
      else r.route = kRoute_wgrad_taps_wrap;
      r.reduce_splits = tsplits;
      return r;
    }
  }
  if (dtype == SE3DS_BF16 && stride <= 2 && old_thin_cin_wgrad_ok(cin, cout, kh, kw, e)) {
    int64_t blocks = (int64_t)n * ceil_div(ho, 8) * ceil_div(wo, 32);
    if (blocks > 256) blocks = 256;
    r.route = kRoute_thin_cin_wgrad;
    r.reduce_splits = (int)blocks;
    return r;
  }
  r.linear_k = cin <= 16 ? 1 : 0;
  const int64_t L = (int64_t)n * ho * wo;
  const int64_t row_tiles = r.linear_k ? ceil_div((int64_t)kh * kw * cin, 128)
                                       : (int64_t)kh * kw * (int)ceil_div(cin, 128);
  const int64_t tiles = row_tiles * ceil_div(cout, 128);
  const int splits = old_wgrad_splits(L, tiles, (int64_t)kh * kw * cin * cout);
  r.l_per_split = ceil_div(ceil_div(L, splits), kOldWgBl) * kOldWgBl;
  r.row_tiles = row_tiles;
  const int epc = dtype == SE3DS_F32 ? 4 : 8;
  const bool glds = !r.linear_k && (!in_mask || in_mask_binary) &&
                    !row_scale &&
                    (cin % epc) == 0 && (cout % epc) == 0;
  if (glds) {
    r.l_per_split = ceil_div(ceil_div(L, splits), 64) * 64;
    if (dtype == SE3DS_F32) r.route = kRoute_wgrad_glds_f32;
    else r.route = kRoute_wgrad_glds_bf16;
  } else if (dtype == SE3DS_F32) {
    r.route = kRoute_wgrad_f32;
  } else {
    r.route = kRoute_wgrad_bf16;
  }
  r.reduce_splits = splits;
  return r;
}
static int old_wgrad_taps_thin_splits(int n, int h, int w, int cin, int cout, int k, int* steps) {
  if (k != 3 || cout > 8 || (cin % 64) != 0) return 0;
  const int64_t total = (int64_t)n * ceil_div(h, 2) * ceil_div(w, 32);
  if (total > (1 << 30)) return 0;
  *steps = (int)total;
  const int64_t tiles = cin / 64;
  int64_t sp = ceil_div((int64_t)256, tiles);
  if (sp > total / 8) sp = total / 8;
  if (sp < 1) sp = 1;
  return (int)sp;
}
static size_t old_wgrad_swapped_workspace_bytes(int n, int h, int w, int cin, int cout, int k, const OldSw& e) {
  const size_t a = old_wgrad_workspace_bytes(n, h, w, cout, cin, k, k, e) +
                   sizeof(float) * (size_t)k * k * cin * cout + 64;
  int steps = 0;
  const int sp = old_wgrad_taps_thin_splits(n, h, w, cin, cout, k, &steps);
  const size_t b = sp ? (size_t)n * h * w * 16 + 256 + sizeof(float) * (size_t)sp * 9 * cin * cout + 64
                      : 0;
  const size_t c = (k == 3 && cout <= 4) ? sizeof(float) * (size_t)256 * 9 * cin * cout + 64 : 0;
  const size_t ab = a > b ? a : b;
  return ab > c ? ab : c;
}
// (the caller has passed the size check, so workspace_bytes >= the thin kernel's slabs holds)
static OldWgrad old_wgrad_swapped(int dtype, int n, int h, int w, int cin, int cout, int k, const OldSw& e) {
  OldWgrad r = {-1, 0, 0, 0, 0, 0, 0, 0};
  if (dtype == SE3DS_BF16 && k == 3 && cout <= 4 && (cin % 32) == 0 && cin <= 128 &&
      old_thin_on(e)) {
    int64_t blocks = (int64_t)n * ceil_div(h, 8) * ceil_div(w, 32);
    if (blocks > 256) blocks = 256;
    const int tiles_per_wave = (int)ceil_div(9 * (cin / 32), 8);
    switch (tiles_per_wave) {
      case 2: r.route = kRoute_thin_cout_wgrad_t2; break;
      case 3: r.route = kRoute_thin_cout_wgrad_t3; break;
      case 4: r.route = kRoute_thin_cout_wgrad_t4; break;
      default: r.route = kRoute_thin_cout_wgrad_t5; break;
    }
    r.reduce_splits = (int)blocks;
    return r;
  }
  if (dtype == SE3DS_BF16) {
    int tsteps = 0;
    const int tsplits = old_wgrad_taps_thin_splits(n, h, w, cin, cout, k, &tsteps);
    if (tsplits > 0) {
      const int64_t px = (int64_t)n * h * w;
      r.lead = ((size_t)px * 16 + 255) / 256 * 256;
      r.steps = tsteps;
      r.steps_per_split = (int)ceil_div(tsteps, tsplits);
      r.route = kRoute_wgrad_taps_thin;
      r.reduce_splits = tsplits;
      return r;
    }
  }
  r.lead = (sizeof(float) * (size_t)k * k * cin * cout + 63) / 64 * 64;
  r.route = kRoute_wgrad_swap_fixup;
  return r;
}

// ---------------------------------------------------------------- the comparison
static bool fail(const std::string& what, const char* field, long long got, long long want) {
  fprintf(stderr, "%s: %s: got %lld, expected %lld\n", what.c_str(), field, got, want);
  return false;
}
static ConvSwitches switches_of(const OldSw& e) {
  return ConvSwitches{!e.no_thin, e.big, e.halo, e.m16 != 0, e.fused};
}
static const OldSw kDefaultSw = {false, -1, -1, 1, 2};

struct Shape { int mode, dtype, n, h, w, cin, ho, wo, cout, k, stride, pad; };
struct Flags { int mask; bool row_a, bias, act, stats, addend, bn_x, pitched, wrap_w; };   // mask: 0 none, 1 binary, 2 fractional

static bool check_conv(const Shape& s, const Flags& f, const OldSw& e) {
  // (what conv_common refuses before it routes)
  if (f.wrap_w && s.mode == MODE_DGRAD && (s.stride != 1 || s.wo != s.w)) return true;
  const auto t = [&] {   // (made only for a report: the sweep has millions of cases)
    char tag[200];
    snprintf(tag, sizeof tag, "%s dtype %d n %d %dx%d->%dx%d %d->%d k %d s %d pad %d mask %d flags %d%d%d%d%d%d%d%d switches %d %d %d %d %d",
             s.mode == MODE_FWD ? "fwd" : "dgrad", s.dtype, s.n, s.h, s.w, s.ho, s.wo, s.cin, s.cout, s.k, s.stride, s.pad,
             f.mask, f.row_a, f.bias, f.act, f.stats, f.addend, f.bn_x, f.pitched, f.wrap_w, e.no_thin, e.big, e.halo,
             e.m16, e.fused);
    return std::string(tag);
  };
  const OldConv o = old_conv_common(s.mode, s.dtype, s.n, s.h, s.w, s.cin, s.ho, s.wo, s.cout, s.k, s.k, s.stride, s.pad,
                                    s.pad, f.wrap_w, f.mask != 0, f.mask == 1, f.bias, f.row_a, f.act ? 2 : 0, f.stats,
                                    f.addend, f.bn_x, f.bn_x, f.pitched, e);
  ConvCall c;
  c.mode = s.mode; c.dtype = s.dtype; c.n = s.n; c.h = s.h; c.w = s.w; c.cin = s.cin; c.ho = s.ho; c.wo = s.wo;
  c.cout = s.cout; c.kh = s.k; c.kw = s.k; c.stride = s.stride; c.pad_t = s.pad; c.pad_l = s.pad; c.wrap_w = f.wrap_w;
  c.mask = (ConvMask)f.mask; c.row_a = f.row_a; c.bias = f.bias; c.act = f.act; c.stats = f.stats; c.addend = f.addend;
  c.bn_x = f.bn_x; c.pitched = f.pitched;
  const ConvChoice ch = conv_route(c, switches_of(e));
  // conv_common after the choice: the two refusals, then the launch of ch.route
  int status = SE3DS_OK;
  if (f.stats && ch.stats_rows == 0) status = SE3DS_E_UNSUPPORTED;
  else if (f.stats && s.mode == MODE_DGRAD && (!f.bn_x || (s.cin & 7) != 0)) status = SE3DS_E_UNSUPPORTED;
  if (status != o.status) return fail(t(), "status", status, o.status);
  if (ch.stats_rows != o.rows) return fail(t(), "stats_rows", ch.stats_rows, o.rows);
  if (ch.glds != o.glds) return fail(t(), "glds", ch.glds, o.glds);
  if (ch.stats_rows > 0 && !(s.dtype == SE3DS_BF16 && ch.glds && (ch.family == ConvFamily::Halo || ch.family == ConvFamily::Big ||
                                                                   ch.family == ConvFamily::Glds)))
    return fail(t(), "stats_rows on a route without the fused epilogue", ch.stats_rows, 0);
  if (status == SE3DS_OK) {
    if ((int)ch.route != o.route) { fprintf(stderr, "%s: route %s, expected %s\n", t().c_str(), kNames[ch.route], kNames[o.route]); return false; }
    if ((int)ch.family != o.family) return fail(t(), "family", (int)ch.family, o.family);
    if (ch.channels != o.channels) return fail(t(), "channels", ch.channels, o.channels);
    if (ch.route >= kIgemmRouteCount) return fail(t(), "route outside the forward / data-gradient table", ch.route, kIgemmRouteCount);
    g_seen[ch.route] = true;
  }
  // the two queries describe this shape's statistics call
  if (f.stats && !f.bn_x && s.mode == MODE_FWD && !f.wrap_w) {
    const int64_t got = conv_fwd_stats_rows(s.dtype, s.n, s.cin, s.ho, s.wo, s.cout, s.k, s.k, s.stride, f.mask != 0,
                                            f.mask == 1, switches_of(e));
    const int64_t want = old_fwd_stats_rows_query(s.dtype, s.n, s.cin, s.ho, s.wo, s.cout, s.k, s.k, s.stride, f.mask != 0,
                                                  f.mask == 1, e);
    if (got != want) return fail(t(), "se3ds_conv2d_fwd_stats_rows", got, want);
    // ... and what it promises the call delivers (SE3DS_FUSED_BN_STATS only makes it promise less)
    if (got != 0 && (status != SE3DS_OK || got != ch.stats_rows)) return fail(t(), "rows promised, rows of the call", got, ch.stats_rows);
  }
  if (f.stats && f.bn_x && s.mode == MODE_DGRAD && !f.wrap_w) {
    const int64_t got = conv_dgrad_bnstats_rows(s.dtype, s.n, s.h, s.w, s.cin, s.cout, s.k, s.k, s.stride, f.mask != 0,
                                                switches_of(e));
    const int64_t want = old_dgrad_bnstats_rows_query(s.dtype, s.n, s.h, s.w, s.cin, s.cout, s.k, s.k, s.stride,
                                                      f.mask != 0, e);
    if (got != want) return fail(t(), "se3ds_conv2d_dgrad_bnstats_rows", got, want);
    if (got != 0 && (status != SE3DS_OK || got != ch.stats_rows)) return fail(t(), "rows promised, rows of the call", got, ch.stats_rows);
  }
  ++g_cases;
  return true;
}

// the documented values of every switch, one switch off its default at a time (first row: all default),
// then three pairs
static const OldSw kSwitchRows[] = {
    {false, -1, -1, 1, 2}, {true, -1, -1, 1, 2},  {false, 0, -1, 1, 2},  {false, 1, -1, 1, 2},  {false, -1, 0, 1, 2},
    {false, -1, 1, 1, 2},  {false, -1, 128, 1, 2}, {false, -1, 256, 1, 2}, {false, -1, -1, 0, 2}, {false, -1, -1, 1, 0},
    {false, -1, -1, 1, 1},
    // the forced 128-channel macro tile at m32, and on the 3x3 layers (halo kernel off)
    {false, 1, -1, 0, 2},  {false, 1, 0, 1, 2},   {false, 1, 0, 0, 2}};

static bool check_conv_shape(const Shape& s, int mask) {
  const Flags none = {mask, false, false, false, false, false, false, false, false};
  Flags stats = none;
  stats.stats = true;
  stats.bn_x = s.mode == MODE_DGRAD;
  for (const OldSw& e : kSwitchRows)
    if (!check_conv(s, none, e) || !check_conv(s, stats, e)) return false;
  for (int flag = 0; flag < 7; ++flag) {
    Flags f = none;
    (flag == 0 ? f.row_a : flag == 1 ? f.bias : flag == 2 ? f.act : flag == 3 ? f.addend : flag == 4 ? f.pitched
     : flag == 5 ? f.wrap_w : f.stats) = true;   // (stats without bn_x: the data gradient refuses)
    if (!check_conv(s, f, kDefaultSw)) return false;
  }
  Flags both = stats;   // the fused statistics with their usual company
  both.addend = true;
  both.row_a = true;
  return check_conv(s, both, kDefaultSw);
}

static bool check_wgrad_shape(int dtype, int n, int ho, int wo, int cin, int cout, int k) {
  for (const OldSw& e : {kDefaultSw, OldSw{true, -1, -1, 1, 2}, OldSw{false, -1, -1, 0, 2}}) {
    const ConvSwitches sw = switches_of(e);
    char tag[160];
    snprintf(tag, sizeof tag, "wgrad dtype %d n %d @%dx%d %d->%d k %d switches %d %d", dtype, n, ho, wo, cin, cout, k,
             e.no_thin, e.m16);
    const size_t bytes = wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k, sw);
    if (bytes != old_wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k, e))
      return fail(tag, "se3ds_conv2d_wgrad_workspace_bytes", (long long)bytes,
                  (long long)old_wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k, e));
    const int64_t nel = (int64_t)k * k * cin * cout;
    for (int stride = 1; stride <= 2; ++stride)
      for (int mask = 0; mask < 3; ++mask)
        for (int row_scale = 0; row_scale < 2; ++row_scale)
          for (int wrap = 0; wrap < 2; ++wrap) {
            const WgradChoice c = wgrad_route(dtype, n, ho, wo, cin, cout, k, k, stride, wrap, (ConvMask)mask, row_scale != 0, sw);
            const OldWgrad o = old_wgrad(dtype, n, ho, wo, cin, cout, k, k, stride, wrap, mask != 0, mask == 1, row_scale != 0, e);
            const auto t = [&] {
              return std::string(tag) + " stride " + std::to_string(stride) + " mask " + std::to_string(mask) +
                     " row_scale " + std::to_string(row_scale) + " wrap " + std::to_string(wrap);
            };
            if ((int)c.route != o.route) { fprintf(stderr, "%s: route %s, expected %s\n", t().c_str(), kNames[c.route], kNames[o.route]); return false; }
            if (c.splits != o.reduce_splits) return fail(t(), "splits", c.splits, o.reduce_splits);
            if (c.steps != o.steps) return fail(t(), "steps", c.steps, o.steps);
            if (c.steps_per_split != o.steps_per_split) return fail(t(), "steps_per_split", c.steps_per_split, o.steps_per_split);
            if (c.row_tiles != o.row_tiles) return fail(t(), "row_tiles", c.row_tiles, o.row_tiles);
            if (c.linear_k != o.linear_k) return fail(t(), "linear_k", c.linear_k, o.linear_k);
            if (c.l_per_split != o.l_per_split) return fail(t(), "l_per_split", c.l_per_split, o.l_per_split);
            // the launch fits the size the query reported
            if (c.slabs < c.splits || wgrad_slab_bytes(c.slabs, nel) > bytes) return fail(t(), "slabs", c.slabs, c.splits);
            g_seen[c.route] = true;
            ++g_cases;
          }
    // the swapped form (k x k, stride 1): cin and cout as the caller gives them
    const size_t sbytes = wgrad_swapped_workspace_bytes(n, ho, wo, cin, cout, k, sw);
    if (sbytes != old_wgrad_swapped_workspace_bytes(n, ho, wo, cin, cout, k, e))
      return fail(tag, "se3ds_conv2d_wgrad_swapped_workspace_bytes", (long long)sbytes,
                  (long long)old_wgrad_swapped_workspace_bytes(n, ho, wo, cin, cout, k, e));
    const WgradChoice c = wgrad_swapped_route(dtype, n, ho, wo, cin, cout, k, sw);
    const OldWgrad o = old_wgrad_swapped(dtype, n, ho, wo, cin, cout, k, e);
    const std::string t = std::string(tag) + " swapped";
    if ((int)c.route != o.route) { fprintf(stderr, "%s: route %s, expected %s\n", t.c_str(), kNames[c.route], kNames[o.route]); return false; }
    if (c.splits != o.reduce_splits) return fail(t, "splits", c.splits, o.reduce_splits);
    if (c.steps != o.steps) return fail(t, "steps", c.steps, o.steps);
    if (c.steps_per_split != o.steps_per_split) return fail(t, "steps_per_split", c.steps_per_split, o.steps_per_split);
    if (c.lead_bytes != o.lead) return fail(t, "lead_bytes", (long long)c.lead_bytes, (long long)o.lead);
    if (c.route != kRoute_wgrad_swap_fixup && c.lead_bytes + sizeof(float) * (size_t)c.slabs * (size_t)nel > sbytes)
      return fail(t, "slabs beyond the workspace", c.slabs, (long long)sbytes);
    g_seen[c.route] = true;
    ++g_cases;
  }
  return true;
}

// ---------------------------------------------------------------- the production shapes
// profiles/r06_shapes_b8.txt (batch 8, 512 x 1024, bf16), every fwd / dgrad / wgrad line once: kind,
// k, stride, cin, cout, H x W of the line, n -> the route under the default switches and, for the
// weight gradient, its split count.  The layers pad 'SAME': the output is H / stride rounded up.
struct Pinned { const char* kind; int k, stride, cin, cout, h, w, n; const char* route; int splits; };
static const Pinned kPinned[] = {
    {"wgrad", 3, 1, 1024, 1024, 32, 64, 8, "wgrad_taps3_m16", 2},
    {"dgrad", 3, 1, 1024, 1024, 32, 64, 8, "halo256_dgrad_m16", 0},
    {"fwd", 3, 1, 1024, 1024, 32, 64, 8, "halo256_fwd_m16", 0},
    {"fwd", 3, 1, 128, 128, 512, 1024, 8, "halo128_fwd_m16", 0},
    {"dgrad", 3, 1, 128, 128, 512, 1024, 8, "halo128_dgrad_m16", 0},
    {"fwd", 3, 1, 128, 128, 256, 512, 8, "halo128_fwd_m16", 0},
    {"dgrad", 3, 1, 128, 128, 256, 512, 8, "halo128_dgrad_m16", 0},
    {"wgrad", 3, 1, 128, 128, 512, 1024, 8, "wgrad_taps3_m16", 128},
    {"wgrad", 3, 1, 128, 128, 256, 512, 8, "wgrad_taps3_m16", 128},
    {"dgrad", 1, 1, 2048, 512, 32, 64, 8, "big256_dgrad_m16", 0},
    {"wgrad", 3, 1, 512, 512, 32, 64, 8, "wgrad_taps3_m16", 8},
    {"fwd", 3, 1, 512, 512, 32, 64, 8, "halo128_fwd_m16", 0},
    {"dgrad", 3, 1, 512, 512, 32, 64, 8, "halo128_dgrad_m16", 0},
    {"fwd", 1, 1, 512, 2048, 32, 64, 8, "big256_fwd_m16", 0},
    {"wgrad", 1, 1, 2048, 512, 32, 64, 8, "wgrad_glds_bf16", 8},
    {"wgrad", 1, 1, 512, 2048, 32, 64, 8, "wgrad_glds_bf16", 8},
    {"fwd", 1, 1, 2048, 512, 32, 64, 8, "glds_bf16_fwd_m16", 0},
    {"dgrad", 4, 2, 128, 256, 129, 257, 16, "glds_bf16_dgrad_m16", 0},
    {"dgrad", 1, 1, 512, 2048, 32, 64, 8, "glds_bf16_dgrad_m16", 0},
    {"fwd", 3, 1, 128, 128, 128, 256, 8, "halo128_fwd_m16", 0},
    {"dgrad", 3, 1, 128, 128, 128, 256, 8, "halo128_dgrad_m16", 0},
    {"wgrad", 3, 1, 256, 256, 64, 128, 8, "wgrad_taps3_m16", 27},
    {"wgrad", 3, 1, 128, 128, 128, 256, 8, "wgrad_taps3_m16", 114},
    {"dgrad", 4, 2, 256, 512, 65, 129, 16, "big256_dgrad_m16", 0},
    {"wgrad", 4, 2, 128, 256, 129, 257, 16, "wgrad_glds_bf16", 16},
    {"dgrad", 3, 1, 256, 256, 64, 128, 8, "halo256_dgrad_m16", 0},
    {"wgrad", 4, 2, 256, 512, 65, 129, 16, "wgrad_glds_bf16", 4},
    {"fwd", 3, 1, 256, 256, 64, 128, 8, "halo256_fwd_m16", 0},
    {"fwd", 4, 2, 128, 256, 129, 257, 16, "big256_fwd_m16", 0},
    {"dgrad", 1, 1, 512, 128, 128, 256, 8, "big256_dgrad_m16", 0},
    {"fwd", 4, 2, 256, 512, 65, 129, 16, "glds_bf16_fwd_m16", 0},
    {"fwd", 1, 1, 128, 512, 128, 256, 8, "big256_fwd_m16", 0},
    {"dgrad", 1, 1, 1024, 256, 64, 128, 8, "big256_dgrad_m16", 0},
    {"dgrad", 4, 2, 512, 512, 33, 65, 16, "glds_bf16_dgrad_m16", 0},
    {"wgrad", 3, 1, 128, 1, 512, 1024, 8, "wgrad_bf16", 227},
    {"wgrad", 3, 1, 128, 3, 512, 1024, 8, "wgrad_bf16", 227},
    {"fwd", 4, 2, 512, 512, 33, 65, 16, "glds_bf16_fwd_m16", 0},
    {"fwd", 3, 1, 128, 3, 512, 1024, 8, "thin_cout_fwd", 0},
    {"fwd", 3, 1, 4096, 512, 16, 32, 8, "halo128_fwd_m16", 0},
    {"wgrad", 4, 2, 512, 512, 33, 65, 16, "wgrad_glds_bf16", 2},
    {"fwd", 1, 1, 512, 128, 128, 256, 8, "glds_bf16_fwd_m16", 0},
    {"wgrad", 1, 1, 1024, 256, 64, 128, 8, "wgrad_glds_bf16", 32},
    {"fwd", 1, 1, 256, 1024, 64, 128, 8, "big256_fwd_m16", 0},
    {"wgrad", 1, 1, 128, 512, 128, 256, 8, "wgrad_glds_bf16", 128},
    {"fwd", 3, 1, 128, 1, 512, 1024, 8, "thin_cout_fwd", 0},
    {"wgrad", 1, 1, 512, 128, 128, 256, 8, "wgrad_glds_bf16", 128},
    {"dgrad", 4, 2, 512, 512, 17, 33, 16, "glds_bf16_dgrad_m16", 0},
    {"dgrad", 1, 1, 128, 128, 256, 512, 8, "glds_bf16_dgrad_m16", 0},
    {"fwd", 1, 1, 128, 128, 256, 512, 8, "glds_bf16_fwd_m16", 0},
    {"dgrad", 1, 1, 128, 512, 128, 256, 8, "glds_bf16_dgrad_m16", 0},
    {"dgrad", 3, 1, 128, 3, 512, 1024, 8, "thin_cout_dgrad", 0},
    {"dgrad", 4, 2, 128, 256, 65, 129, 16, "glds_bf16_dgrad_m16", 0},
    {"wgrad", 1, 1, 256, 1024, 64, 128, 8, "wgrad_glds_bf16", 32},
    {"wgrad", 4, 2, 4, 128, 257, 513, 16, "thin_cin_wgrad", 256},
    {"dgrad", 4, 2, 256, 512, 33, 65, 16, "big256_dgrad_m16", 0},
    {"dgrad", 3, 1, 128, 1, 512, 1024, 8, "thin_cout_dgrad", 0},
    {"fwd", 1, 1, 1024, 256, 64, 128, 8, "big256_fwd_m16", 0},
    {"wgrad", 1, 1, 128, 128, 256, 512, 8, "wgrad_glds_bf16", 256},
    {"wgrad", 3, 1, 1024, 512, 32, 64, 8, "wgrad_taps3_m16", 4},
    {"fwd", 4, 2, 4, 128, 257, 513, 16, "thin_cin_fwd", 0},
    {"fwd", 3, 1, 1024, 512, 32, 64, 8, "halo128_fwd_m16", 0},
    {"dgrad", 4, 1, 512, 512, 18, 34, 16, "glds_bf16_dgrad_m16", 0},
    {"fwd", 4, 2, 512, 512, 17, 33, 16, "glds_bf16_fwd_m16", 0},
    {"dgrad", 4, 1, 512, 512, 10, 18, 16, "glds_bf16_dgrad_m16", 0},
    {"wgrad", 4, 2, 512, 512, 17, 33, 16, "wgrad_glds_bf16", 2},
    {"dgrad", 3, 1, 1024, 512, 32, 64, 8, "halo256_dgrad_m16", 0},
    {"fwd", 3, 1, 1024, 1024, 16, 32, 8, "halo128_fwd_m16", 0},
    {"wgrad", 7, 2, 5, 128, 256, 512, 8, "thin_cin_wgrad", 256},
    {"dgrad", 3, 1, 1024, 1024, 16, 32, 8, "halo128_dgrad_m16", 0},
    {"dgrad", 4, 2, 4, 128, 257, 513, 16, "glds_bf16_dgrad_m32", 0},
    {"wgrad", 4, 2, 256, 512, 33, 65, 16, "wgrad_glds_bf16", 4},
    {"fwd", 4, 2, 256, 512, 33, 65, 16, "glds_bf16_fwd_m16", 0},
    {"wgrad", 4, 2, 128, 256, 65, 129, 16, "wgrad_glds_bf16", 16},
    {"fwd", 7, 2, 5, 128, 256, 512, 8, "thin_cin_fwd", 0},
    {"dgrad", 1, 1, 1024, 4096, 16, 32, 8, "glds_bf16_dgrad_m16", 0},
    {"fwd", 4, 2, 128, 256, 65, 129, 16, "big256_fwd_m16", 0},
    {"dgrad", 1, 1, 512, 256, 128, 256, 8, "big256_dgrad_m16", 0},
    {"dgrad", 1, 1, 256, 1024, 64, 128, 8, "big256_dgrad_m16", 0},
    {"wgrad", 1, 1, 1024, 4096, 16, 32, 8, "wgrad_glds_bf16", 2},
    {"dgrad", 1, 2, 512, 1024, 64, 128, 8, "big256_dgrad_m16", 0},
    {"wgrad", 1, 1, 512, 256, 128, 256, 8, "wgrad_glds_bf16", 64},
    {"wgrad", 3, 1, 1024, 1024, 16, 32, 8, "wgrad_taps3_m16", 2},
    {"fwd", 3, 2, 1024, 1024, 16, 32, 8, "glds_bf16_fwd_m16", 0},
    {"wgrad", 3, 2, 1024, 1024, 16, 32, 8, "wgrad_glds_bf16", 1},
    {"dgrad", 1, 2, 2048, 4096, 16, 32, 8, "glds_bf16_dgrad_m16", 0},
    {"fwd", 1, 1, 4096, 1024, 16, 32, 8, "glds_bf16_fwd_m16", 0},
    {"wgrad", 1, 1, 1024, 512, 64, 128, 8, "wgrad_glds_bf16", 16},
    {"dgrad", 1, 2, 1024, 2048, 32, 64, 8, "big256_dgrad_m16", 0},
    {"fwd", 1, 1, 1024, 4096, 16, 32, 8, "big256_fwd_m16", 0},
    {"wgrad", 3, 2, 256, 256, 64, 128, 8, "wgrad_glds_bf16", 14},
    {"dgrad", 1, 1, 1024, 512, 64, 128, 8, "big256_dgrad_m16", 0},
    {"wgrad", 3, 1, 4096, 512, 16, 32, 8, "wgrad_taps3_m16", 1},
    {"wgrad", 3, 2, 512, 512, 32, 64, 8, "wgrad_glds_bf16", 3},
    {"wgrad", 4, 1, 512, 512, 18, 34, 16, "wgrad_glds_bf16", 2},
    {"fwd", 4, 1, 512, 512, 18, 34, 16, "glds_bf16_fwd_m16", 0},
    {"fwd", 3, 1, 512, 512, 16, 32, 8, "halo128_fwd_m16", 0},
    {"dgrad", 3, 1, 512, 512, 16, 32, 8, "halo128_dgrad_m16", 0},
    {"fwd", 1, 1, 512, 256, 128, 256, 8, "big256_fwd_m16", 0},
    {"dgrad", 3, 2, 1024, 1024, 16, 32, 8, "glds_bf16_dgrad_m16", 0},
    {"dgrad", 3, 1, 4096, 512, 16, 32, 8, "halo256_dgrad_m16", 0},
    {"dgrad", 3, 2, 512, 512, 32, 64, 8, "glds_bf16_dgrad_m16", 0},
    {"dgrad", 3, 1, 512, 1024, 16, 32, 8, "halo128_dgrad_m16", 0},
    {"fwd", 1, 2, 512, 1024, 64, 128, 8, "big256_fwd_m16", 0},
    {"fwd", 4, 1, 512, 512, 10, 18, 16, "glds_bf16_fwd_m16", 0},
    {"fwd", 4, 2, 512, 512, 9, 17, 16, "glds_bf16_fwd_m16", 0},
    {"fwd", 3, 1, 1024, 512, 16, 32, 8, "halo128_fwd_m16", 0},
    {"wgrad", 1, 1, 4096, 1024, 16, 32, 8, "wgrad_glds_bf16", 2},
    {"wgrad", 1, 2, 512, 1024, 64, 128, 8, "wgrad_glds_bf16", 16},
    {"dgrad", 3, 2, 256, 256, 64, 128, 8, "big256_dgrad_m16", 0},
    {"dgrad", 1, 1, 4096, 1024, 16, 32, 8, "big256_dgrad_m16", 0},
    {"wgrad", 1, 2, 2048, 4096, 16, 32, 8, "wgrad_glds_bf16", 1},
    {"wgrad", 1, 2, 1024, 2048, 32, 64, 8, "wgrad_glds_bf16", 4},
    {"fwd", 3, 2, 256, 256, 64, 128, 8, "glds_bf16_fwd_m16", 0},
    {"fwd", 4, 1, 512, 1, 18, 34, 16, "glds_bf16_fwd_m32", 0},
    {"fwd", 1, 1, 1024, 512, 64, 128, 8, "big256_fwd_m16", 0},
    {"fwd", 4, 1, 512, 1, 10, 18, 16, "glds_bf16_fwd_m32", 0},
    {"wgrad", 1, 1, 2048, 1024, 32, 64, 8, "wgrad_glds_bf16", 4},
    {"fwd", 3, 2, 512, 512, 32, 64, 8, "glds_bf16_fwd_m16", 0},
    {"wgrad", 4, 2, 4, 128, 129, 257, 16, "thin_cin_wgrad", 256},
    {"fwd", 4, 2, 4, 128, 129, 257, 16, "thin_cin_fwd", 0},
    {"wgrad", 3, 1, 512, 512, 16, 32, 8, "wgrad_taps3_m16", 4},
    {"dgrad", 1, 1, 2048, 1024, 32, 64, 8, "big256_dgrad_m16", 0},
    {"dgrad", 4, 2, 512, 512, 9, 17, 16, "glds_bf16_dgrad_m16", 0},
    {"fwd", 1, 2, 1024, 2048, 32, 64, 8, "glds_bf16_fwd_m16", 0},
    {"fwd", 1, 1, 2048, 1024, 32, 64, 8, "big256_fwd_m16", 0},
    {"wgrad", 1, 1, 1024, 512, 32, 64, 8, "wgrad_glds_bf16", 16},
    {"wgrad", 4, 1, 512, 1, 18, 34, 16, "wgrad_bf16", 8},
    {"fwd", 1, 2, 2048, 4096, 16, 32, 8, "glds_bf16_fwd_m16", 0},
    {"fwd", 3, 1, 512, 1024, 16, 32, 8, "halo128_fwd_m16", 0},
    {"wgrad", 4, 1, 512, 1, 10, 18, 16, "wgrad_bf16", 8},
    {"dgrad", 3, 1, 1024, 512, 16, 32, 8, "halo128_dgrad_m16", 0},
    {"dgrad", 4, 1, 512, 1, 18, 34, 16, "igemm_bf16_dgrad", 0},
    {"dgrad", 4, 1, 512, 1, 10, 18, 16, "igemm_bf16_dgrad", 0},
    {"fwd", 1, 1, 1024, 512, 32, 64, 8, "glds_bf16_fwd_m16", 0},
    {"fwd", 1, 1, 256, 1024, 32, 64, 8, "big256_fwd_m16", 0},
    {"dgrad", 1, 1, 1024, 512, 32, 64, 8, "big256_dgrad_m16", 0},
    {"wgrad", 1, 1, 256, 1024, 32, 64, 8, "wgrad_glds_bf16", 32},
    {"wgrad", 4, 1, 512, 512, 10, 18, 16, "wgrad_glds_bf16", 2},
    {"dgrad", 1, 1, 256, 1024, 32, 64, 8, "glds_bf16_dgrad_m16", 0},
    {"wgrad", 3, 1, 512, 1024, 16, 32, 8, "wgrad_taps3_m16", 3},
    {"wgrad", 3, 1, 1024, 512, 16, 32, 8, "wgrad_taps3_m16", 3},
    {"wgrad", 4, 2, 512, 512, 9, 17, 16, "wgrad_glds_bf16", 1},
    {"dgrad", 1, 1, 128, 128, 128, 256, 8, "glds_bf16_dgrad_m16", 0},
    {"fwd", 1, 1, 128, 128, 128, 256, 8, "glds_bf16_fwd_m16", 0},
    {"dgrad", 4, 2, 4, 128, 129, 257, 16, "glds_bf16_dgrad_m32", 0},
    {"fwd", 1, 1, 512, 256, 16, 32, 8, "glds_bf16_fwd_m16", 0},
    {"wgrad", 1, 1, 128, 128, 128, 256, 8, "wgrad_glds_bf16", 256},
    {"dgrad", 1, 1, 512, 256, 16, 32, 8, "glds_bf16_dgrad_m16", 0},
    {"wgrad", 1, 1, 512, 256, 16, 32, 8, "wgrad_glds_bf16", 16},
};
static bool check_pinned() {
  bool ok = true;
  for (const Pinned& r : kPinned) {
    const int ho = (int)ceil_div(r.h, r.stride), wo = (int)ceil_div(r.w, r.stride);
    const ConvSwitches sw = switches_of(kDefaultSw);
    const char* got = nullptr;
    int splits = 0;
    if (!strcmp(r.kind, "wgrad")) {
      const WgradChoice c = wgrad_route(SE3DS_BF16, r.n, ho, wo, r.cin, r.cout, r.k, r.k, r.stride, 0, kMaskNone, false, sw);
      got = kNames[c.route];
      splits = c.splits;
    } else {
      ConvCall c = {};
      c.mode = !strcmp(r.kind, "fwd") ? MODE_FWD : MODE_DGRAD;
      c.dtype = SE3DS_BF16; c.n = r.n; c.h = r.h; c.w = r.w; c.cin = r.cin; c.ho = ho; c.wo = wo; c.cout = r.cout;
      c.kh = c.kw = r.k; c.stride = r.stride;
      const int total_t = (ho - 1) * r.stride + r.k - r.h, total_l = (wo - 1) * r.stride + r.k - r.w;
      c.pad_t = (total_t > 0 ? total_t : 0) / 2; c.pad_l = (total_l > 0 ? total_l : 0) / 2;
      got = kNames[conv_route(c, sw).route];
    }
    if (strcmp(got, r.route) || splits != r.splits) {
      fprintf(stderr, "pinned %s %dx%ds%d %d->%d @%dx%d n%d: got %s, %d expected %s, %d\n", r.kind, r.k, r.k, r.stride, r.cin,
              r.cout, r.h, r.w, r.n, got, splits, r.route, r.splits);
      ok = false;
    }
  }
  return ok;
}

static bool sweep() {
  const int ks[] = {1, 2, 3, 4, 7}, cins[] = {3, 4, 8, 16, 32, 64, 96, 128, 192, 256, 512, 1024, 2048};
  const int couts[] = {1, 3, 4, 8, 64, 128, 192, 256, 512, 1024, 2048}, ns[] = {1, 8, 16};
  const int hw[][2] = {{8, 16}, {32, 64}, {33, 65}, {129, 257}, {512, 1024}};
  for (int dtype : {SE3DS_F32, SE3DS_BF16})
    for (int k : ks)
      for (int cin : cins)
        for (int cout : couts)
          for (const auto& d : hw)
            for (int n : ns) {
              for (int mode : {(int)MODE_FWD, (int)MODE_DGRAD})
                for (int stride = 1; stride <= 2; ++stride)
                  for (int pad = 0; pad <= 2; ++pad) {
                    if (!(k == 4 && stride == 2) && pad != (k - 1) / 2) continue;
                    const int ho = (d[0] + 2 * pad - k) / stride + 1, wo = (d[1] + 2 * pad - k) / stride + 1;
                    const Shape s = {mode, dtype, n, d[0], d[1], cin, ho, wo, cout, k, stride, pad};
                    for (int mask = 0; mask < 3; ++mask)
                      if (!check_conv_shape(s, mask)) return false;
                  }
              if (!check_wgrad_shape(dtype, n, d[0], d[1], cin, cout, k)) return false;
            }
  for (int r = 0; r < kConvRouteCount; ++r) {
    bool exempt = false;
    for (ConvRoute x : kLaunchedUnconditionally) exempt = exempt || x == r;
    if (g_seen[r] == exempt) {
      fprintf(stderr, "route %s: %s\n", kNames[r], exempt ? "chosen, but listed as launched unconditionally" : "never chosen in the sweep");
      return false;
    }
  }
  return check_pinned();
}

int main(int argc, char** argv) {
  const std::string mode = argc >= 2 ? argv[1] : "";
  if (mode == "corrupt" && argc == 2) {
    g_corrupt = true;
    if (sweep()) {
      fprintf(stderr, "a yardstick with the macro tile before the halo kernel went unnoticed\n");
      return 3;
    }
    return 1;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: %s [corrupt]\n", argv[0]);
    return 2;
  }
  if (!sweep()) return 1;
  printf("conv_route_host_check: %lld cases OK\n", g_cases);
  return 0;
}
