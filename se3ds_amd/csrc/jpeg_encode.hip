// Baseline JPEG encode of a whole batch on the device: the panoramas of the VLN augmentation
// (inference/perturbation_utils.py), roll-outs and TensorBoard sheets as the files Pillow's
// Image.save(f, 'JPEG', quality=q, subsampling=s) writes, byte for byte.  The arithmetic is
// jpeg_encode_core.h; this file holds the kernels and the entry.  The container (SOI .. SOS, EOI)
// is put together by the caller (utils/jpeg.py), as png_container is.
//
//   phase 1  jpeg_transform_kernel     one workgroup per tile of up to 240 blocks of one MCU row: the
//            lanes read the tile's pixels in row order, convert every pixel once, downsample and
//            stage the planes in LDS (edge replication on the way); then one lane per 8 x 8 block
//            runs the slow-integer forward DCT from LDS, quantises, applies the dummy-block rule
//            -> int16 coefficients in zig-zag order, blocks in scan order.
//   phase 2  jpeg_measure_kernel       one lane per block, one workgroup per scan group of 256
//            blocks: the block's Huffman bits into its slot (produced once, kept), its length, and
//            the inclusive scan of the group's spans (Hillis-Steele in LDS over `then`).
//            jpeg_group_scan_kernel    one workgroup: the groups' aggregates -> every group's raw
//            bit position.
//   phase 4  jpeg_pack_kernel<false>   one workgroup per unit of 64 blocks: assembles the unit's
//            raw bytes in LDS and counts the FFs to stuff -> the unit's stuffed length.
//            jpeg_unit_scan_kernel     one workgroup: the units' lengths -> their output offsets.
//   phase 8  jpeg_pack_kernel<true>    assembles again, stuffs in LDS, stores 16 bytes a lane to
//            the unit's place; writes where every image starts.
//
// Everything is queued on the caller's stream; no host synchronisation, no global atomics (the
// LDS buffer is assembled with LDS atomic OR, which commutes), integer arithmetic only: the same
// bytes on every run.  LDS: TileShared = 25 KiB, PackShared = 43 KiB static (three workgroups per CU).
#include "common.h"
#include "jpeg_encode_core.h"

namespace se3ds {
namespace {

namespace je = jpeg_encode;
using je::Image;

constexpr int kScanLanes = 256;   // lanes of the two single-workgroup scans

// What the entry derives from the host table.
struct Layout {
  int64_t blocks, groups, units, tiles, segments, out_bytes;
  int64_t coef_at, slot_at, bits_at, inclusive_at, aggregate_at, group_start_at, unit_len_at, unit_start_at,
      bytes;
};

int64_t aligned16(int64_t n) { return (n + 15) & ~(int64_t)15; }

void carve(Layout* l) {
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at = aligned16(at + bytes);
    return here;
  };
  l->coef_at = take(l->blocks * 128);
  l->slot_at = take(l->blocks * je::kBlockWords * 4);
  l->bits_at = take(l->blocks * 2);
  l->inclusive_at = take(l->blocks * (int64_t)sizeof(je::Span32));
  l->aggregate_at = take(l->groups * (int64_t)sizeof(je::Span32));
  l->group_start_at = take((l->groups + 1) * 8);
  l->unit_len_at = take(l->units * 4);
  l->unit_start_at = take((l->units + 1) * 8);
  l->bytes = at;
}

int check_table(const int64_t* host_table, int n, Layout* l) {
  if (n < 1 || n > 65535 || !host_table) return SE3DS_E_BADSHAPE;
  const Image* images = reinterpret_cast<const Image*>(host_table);
  int64_t blocks = 0, segments = 0, out = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    const Image& im = images[i];
    if (im.src == 0 || im.width < 1 || im.height < 1) return SE3DS_E_BADSHAPE;
    if (im.width > 65535 || im.height > 65535) return SE3DS_E_UNSUPPORTED;
    if (im.ncomp != 1 && im.ncomp != 3) return SE3DS_E_BADSHAPE;
    const bool sampling = (im.h0 == 1 && im.v0 == 1) || (im.ncomp == 3 && im.h0 == 2 && (im.v0 == 1 || im.v0 == 2));
    if (!sampling) return SE3DS_E_UNSUPPORTED;
    if (im.restart < 0 || im.restart > 65535 || im.first_block != blocks || im.first_tile != tiles)
      return SE3DS_E_BADSHAPE;
    for (int t = 0; t < 2; ++t)
      for (int k = 0; k < 64; ++k)
        if (im.quant[t][k] < 1 || im.quant[t][k] > 255) return SE3DS_E_BADSHAPE;
    blocks += je::blocks_of(im);
    tiles += je::tiles_of(im);
    segments += je::segments_of(im);
    out += je::out_bound(im);
  }
  if (blocks > 0x7fffffff) return SE3DS_E_UNSUPPORTED;
  l->blocks = blocks;
  l->tiles = tiles;
  l->segments = segments;
  l->out_bytes = aligned16(out);
  l->groups = ceil_div(blocks, je::kScanGroup);
  l->units = ceil_div(blocks, je::kPackBlocks);
  carve(l);
  return SE3DS_OK;
}

__global__ void __launch_bounds__(256)
jpeg_transform_kernel(const Image* __restrict__ table, int n, uint8_t* __restrict__ workspace, Layout l) {
  __shared__ je::TileShared sh;
  const int64_t tile = (int64_t)blockIdx.x;
  const Image& im = table[je::image_of_tile(table, n, tile)];
  const je::Tile t = je::tile_of(im, tile - im.first_tile);
  je::tile_load((int)threadIdx.x, 256, im, t, sh);
  __syncthreads();
  je::tile_dct((int)threadIdx.x, im, t, sh, reinterpret_cast<int16_t*>(workspace + l.coef_at) + im.first_block * 64);
}

__global__ void __launch_bounds__(je::kScanGroup)
jpeg_measure_kernel(const Image* __restrict__ table, int n, int64_t blocks, uint8_t* __restrict__ workspace,
                    Layout l) {
  __shared__ je::Codes codes;
  __shared__ je::Span32 scan[2][je::kScanGroup];
  const int lane = (int)threadIdx.x;
  if (lane < 4) je::build_codes(lane, codes);
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * je::kScanGroup + lane;
  je::Span mine = {0, 0, 0};
  if (b < blocks) {
    const Image& im = table[je::image_of(table, n, b)];
    const je::Place p = je::place_of(im, b - im.first_block);
    const int16_t* coef = reinterpret_cast<const int16_t*>(workspace + l.coef_at);
    const int pred = p.pred_zero ? 0 : coef[je::predictor_block(im, p, b) * 64];
    const int bits = je::encode_block(coef + b * 64, pred, p.comp ? 1 : 0, codes,
                                      reinterpret_cast<uint32_t*>(workspace + l.slot_at) + b * je::kBlockWords);
    reinterpret_cast<uint16_t*>(workspace + l.bits_at)[b] = (uint16_t)bits;
    mine = je::span_of_block(p, bits);
  }
  // inclusive scan over `then`: the identity span for the lanes behind the last block
  int cur = 0;
  scan[0][lane] = je::narrow(mine);
  __syncthreads();
  for (int step = 1; step < je::kScanGroup; step <<= 1) {
    je::Span s = je::widen(scan[cur][lane]);
    if (lane >= step) s = je::then(je::widen(scan[cur][lane - step]), s);
    scan[cur ^ 1][lane] = je::narrow(s);
    cur ^= 1;
    __syncthreads();
  }
  if (b < blocks) reinterpret_cast<je::Span32*>(workspace + l.inclusive_at)[b] = scan[cur][lane];
  if (lane == je::kScanGroup - 1)
    reinterpret_cast<je::Span32*>(workspace + l.aggregate_at)[blockIdx.x] = scan[cur][lane];
}

__global__ void __launch_bounds__(kScanLanes)
jpeg_group_scan_kernel(uint8_t* __restrict__ workspace, Layout l) {
  __shared__ je::Span carry[kScanLanes];
  __shared__ uint64_t carry_pos[kScanLanes];
  const je::Span32* aggregate = reinterpret_cast<const je::Span32*>(workspace + l.aggregate_at);
  uint64_t* group_start = reinterpret_cast<uint64_t*>(workspace + l.group_start_at);
  for (int step = 1; step <= 3; ++step) {
    je::group_scan(step, (int)threadIdx.x, kScanLanes, aggregate, l.groups, carry, carry_pos, group_start);
    __syncthreads();
  }
}

// the units' stuffed lengths -> their offsets in the output; the end behind the last
__global__ void __launch_bounds__(kScanLanes)
jpeg_unit_scan_kernel(uint8_t* __restrict__ workspace, Layout l) {
  __shared__ uint64_t carry[kScanLanes];
  const uint32_t* len = reinterpret_cast<const uint32_t*>(workspace + l.unit_len_at);
  uint64_t* start = reinterpret_cast<uint64_t*>(workspace + l.unit_start_at);
  const int lane = (int)threadIdx.x;
  const int64_t per = ceil_div(l.units, kScanLanes);
  const int64_t from = lane * per < l.units ? lane * per : l.units;
  const int64_t to = from + per < l.units ? from + per : l.units;
  uint64_t sum = 0;
  for (int64_t u = from; u < to; ++u) sum += len[u];
  carry[lane] = sum;
  __syncthreads();
  uint64_t at = 0;
  for (int i = 0; i < lane; ++i) at += carry[i];
  for (int64_t u = from; u < to; ++u) {
    start[u] = at;
    at += len[u];
  }
  if (lane == kScanLanes - 1) start[l.units] = at;
}

template <bool kWrite>
__global__ void __launch_bounds__(je::kPackLanes)
jpeg_pack_kernel(const Image* __restrict__ table, int n, uint8_t* __restrict__ workspace, Layout l,
                 uint8_t* __restrict__ out, int64_t* __restrict__ starts) {
  __shared__ je::PackShared sh;
  const int lane = (int)threadIdx.x;
  const je::Span32* inclusive = reinterpret_cast<const je::Span32*>(workspace + l.inclusive_at);
  const uint64_t* group_start = reinterpret_cast<const uint64_t*>(workspace + l.group_start_at);
  const je::Unit unit = je::unit_of((int64_t)blockIdx.x, l.blocks, inclusive, group_start);
  je::pack_clear(lane, je::kPackLanes, sh);
  __syncthreads();
  je::pack_deposit(lane, je::kPackLanes, unit, table, n, l.blocks, inclusive, group_start,
                   reinterpret_cast<const uint16_t*>(workspace + l.bits_at),
                   reinterpret_cast<const uint32_t*>(workspace + l.slot_at), sh);
  __syncthreads();
  je::pack_count(lane, je::kPackLanes, unit, sh);
  __syncthreads();
  if (!kWrite) {
    if (lane == 0)
      reinterpret_cast<uint32_t*>(workspace + l.unit_len_at)[blockIdx.x] = je::pack_length(je::kPackLanes, unit, sh);
    return;
  }
  const uint64_t at = reinterpret_cast<const uint64_t*>(workspace + l.unit_start_at)[blockIdx.x];
  const uint64_t next = reinterpret_cast<const uint64_t*>(workspace + l.unit_start_at)[blockIdx.x + 1];
  uint8_t* dst = out + at;
  const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  je::pack_stuff(lane, je::kPackLanes, unit, sh, shift, at, starts);
  if (blockIdx.x == 0 && lane == 0) starts[0] = 0;
  __syncthreads();
  je::pack_store(lane, je::kPackLanes, sh, shift, (uint32_t)(next - at), dst);
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_jpeg_encode_fields(void) { return je::kFields; }
extern "C" int se3ds_jpeg_encode_scan_group_blocks(void) { return je::kScanGroup; }
extern "C" int se3ds_jpeg_encode_pack_unit_blocks(void) { return je::kPackBlocks; }
extern "C" int se3ds_jpeg_encode_block_words(void) { return je::kBlockWords; }
extern "C" int se3ds_jpeg_encode_tile_blocks(void) { return je::kTileBlocks; }

extern "C" size_t se3ds_jpeg_encode_workspace_bytes(const int64_t* host_table, int n) {
  Layout l;
  return check_table(host_table, n, &l) == SE3DS_OK ? (size_t)l.bytes : 0;
}

extern "C" int64_t se3ds_jpeg_encode_out_bytes(const int64_t* host_table, int n) {
  Layout l;
  return check_table(host_table, n, &l) == SE3DS_OK ? l.out_bytes : 0;
}

extern "C" int se3ds_jpeg_encode(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                                 int64_t workspace_bytes, uint8_t* out, int64_t out_bytes, int64_t* sizes_dev,
                                 int phases, void* stream) {
  if (!table || !workspace || !out || !sizes_dev || phases < 1 || phases > 15) return SE3DS_E_BADSHAPE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(table) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(sizes_dev) & 7u) != 0)
    return SE3DS_E_BADSHAPE;
  Layout l;
  const int rc = check_table(host_table, n, &l);
  if (rc != SE3DS_OK) return rc;
  if (workspace_bytes < l.bytes) return SE3DS_E_WORKSPACE;
  if (out_bytes < l.out_bytes) return SE3DS_E_BADSHAPE;
  hipStream_t s = as_stream(stream);
  const Image* images = reinterpret_cast<const Image*>(table);
  if (phases & 1) {
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)l.tiles), dim3(256), 0, s, images, n, workspace, l);
    const int launched = check_launch("jpeg_transform");
    if (launched != SE3DS_OK) return launched;
  }
  if (phases & 2) {
    hipLaunchKernelGGL(jpeg_measure_kernel, dim3((unsigned)l.groups), dim3(je::kScanGroup), 0, s, images, n,
                       l.blocks, workspace, l);
    int launched = check_launch("jpeg_measure");
    if (launched != SE3DS_OK) return launched;
    hipLaunchKernelGGL(jpeg_group_scan_kernel, dim3(1), dim3(kScanLanes), 0, s, workspace, l);
    launched = check_launch("jpeg_group_scan");
    if (launched != SE3DS_OK) return launched;
  }
  if (phases & 4) {
    hipLaunchKernelGGL(jpeg_pack_kernel<false>, dim3((unsigned)l.units), dim3(je::kPackLanes), 0, s, images, n,
                       workspace, l, out, sizes_dev);
    int launched = check_launch("jpeg_pack_count");
    if (launched != SE3DS_OK) return launched;
    hipLaunchKernelGGL(jpeg_unit_scan_kernel, dim3(1), dim3(kScanLanes), 0, s, workspace, l);
    launched = check_launch("jpeg_unit_scan");
    if (launched != SE3DS_OK) return launched;
  }
  if (phases & 8) {
    hipLaunchKernelGGL(jpeg_pack_kernel<true>, dim3((unsigned)l.units), dim3(je::kPackLanes), 0, s, images, n,
                       workspace, l, out, sizes_dev);
    const int launched = check_launch("jpeg_pack_write");
    if (launched != SE3DS_OK) return launched;
  }
  return SE3DS_OK;
}
