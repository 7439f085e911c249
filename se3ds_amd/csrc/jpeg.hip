// Baseline JPEG decode of a whole batch on the device: tf.image.decode_jpeg for the panorama input
// path (the VLN augmentation notebook starts from it; Matterport panoramas are JPEG files).  The
// decoder is jpeg_core.h; this file holds its workgroup policy, the three kernels and the entry.
//
//   phase 1  jpeg_entropy_kernel   one workgroup of kLanes = 256 threads per entropy segment (a
//            restart interval, or the whole scan).  The segment is decoded speculatively in windows
//            of 256 chunks of 128 bytes and proven consistent (jpeg_core.h has the argument); the
//            result is int16 coefficients in scan order, de-zig-zagged, DC accumulated.
//   phase 2  jpeg_idct_kernel      one thread per 8 x 8 block: dequantise, inverse DCT, saturate,
//            into component planes padded to whole MCUs.
//   phase 4  jpeg_pixel_kernel     one thread per output pixel: fancy upsampling, colour, crop.
//
// Everything is queued on the caller's stream: one memset of the coefficients (a block that
// straddles two chunks is written by two lanes, so lanes write coefficients, not blocks), then the
// launches.  No host synchronisation, no atomics, integer arithmetic only: the same bytes on every
// run.
//
// LDS of the entropy kernel (jpeg::Shared<256, 128>), static:
//   window 256 x 128 + 28 slack + 4 alignment      32 800 B
//   four code tables (512 x 2 B look-up, canonical) 6 208 B
//   exit states, two buffers                        4 096 B
//   entries last used                               2 048 B
//   summaries (blocks, three DC sums), errors       5 120 B
//   scan groups, carry                                560 B     total 50 832 B (< 80 KiB: three
//                                                               workgroups per CU)
#include "common.h"
#include "jpeg_core.h"

namespace se3ds {
namespace {

using jpeg::Image;
using jpeg::kImageFields;
using jpeg::kSegmentFields;

using EntropyShared = jpeg::Shared<jpeg::kLanes, jpeg::kChunkBytes>;
static_assert(sizeof(EntropyShared) <= 80 * 1024, "the entropy kernel's LDS: under half a CU");

struct BlockPolicy {
  template <class F> __host__ __device__ void each(F f) const {
#if defined(__HIP_DEVICE_COMPILE__)
    f((int)threadIdx.x);
    __syncthreads();
#else
    (void)f;
#endif
  }
  template <class F> __host__ __device__ bool any(F f) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __syncthreads_or((int)f((int)threadIdx.x)) != 0;
#else
    (void)f;
    return false;
#endif
  }
};

__global__ void __launch_bounds__(jpeg::kLanes)
jpeg_entropy_kernel(const uint8_t* __restrict__ buf, int n_images, uint8_t* __restrict__ workspace,
                    int32_t* __restrict__ status) {
  __shared__ EntropyShared shared;
  const int64_t* seg = reinterpret_cast<const int64_t*>(buf) + (int64_t)n_images * kImageFields +
                       (int64_t)blockIdx.x * kSegmentFields;
  const Image& im = reinterpret_cast<const Image*>(buf)[seg[0]];
  const int slots = jpeg::slots_of(im);
  int16_t* coef = reinterpret_cast<int16_t*>(workspace + im.coef_off) + seg[3] * slots * 64;
  jpeg::Decoder<jpeg::kLanes, jpeg::kChunkBytes> decoder(shared, im, buf + seg[1], (uint32_t)seg[2], coef,
                                                         (uint32_t)(seg[4] * slots));
  const BlockPolicy policy;
  const int32_t word = decoder.run(policy);
  if (threadIdx.x == 0) status[blockIdx.x] = word;
}

__global__ void __launch_bounds__(256)
jpeg_idct_kernel(const uint8_t* __restrict__ buf, uint8_t* __restrict__ workspace) {
  const Image& im = reinterpret_cast<const Image*>(buf)[blockIdx.y];
  const int slots = jpeg::slots_of(im), ny = slots == 1 ? 1 : slots - 2;
  const int64_t blocks = jpeg::blocks_of(im);
  const int16_t* coef = reinterpret_cast<const int16_t*>(workspace + im.coef_off);
  uint8_t* planes = workspace + im.plane_off;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks;
       b += (int64_t)gridDim.x * blockDim.x) {
    const int64_t mcu = b / slots;
    const int slot = (int)(b - mcu * slots);
    const int c = slot < ny ? 0 : slot - ny + 1;
    const int bx = c == 0 ? slot % (int)im.h0 : 0, by = c == 0 ? slot / (int)im.h0 : 0;
    const int64_t col = (mcu % im.mcus_x) * jpeg::comp_h(im, c) + bx;
    const int64_t row = (mcu / im.mcus_x) * jpeg::comp_v(im, c) + by;
    uint8_t* plane = planes;
    for (int i = 0; i < c; ++i) plane += jpeg::plane_w(im, i) * jpeg::plane_h(im, i);
    const int64_t pitch = jpeg::plane_w(im, c);
    jpeg::idct_block(coef + b * 64, im.quant[c], plane + row * 8 * pitch + col * 8, pitch);
  }
}

__global__ void __launch_bounds__(256)
jpeg_pixel_kernel(const uint8_t* __restrict__ buf, const uint8_t* __restrict__ workspace) {
  const Image& im = reinterpret_cast<const Image*>(buf)[blockIdx.y];
  const int64_t pixels = im.width * im.height;
  uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(im.dst));
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = i / im.width;
    jpeg::pixel(im, workspace + im.plane_off, dst, i - y * im.width, y);
  }
}

int64_t aligned16(int64_t n) { return (n + 15) & ~(int64_t)15; }

bool image_geometry_ok(const Image& im) {
  if (im.width < 1 || im.width > 65535 || im.height < 1 || im.height > 65535) return false;
  if (im.ncomp != 1 && im.ncomp != 3) return false;
  if (im.h0 < 1 || im.h0 > 2 || im.v0 < 1 || im.v0 > 2 || (im.v0 == 2 && im.h0 != 2)) return false;
  if (im.ncomp == 1 && (im.h0 != 1 || im.v0 != 1)) return false;
  if (im.out_channels != 1 && im.out_channels != 3) return false;
  if (im.mcus_x != ceil_div(im.width, 8 * im.h0) || im.mcus_y != ceil_div(im.height, 8 * im.v0))
    return false;
  return (im.tables & ~(int64_t)0x77) == 0;
}

// T.81 Annex C: the counts are those of a prefix code iff no length runs out of code words.
bool huffman_ok(const uint8_t* counts) {
  uint32_t code = 0, total = 0;
  for (int l = 1; l <= 16; ++l) {
    code += counts[l - 1];
    total += counts[l - 1];
    if (code > (1u << l)) return false;
    code <<= 1;
  }
  return total <= 256;
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_jpeg_decode_fields(void) { return kImageFields; }
extern "C" int se3ds_jpeg_decode_segment_fields(void) { return kSegmentFields; }
extern "C" int se3ds_jpeg_decode_lanes(void) { return jpeg::kLanes; }
extern "C" int se3ds_jpeg_decode_chunk_bytes(void) { return jpeg::kChunkBytes; }

extern "C" size_t se3ds_jpeg_decode_workspace_bytes(const int64_t* host_images, int n_images) {
  if (!host_images || n_images < 1) return 0;
  int64_t total = 0;
  for (int i = 0; i < n_images; ++i) {
    const Image& im = reinterpret_cast<const Image*>(host_images)[i];
    if (!image_geometry_ok(im)) return 0;
    total += aligned16(jpeg::coef_bytes(im)) + aligned16(jpeg::plane_bytes(im));
  }
  return (size_t)total;
}

extern "C" int se3ds_jpeg_decode(const uint8_t* buf, int64_t buf_bytes, uint8_t* workspace,
                                 int64_t workspace_bytes, const int64_t* host_images, int n_images,
                                 const int64_t* host_segments, int n_segments, int32_t* status_dev,
                                 int phases, void* stream) {
  if (n_images <= 0 || n_images > 65535 || n_segments <= 0 || !buf || !workspace || !host_images ||
      !host_segments || !status_dev || phases < 1 || phases > 7)
    return SE3DS_E_BADSHAPE;
  if ((reinterpret_cast<uintptr_t>(buf) & 7u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(status_dev) & 3u) != 0 || workspace_bytes < 0)
    return SE3DS_E_BADSHAPE;
  const int64_t table_bytes = ((int64_t)n_images * kImageFields + (int64_t)n_segments * kSegmentFields) * 8;
  if (buf_bytes < table_bytes) return SE3DS_E_BADSHAPE;
  const Image* images = reinterpret_cast<const Image*>(host_images);
  int64_t need = 0, seg_at = 0, coef_end = 0, plane_end = 0, max_blocks = 0, max_pixels = 0;
  for (int i = 0; i < n_images; ++i) {
    const Image& im = images[i];
    if (!image_geometry_ok(im) || im.dst == 0) return SE3DS_E_BADSHAPE;
    for (int t = 0; t < 4; ++t)
      if (!huffman_ok(im.huff[t])) return SE3DS_E_BADSHAPE;
    if (im.seg_first != seg_at || im.seg_count < 1 || im.seg_count > n_segments - seg_at)
      return SE3DS_E_BADSHAPE;
    seg_at += im.seg_count;
    need += aligned16(jpeg::coef_bytes(im)) + aligned16(jpeg::plane_bytes(im));
    max_blocks = jpeg::blocks_of(im) > max_blocks ? jpeg::blocks_of(im) : max_blocks;
    max_pixels = im.width * im.height > max_pixels ? im.width * im.height : max_pixels;
  }
  if (seg_at != n_segments) return SE3DS_E_BADSHAPE;
  if (workspace_bytes < need) return SE3DS_E_WORKSPACE;
  // the layout: every image's coefficients, ascending and disjoint, then every image's planes
  for (int i = 0; i < n_images; ++i) {
    const Image& im = images[i];
    const int64_t cb = jpeg::coef_bytes(im);
    if ((im.coef_off & 15) != 0 || im.coef_off < coef_end || im.coef_off > workspace_bytes ||
        cb > workspace_bytes - im.coef_off)
      return SE3DS_E_BADSHAPE;
    coef_end = im.coef_off + cb;
  }
  plane_end = coef_end;
  for (int i = 0; i < n_images; ++i) {
    const Image& im = images[i];
    const int64_t pb = jpeg::plane_bytes(im);
    if ((im.plane_off & 15) != 0 || im.plane_off < plane_end || im.plane_off > workspace_bytes ||
        pb > workspace_bytes - im.plane_off)
      return SE3DS_E_BADSHAPE;
    plane_end = im.plane_off + pb;
  }
  for (int i = 0; i < n_images; ++i) {
    const Image& im = images[i];
    int64_t mcu = 0;
    for (int64_t s = im.seg_first; s < im.seg_first + im.seg_count; ++s) {
      const int64_t* d = host_segments + s * kSegmentFields;
      const int64_t off = d[1], len = d[2];
      if (d[0] != i || d[3] != mcu || d[4] < 1 || d[4] > im.mcus_x * im.mcus_y - mcu) return SE3DS_E_BADSHAPE;
      if (off < table_bytes || off > buf_bytes || len < 0 || len > jpeg::kMaxSegmentBytes ||
          len > buf_bytes - off)
        return SE3DS_E_BADSHAPE;
      mcu += d[4];
    }
    if (mcu != im.mcus_x * im.mcus_y) return SE3DS_E_BADSHAPE;
  }
  hipStream_t s = as_stream(stream);
  if (phases & 1) {
    const int64_t from = images[0].coef_off;
    if (hipMemsetAsync(workspace + from, 0, (size_t)(coef_end - from), s) != hipSuccess)
      return check_launch("jpeg_decode memset");
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_segments), dim3(jpeg::kLanes), 0, s, buf,
                       n_images, workspace, status_dev);
    const int rc = check_launch("jpeg_entropy");
    if (rc != SE3DS_OK) return rc;
  }
  if (phases & 2) {
    const unsigned gx = (unsigned)grid_for(max_blocks, 256);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx, (unsigned)n_images), dim3(256), 0, s, buf, workspace);
    const int rc = check_launch("jpeg_idct");
    if (rc != SE3DS_OK) return rc;
  }
  if (phases & 4) {
    const unsigned gx = (unsigned)grid_for(max_pixels, 256);
    hipLaunchKernelGGL(jpeg_pixel_kernel, dim3(gx, (unsigned)n_images), dim3(256), 0, s, buf, workspace);
    const int rc = check_launch("jpeg_pixel");
    if (rc != SE3DS_OK) return rc;
  }
  return SE3DS_OK;
}
