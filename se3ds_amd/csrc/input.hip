// Device-side half of the training input pipeline: everything
// datasets/indoor_datasets.py does between the decoded frames and the batch dict the step
// consumes -- int -> float conversion (:185-228), random band masking of proj_mask (:281-304),
// bilinear / nearest resize (:312-314), horizontal roll + flip (:34-61,:319-324), random crop
// (:326-330) and the batch transform proj_image *= proj_mask, proj_depth *= proj_mask (:577-585)
// -- as ONE gather kernel: an output pixel pulls its sources straight from the raw uint8 / uint16
// frames, no intermediate (resized, rolled, concatenated) tensor is ever written.  HBM bound:
// reads <= 4 taps x 3 B (image) + 13 B of nearest samples, writes 40 B per output pixel.
// The random draws are made on the host (one small parameter row per sample).
// Compiled with -ffp-contract=off: every fp32 op rounds once, as in the reference's op chain.
#include "common.h"
#include "re10k_box_core.h"

namespace se3ds {
namespace {

constexpr int kB = 256;

struct InputXf {
  // raw frames, (N,H0,W0[,C]) row-major
  const uint8_t* image;        // (N,H0,W0,3)
  const uint8_t* proj_image;   // (N,H0,W0,3)
  const uint16_t* depth;       // (N,H0,W0)
  const uint16_t* proj_depth;  // (N,H0,W0)
  const uint8_t* proj_mask;    // (N,H0,W0)
  const uint8_t* blurred_mask; // (N,H0,W0)
  const uint8_t* segmentation; // (N,H0,W0)
  const int32_t* ip;           // [N][8]: rh, rw, roll, flip, crop_y, crop_x, hmode, vmode
  const float* fp;             // [N][4]: hstart, hend, vstart, vend
  int n, h0, w0, h, w;
  float* o_image;       // (N,h,w,3)
  float* o_proj_image;  // (N,h,w,3)
  float* o_proj_mask;   // (N,h,w,1)
  float* o_proj_depth;  // (N,h,w,1)
  float* o_depth;       // (N,h,w,1)
  float* o_blurred;     // (N,h,w,1)
  int32_t* o_seg;       // (N,h,w,1)
};

__device__ __forceinline__ int floormod(int a, int m) {
  int r = a % m;
  return r < 0 ? r + m : r;
}

__global__ void __launch_bounds__(kB)
input_transform_kernel(const InputXf p) {
  const int64_t total = (int64_t)p.n * p.h * p.w;
  const float s8 = 1.0f / 255.0f, s16 = 1.0f / 65535.0f;   // convert_image_dtype scales
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kB) {
    const int b = (int)(i / ((int64_t)p.h * p.w));
    const int rem = (int)(i - (int64_t)b * p.h * p.w);
    const int y = rem / p.w, x = rem - y * p.w;
    const int32_t* ip = p.ip + b * 8;
    const float* fq = p.fp + b * 4;
    const int rh = ip[0], rw = ip[1], roll = ip[2], flip = ip[3];
    // crop -> flip -> roll, backwards: position in the resized frame
    const int yr = y + ip[4];
    int xs = x + ip[5];
    if (flip) xs = rw - 1 - xs;
    const int xr = floormod(xs - roll, rw);
    const int64_t base = (int64_t)b * p.h0 * p.w0;
    // ---- nearest sources (tf.image.resize 'nearest', half-pixel centres)
    const float sy = (float)p.h0 / (float)rh, sx = (float)p.w0 / (float)rw;
    int ny = (int)floorf(((float)yr + 0.5f) * sy);
    int nx = (int)floorf(((float)xr + 0.5f) * sx);
    ny = ny < p.h0 - 1 ? ny : p.h0 - 1;
    nx = nx < p.w0 - 1 ? nx : p.w0 - 1;
    const int64_t q = base + (int64_t)ny * p.w0 + nx;
    float pm = (float)(p.proj_mask[q] > 0 ? 1 : 0);
    // band masks live on the RAW grid (:281-304)
    const float fx = (float)nx, fy = (float)ny;
    if (ip[6] == 1) pm = pm * (((fx > fq[0]) && (fx < fq[1])) ? 1.0f : 0.0f);
    if (ip[6] == 2) pm = pm * (((fx > fq[0]) || (fx < fq[1])) ? 1.0f : 0.0f);
    if (ip[7] == 1) pm = pm * (((fy > fq[2]) && (fy < fq[3])) ? 1.0f : 0.0f);
    const float dpt = (float)p.depth[q] * s16;
    const float pdp = (float)p.proj_depth[q] * s16;
    p.o_proj_mask[i] = pm;
    p.o_depth[i] = dpt;
    p.o_proj_depth[i] = pdp * pm;
    p.o_blurred[i] = (float)(p.blurred_mask[q] > 0 ? 1 : 0);
    p.o_seg[i] = (int32_t)p.segmentation[q];
#pragma unroll
    for (int c = 0; c < 3; ++c) p.o_proj_image[i * 3 + c] = ((float)p.proj_image[q * 3 + c] * s8) * pm;
    // ---- bilinear image (tf.image.resize default), then clip to [0, 1]
    const float srcy = ((float)yr + 0.5f) * sy - 0.5f;
    const float srcx = ((float)xr + 0.5f) * sx - 0.5f;
    const float fly = floorf(srcy), flx = floorf(srcx);
    const float wy = srcy - fly, wx = srcx - flx;
    int y0 = (int)fly, x0 = (int)flx;
    int y1 = y0 + 1, x1 = x0 + 1;
    y0 = y0 < 0 ? 0 : (y0 > p.h0 - 1 ? p.h0 - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > p.h0 - 1 ? p.h0 - 1 : y1);
    x0 = x0 < 0 ? 0 : (x0 > p.w0 - 1 ? p.w0 - 1 : x0);
    x1 = x1 < 0 ? 0 : (x1 > p.w0 - 1 ? p.w0 - 1 : x1);
    const uint8_t* r0 = p.image + (base + (int64_t)y0 * p.w0) * 3;
    const uint8_t* r1 = p.image + (base + (int64_t)y1 * p.w0) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tl = (float)r0[x0 * 3 + c] * s8, tr = (float)r0[x1 * 3 + c] * s8;
      const float bl = (float)r1[x0 * 3 + c] * s8, br = (float)r1[x1 * 3 + c] * s8;
      float v;
      if (rh == p.h0 && rw == p.w0) {
        v = tl;   // identity size: tf.image.resize returns the input
      } else {
        const float top = tl + (tr - tl) * wx;
        const float bot = bl + (br - bl) * wx;
        v = top + (bot - top) * wy;
      }
      p.o_image[i * 3 + c] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Evaluation input pipeline: R2RVideoDataset._transform_fn (datasets/indoor_datasets.py:734-792)
// over all N*T frames of a batch -- bilinear resize of the RGB frames (no clip), the optional band
// mask on the OUTPUT grid (:753-765), nearest resize of the two label and the two depth planes --
// as one gather, no intermediate tensor.  HBM bound; layout of the work:
//   * one workgroup per run of kB output pixels of ONE output row, so everything that depends on
//     the row (frame, example, both source rows, the vertical weight, the band) is wave-uniform and
//     no thread does a 64-bit division;
//   * one thread per output pixel: its taps of one source row are the RGB triples x0 and x1, 12 B
//     each (one dwordx3 load per tap), and neighbouring lanes read neighbouring triples.  At the
//     exact 2x reduction of the shipped configs x0 = 2x, x1 = 2x + 1: a wave's taps are two runs of
//     64 x 24 B = 1536 contiguous bytes without holes, every source row is touched by exactly one
//     output row, so each image byte leaves HBM once (the x0 / x1 loads of a wave share their cache
//     lines in the vector L1);
//   * the stores of a wave are contiguous: 768 B of RGB (x1 or x2), 64 B per label plane, 256 B
//     per depth plane.
struct VideoXf {
  const float* image;      // (N,T,H0,W0,3)
  const uint8_t* seg;      // (N,T,H0,W0)
  const uint8_t* pd_seg;   // (N,T,H0,W0) or NULL (with o_pd_seg)
  const float* depth;      // (N,T,H0,W0)
  const float* pd_depth;   // (N,T,H0,W0) or NULL (with o_pd_depth)
  const int32_t* hmode;    // [N]: 0 none / 1 start < x < end / 2 x > start or x < end
  const float* hband;      // [N][2]: start, end (output-grid pixels)
  int t, h0, w0, h, w;
  float sy, sx;            // (float)h0 / (float)h, (float)w0 / (float)w: divided once, on the host
  float* o_original;      // (N,T,h,w,3)
  float* o_image;          // (N,T,h,w,3) or NULL: no masked copy
  uint8_t* o_seg;          // (N,T,h,w,1)
  uint8_t* o_pd_seg;
  float* o_depth;          // (N,T,h,w,1)
  float* o_pd_depth;
};

struct Rgb { float r, g, b; };   // 12 B, 4-byte aligned: one dwordx3 access

__global__ void __launch_bounds__(kB)
video_transform_kernel(const VideoXf p) {
  const int bpr = (p.w + kB - 1) / kB;          // workgroups per output row
  const int row = (int)blockIdx.x / bpr;        // frame * h + y  (< N * T * h by the grid size)
  const int x = ((int)blockIdx.x - row * bpr) * kB + (int)threadIdx.x;
  if (x >= p.w) return;
  const int f = row / p.h, y = row - f * p.h;
  const float sy = p.sy, sx = p.sx;
  const int64_t fbase = (int64_t)f * p.h0 * p.w0;   // first pixel of the source frame
  const int64_t o = (int64_t)row * p.w + x;         // output pixel
  // ---- nearest planes (tf.image.resize 'nearest', half-pixel centres)
  int ny = (int)floorf(((float)y + 0.5f) * sy);
  int nx = (int)floorf(((float)x + 0.5f) * sx);
  ny = ny < p.h0 - 1 ? ny : p.h0 - 1;
  nx = nx < p.w0 - 1 ? nx : p.w0 - 1;
  const int64_t q = fbase + (int64_t)ny * p.w0 + nx;
  p.o_seg[o] = p.seg[q];
  p.o_depth[o] = p.depth[q];
  if (p.pd_seg) p.o_pd_seg[o] = p.pd_seg[q];
  if (p.pd_depth) p.o_pd_depth[o] = p.pd_depth[q];
  // ---- bilinear image (tf.image.resize default; the video path does not clip)
  const float srcy = ((float)y + 0.5f) * sy - 0.5f;
  const float srcx = ((float)x + 0.5f) * sx - 0.5f;
  const float fly = floorf(srcy), flx = floorf(srcx);
  const float wy = srcy - fly, wx = srcx - flx;
  int y0 = (int)fly, x0 = (int)flx;
  int y1 = y0 + 1, x1 = x0 + 1;
  y0 = y0 < 0 ? 0 : (y0 > p.h0 - 1 ? p.h0 - 1 : y0);
  y1 = y1 < 0 ? 0 : (y1 > p.h0 - 1 ? p.h0 - 1 : y1);
  x0 = x0 < 0 ? 0 : (x0 > p.w0 - 1 ? p.w0 - 1 : x0);
  x1 = x1 < 0 ? 0 : (x1 > p.w0 - 1 ? p.w0 - 1 : x1);
  const Rgb* r0 = reinterpret_cast<const Rgb*>(p.image) + fbase + (int64_t)y0 * p.w0;
  const Rgb* r1 = reinterpret_cast<const Rgb*>(p.image) + fbase + (int64_t)y1 * p.w0;
  Rgb v;
  if (p.h == p.h0 && p.w == p.w0) {
    v = r0[x0];   // identity size: tf.image.resize returns the input
  } else {
    const Rgb tl = r0[x0], tr = r0[x1], bl = r1[x0], br = r1[x1];
    const float tl_[3] = {tl.r, tl.g, tl.b}, tr_[3] = {tr.r, tr.g, tr.b};
    const float bl_[3] = {bl.r, bl.g, bl.b}, br_[3] = {br.r, br.g, br.b};
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float top = tl_[k] + (tr_[k] - tl_[k]) * wx;
      const float bot = bl_[k] + (br_[k] - bl_[k]) * wx;
      c[k] = top + (bot - top) * wy;
    }
    v.r = c[0]; v.g = c[1]; v.b = c[2];
  }
  reinterpret_cast<Rgb*>(p.o_original)[o] = v;
  if (p.o_image) {
    const int b = f / p.t;
    const int mode = p.hmode[b];
    const float start = p.hband[2 * b], end = p.hband[2 * b + 1];
    const float fx = (float)x;
    float m = 1.0f;
    if (mode == 1) m = ((fx > start) && (fx < end)) ? 1.0f : 0.0f;
    if (mode == 2) m = ((fx > start) || (fx < end)) ? 1.0f : 0.0f;
    Rgb vm;
    vm.r = v.r * m; vm.g = v.g * m; vm.b = v.b * m;
    reinterpret_cast<Rgb*>(p.o_image)[o] = vm;
  }
}

// ---------------------------------------------------------------------------------------------
// RE10K training records: `_transform_fn_re10k` (datasets/indoor_datasets.py:377-535) + the batch
// transform (:577-585).  The crop is bounded by the visible pixels of `visible_mask`, which sits
// decoded in HBM, so the box is found here and the host never sees the mask: two launches, no
// synchronisation.
//
// 1. re10k_extent_kernel: first / last row and column holding a visible pixel, per example.
//    A workgroup owns (example, band of kExtBand rows); its kB / 64 waves take the band's rows in
//    turn, a wave reading one row segment of 64 x VB bytes per instruction (VB = 16 when W0 and the
//    plane's address are multiples of 16, so that every row start is 16-byte aligned; else VB = 1).
//    "The row has a visible pixel" is a wave ballot, so the row extents stay wave-uniform; "the
//    column has one" is an OR over the wave's rows kept in the lane's registers, looked at once per
//    segment.  The waves' results meet in LDS, and a workgroup that saw a pixel sends one integer
//    atomicMin / atomicMax per extent word; min and max commute, the result does not depend on
//    the order.  The words are initialised by the caller (H0, -1, W0, -1), in the upload that
//    carries the draw rows.
// 2. re10k_transform_kernel: the gather, in video_transform_kernel's layout -- one workgroup per run
//    of kB output pixels of one output row, so example, box, source rows and vertical weight are
//    wave-uniform.  The box (re10k_box_core.h) is evaluated by every workgroup: a dozen flops
//    against 4 x 20 B of parameters.  Band masks act on the raw grid, then crop [iy0:iy1, ix0:ix1],
//    then tf.image.resize of the CROPPED planes to (h, w): bilinear + clip for `image`, taps clamped
//    at the crop's edges; nearest for every other plane, proj_image included (:491).  With scale 1
//    the bilinear weights are exactly 0 and the tap is returned unchanged, so the no-crop mode (box =
//    frame, (h, w) = (h0, w0)) needs no branch.  Every source coordinate is clamped into the frame
//    whatever the status; an example with a nonzero status gets zeros.
//    Reads per output pixel <= 4 taps x 3 B + 13 B of nearest samples, writes 40 B, as above.
constexpr int kExtBand = 32;                 // rows per workgroup: kExtBand / (kB / 64) per wave
constexpr int kExtRows = kExtBand / (kB / kWave);

template <int VB> struct ExtVec;
template <> struct ExtVec<16> {
  typedef uint4 T;
  static __device__ __forceinline__ T zero() { return make_uint4(0, 0, 0, 0); }
  static __device__ __forceinline__ bool any(const T& v) { return (v.x | v.y | v.z | v.w) != 0; }
  static __device__ __forceinline__ void accumulate(T& a, const T& v) {
    a.x |= v.x; a.y |= v.y; a.z |= v.z; a.w |= v.w;
  }
  // first / last nonzero byte of a nonzero vector (little-endian: byte k of a word is column k)
  static __device__ __forceinline__ int first(const T& v) {
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    int r = 0;
#pragma unroll
    for (int k = 3; k >= 0; --k) if (q[k]) r = 4 * k + (__ffs((int)q[k]) - 1) / 8;
    return r;
  }
  static __device__ __forceinline__ int last(const T& v) {
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    int r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (q[k]) r = 4 * k + (31 - __clz((int)q[k])) / 8;
    return r;
  }
};
template <> struct ExtVec<1> {
  typedef uint8_t T;
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ bool any(const T& v) { return v != 0; }
  static __device__ __forceinline__ void accumulate(T& a, const T& v) { a |= v; }
  static __device__ __forceinline__ int first(const T&) { return 0; }
  static __device__ __forceinline__ int last(const T&) { return 0; }
};

template <int VB>
__global__ void __launch_bounds__(kB)
re10k_extent_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ ext, int h0, int w0) {
  typedef ExtVec<VB> V;
  const int bands = (h0 + kExtBand - 1) / kExtBand;
  const int b = (int)blockIdx.x / bands;             // < n by the grid size
  const int band = (int)blockIdx.x - b * bands;
  const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
  const int row0 = band * kExtBand + wave;           // this wave's rows: row0 + k * (kB / 64)
  const int vecs = w0 / VB;                          // vectors per row (VB divides w0)
  const typename V::T* plane =
      reinterpret_cast<const typename V::T*>(mask + (int64_t)b * h0 * w0);
  int rmin = h0, rmax = -1, cmin = w0, cmax = -1;
  for (int v0 = 0; v0 < vecs; v0 += kWave) {         // segments of 64 vectors along the row
    const int v = v0 + lane;
    typename V::T got[kExtRows];
#pragma unroll
    for (int k = 0; k < kExtRows; ++k) {             // all loads of the segment in flight at once
      const int row = row0 + k * (kB / kWave);
      got[k] = (row < h0 && v < vecs) ? plane[(int64_t)row * vecs + v] : V::zero();
    }
    typename V::T acc = V::zero();
#pragma unroll
    for (int k = 0; k < kExtRows; ++k) {
      const int row = row0 + k * (kB / kWave);
      if (__ballot(V::any(got[k])) != 0) {           // wave-uniform
        rmin = row < rmin ? row : rmin;
        rmax = row > rmax ? row : rmax;
      }
      V::accumulate(acc, got[k]);
    }
    if (V::any(acc)) {
      const int lo = v * VB + V::first(acc), hi = v * VB + V::last(acc);
      cmin = lo < cmin ? lo : cmin;
      cmax = hi > cmax ? hi : cmax;
    }
  }
  cmin = (int)wave_min_u32((uint32_t)cmin);          // >= 0, so the unsigned order is the signed one;
  cmax = (int)wave_max_u32((uint32_t)(cmax + 1)) - 1;   // -1 + 1 = 0 loses against any column
  // One set of atomics per workgroup, not per wave: all atomics of an example land on one 16-byte
  // line and are served one after the other, so their number is what this kernel's time is made of
  // (8 masks of 512 x 1024: 19.1 us with 128 sets per example, 3.9 us with these 16).
  __shared__ int32_t part[kB / kWave][4];
  if (lane == 0) {
    part[wave][0] = rmin; part[wave][1] = rmax; part[wave][2] = cmin; part[wave][3] = cmax;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 1; k < kB / kWave; ++k) {
    rmin = part[k][0] < rmin ? part[k][0] : rmin;
    rmax = part[k][1] > rmax ? part[k][1] : rmax;
    cmin = part[k][2] < cmin ? part[k][2] : cmin;
    cmax = part[k][3] > cmax ? part[k][3] : cmax;
  }
  if (rmax < 0) return;                              // nothing visible in this band
  int32_t* e = ext + (int64_t)b * 4;
  atomicMin(e + 0, rmin);
  atomicMax(e + 1, rmax);
  atomicMin(e + 2, cmin);
  atomicMax(e + 3, cmax);
}

struct Re10kXf {
  const uint8_t* image;        // (N,H0,W0,3)
  const uint8_t* proj_image;   // (N,H0,W0,3)
  const uint16_t* depth;       // (N,H0,W0)
  const uint16_t* proj_depth;  // (N,H0,W0)
  const uint8_t* proj_mask;    // (N,H0,W0)
  const uint8_t* visible;      // (N,H0,W0)
  const uint8_t* segmentation; // (N,H0,W0)
  const int32_t* ext;          // [N][4]: r0, r1, c0, c1 of re10k_extent_kernel, or NULL: no crop
  const int32_t* ip;           // [N][3]: hmode, vmode, crop flag
  const float* fp;             // [N][7]: hstart, hend, vstart, vend, pad, x_shift, y_shift
  int h0, w0, h, w;
  float* o_image;       // (N,h,w,3)
  float* o_proj_image;  // (N,h,w,3)
  float* o_proj_mask;   // (N,h,w,1)
  float* o_proj_depth;  // (N,h,w,1)
  float* o_depth;       // (N,h,w,1)
  float* o_blurred;     // (N,h,w,1)
  int32_t* o_seg;       // (N,h,w,1)
  int32_t* o_bbox;      // [N][4]: x_min, y_min, x_max, y_max, or NULL (with ext)
  int32_t* o_status;    // [N]
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kB)
re10k_transform_kernel(const Re10kXf p) {
  const int bpr = (p.w + kB - 1) / kB;          // workgroups per output row
  const int row = (int)blockIdx.x / bpr;        // example * h + y  (< N * h by the grid size)
  const int x = ((int)blockIdx.x - row * bpr) * kB + (int)threadIdx.x;
  if (x >= p.w) return;
  const int b = row / p.h, y = row - b * p.h;
  const int32_t* ip = p.ip + b * 3;
  const float* fq = p.fp + b * 7;
  // ---- the box: wave-uniform
  Re10kBox box;
  box.x_min = 0; box.y_min = 0; box.x_max = p.w0; box.y_max = p.h0; box.status = kRe10kOk;
  if (p.ext && ip[2]) {
    const int32_t* e = p.ext + b * 4;
    box = re10k_box(e[0], e[1], e[2], e[3], p.h0, p.w0, fq[4], fq[5], fq[6]);
  }
  if (y == 0 && x == 0) {
    p.o_status[b] = box.status;
    if (p.o_bbox) {
      p.o_bbox[b * 4 + 0] = box.x_min; p.o_bbox[b * 4 + 1] = box.y_min;
      p.o_bbox[b * 4 + 2] = box.x_max; p.o_bbox[b * 4 + 3] = box.y_max;
    }
  }
  const int64_t o = (int64_t)row * p.w + x;     // output pixel
  if (box.status != kRe10kOk) {
    p.o_proj_mask[o] = 0.0f; p.o_depth[o] = 0.0f; p.o_proj_depth[o] = 0.0f; p.o_blurred[o] = 0.0f;
    p.o_seg[o] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { p.o_proj_image[o * 3 + c] = 0.0f; p.o_image[o * 3 + c] = 0.0f; }
    return;
  }
  // Inside the frame whatever the words above held: with status 0 these clamps change nothing.
  const int cy = clampi(box.y_min, 0, p.h0 - 1), cx = clampi(box.x_min, 0, p.w0 - 1);
  const int ch = clampi(box.y_max, cy + 1, p.h0) - cy, cw = clampi(box.x_max, cx + 1, p.w0) - cx;
  const float s8 = 1.0f / 255.0f, s16 = 1.0f / 65535.0f;   // convert_image_dtype scales
  const float sy = (float)ch / (float)p.h, sx = (float)cw / (float)p.w;
  const int64_t base = (int64_t)b * p.h0 * p.w0;
  // ---- nearest planes (tf.image.resize 'nearest' of the crop, half-pixel centres)
  int ny = (int)floorf(((float)y + 0.5f) * sy);
  int nx = (int)floorf(((float)x + 0.5f) * sx);
  ny = cy + clampi(ny, 0, ch - 1);
  nx = cx + clampi(nx, 0, cw - 1);
  const int64_t q = base + (int64_t)ny * p.w0 + nx;
  float pm = (float)(p.proj_mask[q] > 0 ? 1 : 0);
  // band masks live on the RAW grid (:389-412)
  const float fx = (float)nx, fy = (float)ny;
  if (ip[0] == 1) pm = pm * (((fx > fq[0]) && (fx < fq[1])) ? 1.0f : 0.0f);
  if (ip[0] == 2) pm = pm * (((fx > fq[0]) || (fx < fq[1])) ? 1.0f : 0.0f);
  if (ip[1] == 1) pm = pm * (((fy > fq[2]) && (fy < fq[3])) ? 1.0f : 0.0f);
  p.o_proj_mask[o] = pm;
  p.o_depth[o] = (float)p.depth[q] * s16;
  p.o_proj_depth[o] = ((float)p.proj_depth[q] * s16) * pm;
  p.o_blurred[o] = 1.0f - (float)(p.visible[q] > 0 ? 1 : 0);   // blurred = 1 - visible (:238)
  p.o_seg[o] = (int32_t)p.segmentation[q];
#pragma unroll
  for (int c = 0; c < 3; ++c) p.o_proj_image[o * 3 + c] = ((float)p.proj_image[q * 3 + c] * s8) * pm;
  // ---- bilinear image of the crop, then clip to [0, 1]
  const float srcy = ((float)y + 0.5f) * sy - 0.5f;
  const float srcx = ((float)x + 0.5f) * sx - 0.5f;
  const float fly = floorf(srcy), flx = floorf(srcx);
  const float wy = srcy - fly, wx = srcx - flx;
  const int y0 = cy + clampi((int)fly, 0, ch - 1), y1 = cy + clampi((int)fly + 1, 0, ch - 1);
  const int x0 = cx + clampi((int)flx, 0, cw - 1), x1 = cx + clampi((int)flx + 1, 0, cw - 1);
  const uint8_t* r0 = p.image + (base + (int64_t)y0 * p.w0) * 3;
  const uint8_t* r1 = p.image + (base + (int64_t)y1 * p.w0) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tl = (float)r0[x0 * 3 + c] * s8, tr = (float)r0[x1 * 3 + c] * s8;
    const float bl = (float)r1[x0 * 3 + c] * s8, br = (float)r1[x1 * 3 + c] * s8;
    const float top = tl + (tr - tl) * wx;
    const float bot = bl + (br - bl) * wx;
    const float v = top + (bot - top) * wy;
    p.o_image[o * 3 + c] = fminf(fmaxf(v, 0.0f), 1.0f);
  }
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" int se3ds_input_transform(const uint8_t* image, const uint8_t* proj_image,
                                     const uint16_t* depth, const uint16_t* proj_depth,
                                     const uint8_t* proj_mask, const uint8_t* blurred_mask,
                                     const uint8_t* segmentation, const int32_t* iparams,
                                     const float* fparams, int n, int h0, int w0, int h, int w,
                                     float* o_image, float* o_proj_image, float* o_proj_mask,
                                     float* o_proj_depth, float* o_depth, float* o_blurred,
                                     int32_t* o_seg, void* stream) {
  if (n <= 0 || h0 <= 0 || w0 <= 0 || h <= 0 || w <= 0) return SE3DS_E_BADSHAPE;
  InputXf p;
  p.image = image; p.proj_image = proj_image; p.depth = depth; p.proj_depth = proj_depth;
  p.proj_mask = proj_mask; p.blurred_mask = blurred_mask; p.segmentation = segmentation;
  p.ip = iparams; p.fp = fparams; p.n = n; p.h0 = h0; p.w0 = w0; p.h = h; p.w = w;
  p.o_image = o_image; p.o_proj_image = o_proj_image; p.o_proj_mask = o_proj_mask;
  p.o_proj_depth = o_proj_depth; p.o_depth = o_depth; p.o_blurred = o_blurred; p.o_seg = o_seg;
  hipLaunchKernelGGL(input_transform_kernel, dim3(grid_for((int64_t)n * h * w, kB)), dim3(kB), 0,
                     as_stream(stream), p);
  return check_launch("input_transform");
}

extern "C" int se3ds_video_transform(const float* image, const uint8_t* segmentation,
                                     const uint8_t* pd_segmentation, const float* depth,
                                     const float* pd_depth, const int32_t* hmode,
                                     const float* hband, int n, int t, int h0, int w0, int h, int w,
                                     float* o_original, float* o_image, uint8_t* o_seg,
                                     uint8_t* o_pd_seg, float* o_depth, float* o_pd_depth,
                                     void* stream) {
  if (n <= 0 || t <= 0 || h0 <= 0 || w0 <= 0 || h <= 0 || w <= 0) return SE3DS_E_BADSHAPE;
  // older records lack the pathdreamer planes: input and output come and go together
  if ((pd_segmentation == nullptr) != (o_pd_seg == nullptr) ||
      (pd_depth == nullptr) != (o_pd_depth == nullptr))
    return SE3DS_E_BADSHAPE;
  if (o_image && (!hmode || !hband)) return SE3DS_E_BADSHAPE;
  const int64_t rows = (int64_t)n * t * h;
  const int64_t blocks = rows * ((w + kB - 1) / kB);
  // rows: int arithmetic in the kernel; blocks * kB: a launch holds fewer than 2^32 threads
  if (rows > INT32_MAX || blocks * kB > (int64_t)UINT32_MAX) return SE3DS_E_BADSHAPE;
  VideoXf p;
  p.image = image; p.seg = segmentation; p.pd_seg = pd_segmentation; p.depth = depth;
  p.pd_depth = pd_depth; p.hmode = hmode; p.hband = hband;
  p.t = t; p.h0 = h0; p.w0 = w0; p.h = h; p.w = w;
  p.sy = (float)h0 / (float)h; p.sx = (float)w0 / (float)w;
  p.o_original = o_original; p.o_image = o_image; p.o_seg = o_seg; p.o_pd_seg = o_pd_seg;
  p.o_depth = o_depth; p.o_pd_depth = o_pd_depth;
  hipLaunchKernelGGL(video_transform_kernel, dim3((unsigned)blocks), dim3(kB), 0, as_stream(stream),
                     p);
  return check_launch("video_transform");
}

// 16 bytes a lane needs every row start 16-byte aligned: the plane's address and W0 both
extern "C" int se3ds_re10k_extent_vector_bytes(const uint8_t* visible_mask, int w0) {
  return (w0 > 0 && w0 % 16 == 0 && reinterpret_cast<uintptr_t>(visible_mask) % 16 == 0) ? 16 : 1;
}

extern "C" int se3ds_re10k_extent(const uint8_t* visible_mask, int n, int h0, int w0,
                                  int32_t* extents, void* stream) {
  if (n <= 0 || h0 <= 0 || w0 <= 0 || !visible_mask || !extents) return SE3DS_E_BADSHAPE;
  const int64_t blocks = (int64_t)n * ((h0 + kExtBand - 1) / kExtBand);
  if (blocks > INT32_MAX) return SE3DS_E_BADSHAPE;
  if (se3ds_re10k_extent_vector_bytes(visible_mask, w0) == 16)
    hipLaunchKernelGGL(re10k_extent_kernel<16>, dim3((unsigned)blocks), dim3(kB), 0,
                       as_stream(stream), visible_mask, extents, h0, w0);
  else
    hipLaunchKernelGGL(re10k_extent_kernel<1>, dim3((unsigned)blocks), dim3(kB), 0,
                       as_stream(stream), visible_mask, extents, h0, w0);
  return check_launch("re10k_extent");
}

extern "C" int se3ds_re10k_transform(const uint8_t* image, const uint8_t* proj_image,
                                     const uint16_t* depth, const uint16_t* proj_depth,
                                     const uint8_t* proj_mask, const uint8_t* visible_mask,
                                     const uint8_t* segmentation, const int32_t* extents,
                                     const int32_t* iparams, const float* fparams, int n, int h0,
                                     int w0, int h, int w, float* o_image, float* o_proj_image,
                                     float* o_proj_mask, float* o_proj_depth, float* o_depth,
                                     float* o_blurred, int32_t* o_seg, int32_t* o_bbox,
                                     int32_t* o_status, void* stream) {
  if (n <= 0 || h0 <= 0 || w0 <= 0 || h <= 0 || w <= 0) return SE3DS_E_BADSHAPE;
  if (!image || !proj_image || !depth || !proj_depth || !proj_mask || !visible_mask ||
      !segmentation || !iparams || !fparams || !o_image || !o_proj_image || !o_proj_mask ||
      !o_proj_depth || !o_depth || !o_blurred || !o_seg || !o_status)
    return SE3DS_E_BADSHAPE;
  // no extents: no example is cropped and there is no box to report; they come and go together
  if ((extents == nullptr) != (o_bbox == nullptr)) return SE3DS_E_BADSHAPE;
  const int64_t rows = (int64_t)n * h;
  const int64_t blocks = rows * ((w + kB - 1) / kB);
  // rows: int arithmetic in the kernel; blocks * kB: a launch holds fewer than 2^32 threads
  if (rows > INT32_MAX || blocks * kB > (int64_t)UINT32_MAX) return SE3DS_E_BADSHAPE;
  Re10kXf p;
  p.image = image; p.proj_image = proj_image; p.depth = depth; p.proj_depth = proj_depth;
  p.proj_mask = proj_mask; p.visible = visible_mask; p.segmentation = segmentation;
  p.ext = extents; p.ip = iparams; p.fp = fparams; p.h0 = h0; p.w0 = w0; p.h = h; p.w = w;
  p.o_image = o_image; p.o_proj_image = o_proj_image; p.o_proj_mask = o_proj_mask;
  p.o_proj_depth = o_proj_depth; p.o_depth = o_depth; p.o_blurred = o_blurred; p.o_seg = o_seg;
  p.o_bbox = o_bbox; p.o_status = o_status;
  hipLaunchKernelGGL(re10k_transform_kernel, dim3((unsigned)blocks), dim3(kB), 0,
                     as_stream(stream), p);
  return check_launch("re10k_transform");
}
