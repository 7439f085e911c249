// The crop box of `_transform_fn_re10k` (datasets/indoor_datasets.py:445-472): extents of the visible
// pixels + the three draws -> [x_min, y_min, x_max, y_max] in pixels and a status.  One definition,
// used by re10k_transform_kernel (input.hip) and, as plain C++, by tools/re10k_box_check.cpp.
//
// All fp32, every operation rounded once, left to right as Python evaluates the reference's
// expressions; compile with -ffp-contract=off.  The division must be correctly rounded: at H = 100,
// trunc((53 / 100) * 100) is 52, and a reciprocal multiply would give 53.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3DS_HD __host__ __device__
#else
#define SE3DS_HD
#endif

namespace se3ds {

enum Re10kStatus : int32_t {
  kRe10kOk = 0,
  kRe10kBlank = 1,    // no visible pixel: the reference indexes an empty tensor (:445)
  kRe10kOutside = 2,  // the box leaves the frame: tf.image.crop_to_bounding_box refuses it (:477)
};

struct Re10kBox {
  int32_t x_min, y_min, x_max, y_max;   // the order of the reference's bbox (:520)
  int32_t status;
};

// tf.cast(float32 -> int32): truncation toward zero.  Values no draw in the reference's ranges
// reaches (|v| > 2^30, NaN) are pinned so that the conversion is defined; the clamps below take
// them into the frame or to status 2.
SE3DS_HD inline int32_t re10k_trunc(float v) {
  if (!(v > -1073741824.0f)) return -1073741824;
  if (v > 1073741824.0f) return 1073741824;
  return (int32_t)v;
}

// r0 / r1: first / last row holding a visible pixel, c0 / c1: first / last such column (r1 < r0 or
// c1 < c0: none), of a height x width frame.
SE3DS_HD inline Re10kBox re10k_box(int32_t r0, int32_t r1, int32_t c0, int32_t c1, int32_t height,
                                   int32_t width, float pad, float x_shift, float y_shift) {
  const float fh = (float)height, fw = (float)width;
  float y_min = ((float)r0 / fh - pad) + y_shift;
  float y_max = ((float)r1 / fh + pad) + y_shift;
  float x_min = (float)c0 / fw;
  float x_max = (float)c1 / fw;
  // normalised coordinates have the 2 : 1 aspect ratio built in
  const float new_h = y_max - y_min;
  const float pad_w = (new_h - (x_max - x_min)) / 2.0f;
  x_max = (x_max + pad_w) + x_shift;
  x_min = (x_min - pad_w) + x_shift;
  int32_t iy0 = re10k_trunc(y_min * fh), ix0 = re10k_trunc(x_min * fw);
  int32_t iy1 = re10k_trunc(y_max * fh), ix1 = re10k_trunc(x_max * fw);
  iy0 = iy0 > 0 ? iy0 : 0;
  ix0 = ix0 > 0 ? ix0 : 0;
  iy1 = iy1 < height ? iy1 : height;
  ix1 = ix1 < width ? ix1 : width;
  iy1 = iy1 > iy0 + 1 ? iy1 : iy0 + 1;
  ix1 = ix1 > ix0 + 1 ? ix1 : ix0 + 1;
  Re10kBox b;
  b.x_min = ix0; b.y_min = iy0; b.x_max = ix1; b.y_max = iy1;
  b.status = (r1 < r0 || c1 < c0) ? kRe10kBlank
             : (iy1 > height || ix1 > width) ? kRe10kOutside : kRe10kOk;
  return b;
}

}  // namespace se3ds
