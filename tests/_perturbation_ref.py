"""CHECKER (test infrastructure, not product code): a NumPy restatement of the whole reference
function inference/perturbation_utils.py `get_proportion_invalid_for_depth` (:23-71), one
candidate at a time with NumPy fp32 scalars where the reference has fp32 tensors and Python
floats / ints where it has those.  Written from the reference's text, independently of
se3ds_amd/inference/perturbation_utils.py (which is vectorised over candidates).

What TensorFlow does and NumPy is told to do explicitly:
  * tensor (fp32) <op> Python number: the number is converted to fp32, the op runs in fp32;
  * int(tensor) truncates toward zero;
  * math.sqrt(tensor) runs in binary64 and the result goes back to fp32 in tf.math.atan2.
"""
import math

import numpy as np

F32 = np.float32
DEPTH_SCALE = 20.0   # constants.py:25


def window_and_threshold(position_offset, height, width, distance_padding=0.10):
  """Returns (row0, row1, col0, col1), threshold (fp32), and a dict of the intermediate values."""
  p = np.asarray(position_offset, dtype=F32).reshape(3)
  distance = np.sqrt(np.sum(p ** 2, dtype=F32), dtype=F32)                           # :36

  heading = np.arctan2(-p[0], -p[1])                                                 # :40
  assert heading.dtype == F32
  term_h = (F32(2 * math.pi) * F32(heading <= 0)) % F32(2 * math.pi)                 # :42-43
  heading = F32(heading + term_h)
  if heading < 0:                                                                    # :44-45
    heading = F32(heading + F32(2 * math.pi))
  heading_proportion = F32(heading / F32(2 * math.pi))                               # :46

  delta_xy = math.sqrt(float(F32(F32(p[1] ** 2) + F32(p[0] ** 2))))                  # :48 (binary64)
  elevation = np.arctan2(F32(delta_xy), -p[2])                                       # :49
  assert elevation.dtype == F32
  term_e = (F32(math.pi) * F32(elevation <= 0)) % F32(math.pi)                       # :51-52
  elevation = F32(elevation + term_e)
  if elevation < 0:                                                                  # :53-54
    elevation = F32(elevation + F32(math.pi))
  elevation_proportion = F32(elevation / F32(math.pi))                               # :55

  heading_start = int(F32(heading_proportion * F32(width)))                          # :57
  elevation_start = int(F32(elevation_proportion * F32(height)))                     # :58
  threshold_width = int(30 / 360 * width)                                            # :61
  threshold_height = int(60 / 180 * height)                                          # :62
  rows = slice(max(0, elevation_start - threshold_height),
               min(height, elevation_start + threshold_height))                      # :64-65
  cols = slice(max(0, heading_start - threshold_width),
               min(width, heading_start + threshold_width))                          # :66-67
  r0, r1, _ = rows.indices(height)
  c0, c1, _ = cols.indices(width)
  r1, c1 = max(r0, r1), max(c0, c1)
  threshold = F32(distance + F32(distance_padding))                                  # :69-70
  info = dict(heading=heading, elevation=elevation, term_h=term_h, term_e=term_e,
              heading_start=heading_start, elevation_start=elevation_start,
              threshold_width=threshold_width, threshold_height=threshold_height,
              distance=distance)
  return (r0, r1, c0, c1), threshold, info


def get_proportion_invalid_for_depth(position_offset, depth_image, distance_padding=0.10):
  """The reference function on a NumPy fp32 (H, W) image.  Returns (proportion, count, area);
  proportion is np.mean of the boolean slice (NaN for an empty one)."""
  depth_image = np.asarray(depth_image)
  assert depth_image.dtype == F32 and depth_image.ndim == 2
  height, width = depth_image.shape
  (r0, r1, c0, c1), threshold, _ = window_and_threshold(position_offset, height, width,
                                                        distance_padding)
  region = depth_image[r0:r1, c0:c1]
  with np.errstate(invalid='ignore'):
    hit = (region * F32(DEPTH_SCALE)).astype(F32) < threshold                        # :68-70
  with np.errstate(invalid='ignore', divide='ignore'):
    import warnings
    with warnings.catch_warnings():
      warnings.simplefilter('ignore', RuntimeWarning)
      proportion = float(np.mean(hit))
  return proportion, int(hit.sum()), int(hit.size)


def special_offsets():
  """Axis and diagonal directions with both signs of zero, straight up / down, the zero offset."""
  pz, nz = F32(0.0), F32(-0.0)
  out = []
  for d in (0.5, -0.5):
    for zero in (pz, nz):
      out += [[d, zero, zero], [zero, d, zero]]              # along x, along y
  for dx in (0.5, -0.5):
    for dy in (0.5, -0.5):
      out += [[dx, dy, pz], [dx, dy, nz]]                    # diagonals
  for zero in (pz, nz):
    out += [[zero, zero, 0.7], [zero, zero, -0.7]]           # straight up / down
  out += [[pz, pz, pz], [nz, nz, nz], [pz, nz, pz]]          # the zero offset
  return np.array(out, dtype=F32)


def seeded_offsets(count=48, seed=11):
  rng = np.random.default_rng(seed)
  return rng.uniform([-1.5, -1.5, -0.4], [1.5, 1.5, 0.4], size=(count, 3)).astype(F32)
