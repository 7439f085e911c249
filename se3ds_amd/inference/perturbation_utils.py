"""VLN perturbation augmentation -- MI355X implementation of the reference's
inference/perturbation_utils.py and of the loop of notebooks/SE3DS_VLN_Augmentation_Colab.ipynb
(cell 13): draw a random offset, ask the source depth panorama which share of the pixels in the
direction of travel would collide, and render the panorama at the perturbed position when that
share is small.

The split: the candidates are drawn on the host, so the index math (`collision_windows`) runs
there too, in NumPy fp32, microseconds and no synchronisation; the counting over the depth
panorama is one launch of libse3ds_hip.so `se3ds_collision_count` (csrc/perturb.hip) for all K
candidates; the rendering is `SE3DSModel`.  There is no CPU fallback for the device half."""
import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd import constants

F32 = np.float32


def _host_offsets(position_offsets):
  if isinstance(position_offsets, torch.Tensor):
    position_offsets = position_offsets.detach().cpu().numpy()
  off = np.asarray(position_offsets, dtype=F32)
  if off.ndim != 2 or off.shape[1] != 3:
    raise ValueError(f'position_offsets must be (K, 3), got {off.shape}')
  if not np.all(np.isfinite(off)):
    raise ValueError('position_offsets must be finite (the reference\'s int() raises on NaN / inf)')
  return off


def collision_windows(position_offsets, height, width):
  """The window of the depth panorama the reference looks at for each offset, and the distance of
  travel: int32 (K, 4) rows of [row0, row1, col0, col1] (half-open, as the slice of reference
  inference/perturbation_utils.py:63-67) and fp32 (K,) `distance` (:36).

  `position_offsets` is (K, 3) fp32 on the host (NumPy array or CPU tensor).  The function restates
  :36-67 operation by operation in NumPy fp32, including what the reference does by accident:

    * :42-43 and :51-52, `x + c * cast(x <= 0) % c`: `%` binds before `+` and `(c * 1) % c == 0`,
      so both "map to [0, c]" terms add 0 for every input.  They are computed here as written.
    * :44-45 and :53-54: only the `if x < 0: x += c` branches act (the elevation one never: atan2
      of a non-negative first argument is >= 0).
    * :40: negating +0.0 gives -0.0, so [0, d, 0] has heading atan2(-0., -d) = -pi -> +pi (column
      start width / 2), while a -0.0 in the offset gives +pi directly; :49 likewise: z = +0.0
      gives atan2(delta, -0.) and the zero offset atan2(0, -0.) = pi, i.e. row start `height`.
    * :48: delta_xy is an fp32 sum of two fp32 squares, then math.sqrt in binary64, rounded back
      to fp32 by atan2 -- the same number as a correctly rounded fp32 square root.
    * :57-58: int() truncates the fp32 product proportion * size (the Python int is converted to
      fp32 first).
    * :61-62: the thresholds int(30 / 360 * width), int(60 / 180 * height) are Python doubles.
    * :64-67: the window is clipped at the image border with max / min, never wrapped across the
      seam of the panorama, and it may be empty (height < 3 gives a row threshold of 0).

  :36 `reduce_sum(x ** 2) ** 0.5` is taken as the fp32 sum in order followed by a square root.
  The windows rest on NumPy's fp32 arctan2; TensorFlow's may differ in the last place, which
  matters only where proportion * size falls on an integer."""
  off = _host_offsets(position_offsets)
  height, width = int(height), int(width)
  if height <= 0 or width <= 0:
    raise ValueError(f'bad image size {height} x {width}')
  x, y, z = off[:, 0], off[:, 1], off[:, 2]
  two_pi, pi = F32(2 * math.pi), F32(math.pi)
  with np.errstate(invalid='ignore'):
    distance = np.sqrt(((x * x) + (y * y)) + (z * z))                              # :36
    heading = np.arctan2(-x, -y)                                                   # :40
    heading = heading + (two_pi * (heading <= 0).astype(F32)) % two_pi             # :42-43 (+ 0)
    heading = np.where(heading < 0, heading + two_pi, heading)                     # :44-45
    heading_proportion = heading / two_pi                                          # :46
    delta_xy = np.sqrt((y * y) + (x * x))                                          # :48
    elevation = np.arctan2(delta_xy, -z)                                           # :49
    elevation = elevation + (pi * (elevation <= 0).astype(F32)) % pi               # :51-52 (+ 0)
    elevation = np.where(elevation < 0, elevation + pi, elevation)                 # :53-54
    elevation_proportion = elevation / pi                                          # :55
  assert heading.dtype == F32 and elevation.dtype == F32 and distance.dtype == F32
  heading_start = np.trunc(heading_proportion * F32(width)).astype(np.int64)       # :57
  elevation_start = np.trunc(elevation_proportion * F32(height)).astype(np.int64)  # :58
  threshold_width = int(30 / 360 * width)                                          # :61
  threshold_height = int(60 / 180 * height)                                        # :62
  windows = np.empty((off.shape[0], 4), np.int32)
  windows[:, 0] = np.maximum(0, elevation_start - threshold_height)                # :64-67
  windows[:, 1] = np.minimum(height, elevation_start + threshold_height)
  windows[:, 2] = np.maximum(0, heading_start - threshold_width)
  windows[:, 3] = np.minimum(width, heading_start + threshold_width)
  # a[lo:hi] with hi < lo is empty (cannot happen for starts in [0, size]; kept as the slice has it)
  windows[:, 1] = np.maximum(windows[:, 1], windows[:, 0])
  windows[:, 3] = np.maximum(windows[:, 3], windows[:, 2])
  return windows, distance.astype(F32)


class ProportionInvalid(NamedTuple):
  """Device tensors of `get_proportion_invalid_batch`, one entry per candidate."""
  count: torch.Tensor        # int32: pixels of the window closer than distance + padding
  area: torch.Tensor         # int32: pixels of the window
  proportion: torch.Tensor   # float64: count / area (NaN for an empty window, as np.mean of nothing)


def get_proportion_invalid_batch(position_offsets, depth_images, image_index=None,
                                 distance_padding=0.10) -> ProportionInvalid:
  """`get_proportion_invalid_for_depth` for K offsets in one kernel launch.

  position_offsets: (K, 3) on the host.  depth_images: fp32 (H, W) or (N, H, W) on the device,
  values in [0, 1].  image_index: K indices into N on the host (None: image 0 for every
  candidate).  Returns device tensors and does not wait for the device: one small host-to-device
  copy of the window table, one launch, one division."""
  _lib.require_cuda(depth_images)
  if depth_images.dtype != torch.float32:
    raise ValueError(f'depth_images must be float32, got {depth_images.dtype}')
  if depth_images.ndim == 2:
    depth_images = depth_images[None]
  if depth_images.ndim != 3:
    raise ValueError(f'depth_images must be (H, W) or (N, H, W), got {tuple(depth_images.shape)}')
  depth_images = depth_images.contiguous()
  n, height, width = depth_images.shape
  windows, distance = collision_windows(position_offsets, height, width)
  k = windows.shape[0]
  if k == 0:
    raise ValueError('no candidates')
  threshold = distance + F32(distance_padding)                                     # :69-70, fp32
  if image_index is None:
    index = np.zeros((k,), np.int32)
  else:
    if isinstance(image_index, torch.Tensor):
      image_index = image_index.detach().cpu().numpy()
    index = np.ascontiguousarray(image_index, dtype=np.int32)
    if index.shape != (k,):
      raise ValueError(f'image_index must be ({k},), got {index.shape}')
  L = _lib.lib()
  as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  _lib.check(L.se3ds_collision_check_windows(as_p(windows), as_p(index), n, height, width, k),
             'se3ds_collision_check_windows')
  # one table, one copy: windows (4K) | image index (K) | threshold bits (K) | area (K)
  area = (windows[:, 1] - windows[:, 0]) * (windows[:, 3] - windows[:, 2])
  table = np.concatenate([windows.reshape(-1), index, threshold.view(np.int32),
                          area.astype(np.int32)])
  dev = torch.from_numpy(table).to(depth_images.device)
  d_windows, d_index = dev[:4 * k], dev[4 * k:5 * k]
  d_threshold, d_area = dev[5 * k:6 * k].view(torch.float32), dev[6 * k:7 * k]
  count = torch.empty((k,), dtype=torch.int32, device=depth_images.device)
  _lib.check(L.se3ds_collision_count(
      depth_images.data_ptr(), n, height, width, d_windows.data_ptr(), d_index.data_ptr(),
      d_threshold.data_ptr(), float(constants.DEPTH_SCALE), k, count.data_ptr(), _lib.stream()),
      'se3ds_collision_count')
  proportion = count.to(torch.float64) / d_area.to(torch.float64)   # 0 / 0 = NaN
  return ProportionInvalid(count=count, area=d_area, proportion=proportion)


def get_proportion_invalid_for_depth(position_offset, depth_image, distance_padding=0.10):
  """Returns the proportion of collided pixels when moving in a given direction (reference :23-71).

  position_offset: (3,) relative xyz position to move towards.  depth_image: (H, W) fp32 on the
  device, values in [0, 1].  distance_padding: maximum threshold in metres between camera and an
  object.  Returns a Python float, count / area in binary64 (np.mean of the boolean slice); NaN
  for an empty window."""
  if isinstance(position_offset, torch.Tensor):
    position_offset = position_offset.detach().cpu().numpy()
  offset = np.asarray(position_offset, dtype=F32).reshape(1, 3)
  if depth_image.ndim != 2:
    raise ValueError(f'depth_image must be (H, W), got {tuple(depth_image.shape)}')
  res = get_proportion_invalid_batch(offset, depth_image, None, distance_padding)
  count, area = int(res.count.cpu()[0]), int(res.area.cpu()[0])
  return count / area if area else float('nan')


def draw_candidates(rng, count, xy_perturb=1.5, z_perturb=0.1):
  """`count` candidate offsets from `rng` (a numpy Generator), uniform in
  [-xy, xy] x [-xy, xy] x [-z, z] (cell 13's tf.random.uniform with minval / maxval per axis):
  fp32 (count, 3).  Pure: the stream of a seed is the same with and without a device."""
  hi = np.array([xy_perturb, xy_perturb, z_perturb], np.float64)
  return rng.uniform(-hi, hi, size=(int(count), 3)).astype(F32)


class Augmentation(NamedTuple):
  images: torch.Tensor              # uint8 (S, H, W, 3): pred_rgb at the accepted positions
  positions: torch.Tensor           # fp32 (S, 3): start_pos + offset
  offsets: np.ndarray               # fp32 (S, 3)
  proportion_invalid: np.ndarray    # float64 (S,)
  num_drawn: int                    # candidates looked at, up to and including the last accepted one


def perturbation_augment(model, num_samples, start_pos, depth, xy_perturb=1.5, z_perturb=0.1,
                         max_proportion_invalid=0.02, distance_padding=0.1, seed=0,
                         candidates_per_round=64, max_rounds=16, views_per_forward=1) -> Augmentation:
  """The augmentation loop of notebook cell 13 for one panorama.

  model: an SE3DSModel whose memory already holds the context panorama.  start_pos: (1, 3) device
  tensor, the panorama's position.  depth: its depth map, (H, W) or (1, H, W) on the device.
  Candidates come from numpy.random.default_rng(seed) in rounds of `candidates_per_round`
  (`draw_candidates`); a round is screened by one `get_proportion_invalid_batch` launch and one
  read-back of its K proportions.  Accepted are the first `num_samples` candidates in draw order
  with proportion < max_proportion_invalid (a NaN is never accepted).  The notebook loops until it
  has enough; here RuntimeError is raised after `max_rounds` rounds.

  views_per_forward = 1 renders each accepted position with model(pos, add_preds_to_memory=False);
  B > 1 renders B positions per generator forward (SE3DSModel.predict_views)."""
  if num_samples < 1 or candidates_per_round < 1 or max_rounds < 1 or views_per_forward < 1:
    raise ValueError('num_samples, candidates_per_round, max_rounds, views_per_forward must be >= 1')
  _lib.require_cuda(start_pos, depth)
  if depth.ndim == 3 and depth.shape[0] == 1:
    depth = depth[0]
  if depth.ndim != 2:
    raise ValueError(f'depth must be (H, W) or (1, H, W), got {tuple(depth.shape)}')
  start_pos = start_pos.to(torch.float32).reshape(1, 3)
  rng = np.random.default_rng(seed)
  offsets, proportions, seen, num_drawn = [], [], 0, 0
  for _ in range(max_rounds):
    cand = draw_candidates(rng, candidates_per_round, xy_perturb, z_perturb)
    prop = get_proportion_invalid_batch(cand, depth, None, distance_padding).proportion.cpu().numpy()
    for c in range(candidates_per_round):
      if prop[c] < max_proportion_invalid:   # False for NaN
        offsets.append(cand[c])
        proportions.append(prop[c])
        num_drawn = seen + c + 1
        if len(offsets) == num_samples:
          break
    seen += candidates_per_round
    if len(offsets) == num_samples:
      break
  else:
    raise RuntimeError(
        f'perturbation_augment: {len(offsets)} of {num_samples} samples after {max_rounds} rounds of '
        f'{candidates_per_round} candidates with proportion_invalid < {max_proportion_invalid}: the '
        'panorama leaves no room to move (or max_rounds is too small)')
  offsets = np.stack(offsets).astype(F32)
  positions = start_pos + torch.from_numpy(offsets).to(start_pos.device)   # (S, 3), fp32 add
  images = []
  if views_per_forward == 1:
    for s in range(num_samples):
      images.append(model(positions[s:s + 1], add_preds_to_memory=False).pred_rgb)
  else:
    for s in range(0, num_samples, views_per_forward):
      images.append(model.predict_views(positions[s:s + views_per_forward]).pred_rgb)
  return Augmentation(images=torch.cat(images, dim=0), positions=positions, offsets=offsets,
                      proportion_invalid=np.asarray(proportions, np.float64), num_drawn=num_drawn)


def save_augmentation(aug: Augmentation, directory, prefix='aug', quality=90, subsampling='4:2:0'):
  """Writes what `perturbation_augment` returned the way a VLN training set stores panoramas:
  `<prefix>_<i>.jpg` for every image, all encoded on the device in one call
  (utils.jpeg.encode_jpeg_batch), and `<prefix>.npz` with positions, offsets, proportion_invalid and
  num_drawn.  Every file is written under a temporary name, synced and renamed
  (npz_writer.write_bytes_atomic), so a reader never sees a partial one.  Returns the paths, the images' first and the .npz last."""
  import os
  from se3ds_amd.utils import jpeg, npz_writer
  files = jpeg.encode_jpeg_batch(list(aug.images), quality=quality, subsampling=subsampling)
  os.makedirs(directory, exist_ok=True)
  paths = []
  for i, data in enumerate(files):
    path = os.path.join(directory, f'{prefix}_{i}.jpg')
    npz_writer.write_bytes_atomic(path, data)
    paths.append(path)
  path = os.path.join(directory, f'{prefix}.npz')
  npz_writer.savez(path, {
      'positions': aug.positions.detach().cpu().numpy(), 'offsets': np.asarray(aug.offsets),
      'proportion_invalid': np.asarray(aug.proportion_invalid), 'num_drawn': np.asarray(aug.num_drawn, np.int64)})
  return paths + [path]
