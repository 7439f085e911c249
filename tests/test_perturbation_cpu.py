"""Host half of the VLN perturbation augmentation (se3ds_amd/inference/perturbation_utils.py):
`collision_windows` and the candidate stream, against the NumPy restatement of the reference
function (tests/_perturbation_ref.py) and the reference's own known answers
(inference/perturbation_utils_test.py).  No GPU: the counting here is the restatement's."""
import math

import numpy as np
import pytest

import _perturbation_ref as ref
from se3ds_amd.inference import perturbation_utils as pu

F32 = np.float32
H, W = 64, 128


def _proportion_from_windows(offset, depth, padding=0.10):
  """collision_windows + the restatement's compare on the window it returns."""
  win, dist = pu.collision_windows(np.asarray(offset, F32).reshape(1, 3), *depth.shape)
  r0, r1, c0, c1 = (int(v) for v in win[0])
  thr = F32(dist[0] + F32(padding))
  return float(np.mean((depth[r0:r1, c0:c1] * F32(ref.DEPTH_SCALE)).astype(F32) < thr))


def _both(offset, depth):
  a = ref.get_proportion_invalid_for_depth(offset, depth)[0]
  b = _proportion_from_windows(offset, depth)
  assert a == b
  return a


@pytest.mark.parametrize('distance,depth_distance,expected', [(0.5, 0.5, 1.0), (0.3, 0.5, 0.0)])
def test_reference_uniform_depth(distance, depth_distance, expected):
  """perturbation_utils_test.py:30-40."""
  depth = np.full((H, W), depth_distance / ref.DEPTH_SCALE, F32)
  assert _both([0.0, distance, 0.0], depth) == expected


def _patch(r0, r1, c0, c1):
  depth = np.full((H, W), 1.0, F32)
  depth[r0:r1, c0:c1] = 0.0
  return depth


def test_reference_offset_forward():
  """perturbation_utils_test.py:42-66."""
  assert _both([0.0, 0.5, 0.0], _patch(22, 42, 54, 74)) > 0.0
  assert _both([0.0, 0.5, 0.0], _patch(0, 10, 0, 10)) == 0.0


def test_reference_offset_diagonal():
  """perturbation_utils_test.py:68-94."""
  hs, ws = int(H * 3 / 4), int(W * 3 / 4)
  assert (hs, ws) == (48, 96)
  assert _both([0.5, 0.5, 0.0], _patch(hs - 10, hs + 10, ws - 10, ws + 10)) > 0.0
  assert _both([0.5, 0.5, 0.0], _patch(0, 10, 0, 10)) == 0.0


def test_pinned_windows_64x128():
  """Derived by hand from the reference: [0, .5, 0] has heading atan2(-0., -.5) = -pi -> +pi,
  proportion 0.5, column start 64; elevation atan2(.5, -0.) = pi / 2, row start 32; thresholds
  int(128 / 12) = 10 and int(64 / 3) = 21."""
  win, dist = pu.collision_windows(np.array([[0, .5, 0], [.5, .5, 0], [0, 0, 0]], F32), H, W)
  assert win.dtype == np.int32 and win.shape == (3, 4) and dist.dtype == F32
  assert win[0].tolist() == [11, 53, 54, 74]
  _, _, info = ref.window_and_threshold([0, .5, 0], H, W)
  assert (info['elevation_start'], info['heading_start']) == (32, 64)
  assert (info['threshold_height'], info['threshold_width']) == (21, 10)
  # [.5, .5, 0]: heading atan2(-.5, -.5) = -3 pi / 4 -> 5 pi / 4, proportion 0.625, start 80
  assert win[1].tolist() == [11, 53, 70, 90]
  assert ref.window_and_threshold([.5, .5, 0], H, W)[2]['heading_start'] == 80
  # the zero offset: elevation atan2(0, -0.) = pi, row start = height, window [height - 21, height)
  _, _, info0 = ref.window_and_threshold([0, 0, 0], H, W)
  assert info0['elevation'] == F32(math.pi) and info0['elevation_start'] == H
  assert win[2, :2].tolist() == [H - 21, H]
  assert dist[0] == F32(0.5) and dist[2] == 0


def test_empty_row_range_2x24():
  win, _ = pu.collision_windows(ref.special_offsets(), 2, 24)
  assert np.all(win[:, 0] == win[:, 1])          # int(60 / 180 * 2) == 0
  assert np.all(win[:, 3] - win[:, 2] >= 1)      # int(30 / 360 * 24) == 2
  p, count, area = ref.get_proportion_invalid_for_depth([0, .5, 0], np.zeros((2, 24), F32))
  assert math.isnan(p) and count == 0 and area == 0


@pytest.mark.parametrize('shape', [(64, 128), (6, 12), (37, 75), (100, 200), (2, 24), (512, 1024)])
def test_collision_windows_match_restatement(shape):
  h, w = shape
  offs = np.concatenate([ref.seeded_offsets(), ref.special_offsets()])
  win, dist = pu.collision_windows(offs, h, w)
  for c, off in enumerate(offs):
    want, thr, info = ref.window_and_threshold(off, h, w)
    assert tuple(int(v) for v in win[c]) == want, (c, off)
    assert dist[c] == info['distance'] and F32(dist[c] + F32(0.1)) == thr
  assert np.all((0 <= win[:, 0]) & (win[:, 0] <= win[:, 1]) & (win[:, 1] <= h))
  assert np.all((0 <= win[:, 2]) & (win[:, 2] <= win[:, 3]) & (win[:, 3] <= w))
  # clipped at the border, never wrapped: a window is narrower than 2 * threshold only at an edge
  tw = int(30 / 360 * w)
  narrow = (win[:, 3] - win[:, 2]) < 2 * tw
  assert np.all((win[narrow, 2] == 0) | (win[narrow, 3] == w))


def test_signs_of_zero():
  """[0, d, 0]: negating +0.0 gives atan2(-0., -d) = -pi, mapped to +pi by the `< 0` branch;
  a -0.0 in the offset gives +pi at once.  Both land on column start width / 2."""
  for zero in (F32(0.0), F32(-0.0)):
    _, _, info = ref.window_and_threshold(np.array([zero, 0.5, 0.0], F32), H, W)
    assert info['heading'] == F32(math.pi) and info['heading_start'] == W // 2
  # z = +0.0 -> atan2(0, -0.) = pi (row start H); z = -0.0 -> atan2(0, +0.) = 0 (row start 0)
  win, _ = pu.collision_windows(np.array([[0, 0, 0.0], [0, 0, -0.0]], F32), H, W)
  assert win[0, :2].tolist() == [H - 21, H] and win[1, :2].tolist() == [0, 21]


def test_modulo_terms_are_inert():
  """:42-43 / :51-52: `x + c * cast(x <= 0) % c` adds (c * 1) % c == 0 or (c * 0) % c == 0."""
  offs = np.concatenate([ref.seeded_offsets(200, seed=3), ref.special_offsets()])
  seen_nonpositive = 0
  for off in offs:
    _, _, info = ref.window_and_threshold(off, H, W)
    assert info['term_h'] == 0 and info['term_e'] == 0
    seen_nonpositive += int(np.arctan2(-off[0], -off[1]) <= 0)
  assert seen_nonpositive > 50   # the `<= 0` side of the cast was exercised
  two_pi, pi = F32(2 * math.pi), F32(math.pi)
  assert (two_pi * F32(1)) % two_pi == 0 and (pi * F32(1)) % pi == 0
  # so a negative heading is fixed by the `if` alone: the windows equal those of a plain wrap
  win, _ = pu.collision_windows(offs, H, W)
  hd = np.arctan2(-offs[:, 0], -offs[:, 1])
  hd = np.where(hd < 0, hd + two_pi, hd)
  start = np.trunc(hd / two_pi * F32(W)).astype(np.int64)
  assert np.array_equal(win[:, 2], np.maximum(0, start - 10))


def test_collision_windows_input_forms_and_errors():
  import torch
  offs = ref.seeded_offsets(5)
  a = pu.collision_windows(offs, H, W)
  b = pu.collision_windows(torch.from_numpy(offs), H, W)
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
  with pytest.raises(ValueError):
    pu.collision_windows(np.zeros((3,), F32), H, W)
  with pytest.raises(ValueError):
    pu.collision_windows(np.array([[np.nan, 0, 0]], F32), H, W)


def test_candidate_stream_is_reproducible():
  a = pu.draw_candidates(np.random.default_rng(1), 64)
  b = pu.draw_candidates(np.random.default_rng(1), 64)
  c = pu.draw_candidates(np.random.default_rng(2), 64)
  assert a.dtype == F32 and a.shape == (64, 3)
  assert np.array_equal(a, b) and not np.array_equal(a, c)
  assert np.all(np.abs(a[:, :2]) <= 1.5) and np.all(np.abs(a[:, 2]) <= F32(0.1))
  assert np.abs(a[:, 0]).max() > 1.0 and np.abs(a[:, 2]).max() > 0.05
  # rounds continue one stream: two rounds of 32 are not the first 64 drawn at once, but are the
  # same two rounds every time
  r = np.random.default_rng(1)
  r1, r2 = pu.draw_candidates(r, 32), pu.draw_candidates(r, 32)
  assert np.array_equal(np.concatenate([r1, r2]), a)
  d = pu.draw_candidates(np.random.default_rng(1), 8, xy_perturb=0.25, z_perturb=0.0)
  assert np.all(np.abs(d[:, :2]) <= 0.25) and np.all(d[:, 2] == 0)


def test_device_functions_have_no_cpu_fallback():
  import torch
  from se3ds_amd import _lib
  with pytest.raises(_lib.Se3dsHipError):
    pu.get_proportion_invalid_for_depth(np.array([0, .5, 0], F32), torch.zeros((H, W)))
  with pytest.raises(_lib.Se3dsHipError):
    pu.get_proportion_invalid_batch(np.zeros((2, 3), F32), torch.zeros((H, W)))


def test_host_window_check_reports_badshape():
  """se3ds_collision_check_windows (host pointers, no device work): what the launch refuses."""
  import ctypes
  from se3ds_amd import _lib
  L = _lib.lib()
  p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  def rc(win, idx, n=2):
    win = np.array(win, np.int32).reshape(-1, 4)
    idx = None if idx is None else np.array(idx, np.int32)
    return L.se3ds_collision_check_windows(p(win), None if idx is None else p(idx), n, H, W,
                                           win.shape[0])
  assert rc([[0, H, 0, W], [5, 5, 7, 7]], [0, 1]) == 0          # full and empty windows
  assert rc([[0, H, 0, W]], None) == 0
  assert rc([[0, H + 1, 0, W]], [0]) == -1
  assert rc([[-1, H, 0, W]], [0]) == -1
  assert rc([[0, H, 0, W + 1]], [0]) == -1
  assert rc([[0, H, -1, W]], [0]) == -1
  assert rc([[9, 8, 0, W]], [0]) == -1                          # row0 > row1
  assert rc([[0, H, 9, 8]], [0]) == -1
  assert rc([[0, H, 0, W]], [2]) == -1 and rc([[0, H, 0, W]], [-1]) == -1
