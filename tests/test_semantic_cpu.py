"""se3ds_amd.utils.utils without a GPU: csrc/nn_inpaint_core.h as a stand-alone host program
(tools/nn_inpaint_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, the host
colour map, the argument checks of the wrappers and of the entry points (all of which run before any
HIP call) and the oracles of tests/_semantic_ref.py against themselves.  The device runs are
tests/test_semantic_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _semantic_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADSHAPE, BADDTYPE, WORKSPACE = -1, -2, -3


def test_core_as_a_sanitised_host_program(tmp_path):
  """Both passes, serially, with the functions the kernels call, against the pairwise definition
  written in the program; every buffer is an exact-size heap allocation.  Reports are fatal.  No
  sanitizer touches code loaded into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the inpaint core cannot be checked on the host'
  exe = str(tmp_path / 'nn_inpaint_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'nn_inpaint_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  m = re.search(r'nn_inpaint_host_check: (\d+) cases OK', r.stdout)
  # 13 shapes x 3 pixel kinds x 6 patterns, and 13 ring states per kind
  assert m and int(m.group(1)) == 13 * 3 * 6 + 3 * 13
  # the checker does fail when it should: one table entry flipped between the passes
  r = subprocess.run([exe, 'corrupt'], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected' in r.stderr


def test_constants_of_the_core_and_the_library_agree():
  text = open(os.path.join(ROOT, 'se3ds_amd', 'csrc', 'nn_inpaint_core.h')).read()
  L = _lib.lib()
  assert L.se3ds_nn_inpaint_row_segment() == int(re.search(r'constexpr int kRowSegment = (\d+);', text).group(1))
  assert L.se3ds_nn_inpaint_col_tile_rows() == int(re.search(r'constexpr int kColTileRows = (\d+);', text).group(1))
  assert int(re.search(r'constexpr int kMaxSide = (\d+);', text).group(1)) == U.MAX_SIDE == 16384
  assert L.se3ds_seq_sums_chunk() % 1024 == 0


def test_label_colormap():
  cmap = U.create_label_colormap()
  assert isinstance(cmap, np.ndarray) and cmap.shape == (256, 3) and cmap.dtype == np.dtype(int)
  assert cmap[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]]
  assert cmap[255].tolist() == [224, 224, 192]
  assert len({tuple(row) for row in cmap.tolist()}) == 256
  assert cmap.min() >= 0 and cmap.max() <= 255
  assert np.array_equal(cmap, R.label_colormap())
  # the oracle of the inverse on the host: every colour maps back to its label, others to 0
  assert np.array_equal(R.cmap_to_label(cmap.reshape(16, 16, 3), cmap), np.arange(256).reshape(16, 16))
  assert R.cmap_to_label(np.array([[1, 2, 3]]), cmap).tolist() == [0]


def test_inpaint_workspace_query():
  L = _lib.lib()
  q = L.se3ds_nn_inpaint_workspace_bytes
  for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 16385, 4), (1, 4, 16385), (-1, 4, 4)):
    assert q(*bad) == 0, bad
  last = 0
  for shape in ((1, 1, 1), (1, 1, 9), (1, 7, 5), (2, 7, 5), (3, 13, 17), (3, 16, 33), (3, 512, 1024),
                (8, 1024, 2048), (8, 16384, 16384)):
    b = q(*shape)
    assert b % 16 == 0 and b >= 2 * shape[0] * shape[1] * shape[2] and b >= last, shape
    last = b
  s = L.se3ds_seq_sums_workspace_bytes
  assert s(0, 5) == 0 and s(5, 0) == 0 and s(1, 2 ** 31) == 0
  chunk = L.se3ds_seq_sums_chunk()
  assert s(1, 1) == 16 and s(3, chunk) == 48 and s(3, chunk + 1) == 96
  assert all(s(f, e) % 16 == 0 for f in (1, 2, 7) for e in (1, 105, 2583, 10752, 22020096))


def test_entry_points_check_their_arguments_before_the_device():
  """Every refusal returns before the first HIP call, so it shows without a GPU: the pointers only
  have to be non-null and aligned, nothing follows them."""
  L = _lib.lib()
  mem = (ctypes.c_uint8 * 1024)()
  p = (ctypes.addressof(mem) + 15) & ~15   # 16-byte aligned, 1008 bytes behind it
  big = 1 << 40

  def inpaint(dtype=_lib.I32, n=1, h=4, w=4, image=p, out=p + 64, indices=None, ws=p + 128, ws_bytes=big, phases=3):
    return L.se3ds_nn_inpaint(image, dtype, 0, n, h, w, out, indices, ws, ws_bytes, phases, None)

  for kw in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385), dict(n=0), dict(n=65536), dict(h=-1)):
    assert inpaint(**kw) == BADSHAPE, kw
  assert inpaint(dtype=_lib.BF16) == BADDTYPE and inpaint(dtype=7) == BADDTYPE
  for kw in (dict(image=None), dict(out=None), dict(ws=None), dict(phases=0), dict(phases=4),
             dict(image=p + 2), dict(out=p + 1), dict(indices=p + 2), dict(ws=p + 8)):
    assert inpaint(**kw) == BADSHAPE, kw
  assert inpaint(ws_bytes=31) == WORKSPACE and inpaint(n=2, h=16384, w=16384, ws_bytes=2 ** 30 - 1) == WORKSPACE

  def iou(frames=2, pixels=16, channels=3, pred=p, truth=p, spatial=None, sums=p, ws=p, ws_bytes=big):
    return L.se3ds_seq_iou_sums(pred, truth, spatial, frames, pixels, channels, sums, ws, ws_bytes, None)

  for kw in (dict(frames=0), dict(pixels=0), dict(channels=0), dict(pixels=2 ** 30, channels=2), dict(pred=None),
             dict(truth=None), dict(sums=None), dict(ws=None), dict(pred=p + 2), dict(spatial=p + 1),
             dict(sums=p + 4)):
    assert iou(**kw) == BADSHAPE, kw
  assert iou(ws_bytes=16) == WORKSPACE

  def match(label=_lib.U8, spatial=None, spatial_dtype=-1, frames=2, pixels=16, pred=p, gt=p, sums=p, ws=p,
            ws_bytes=big):
    return L.se3ds_seq_label_match(pred, gt, label, spatial, spatial_dtype, frames, pixels, sums, ws, ws_bytes, None)

  assert match(label=_lib.F32) == BADDTYPE and match(label=_lib.BF16) == BADDTYPE
  assert match(spatial=p, spatial_dtype=_lib.BF16) == BADDTYPE and match(spatial=p, spatial_dtype=-1) == BADDTYPE
  for kw in (dict(frames=0), dict(pixels=0), dict(pixels=2 ** 31), dict(pred=None), dict(gt=None),
             dict(label=_lib.I32, gt=p + 2), dict(spatial=p + 2, spatial_dtype=_lib.F32), dict(ws=p + 4)):
    assert match(**kw) == BADSHAPE, kw
  assert match(ws_bytes=0) == WORKSPACE

  assert L.se3ds_seq_finalize(p, p, 0, 3, 0, p, p, None) == BADSHAPE
  assert L.se3ds_seq_finalize(p, p, 2, 0, 0, p, p, None) == BADSHAPE
  assert L.se3ds_seq_finalize(p, p, 2, 3, 3, p, p, None) == BADSHAPE
  assert L.se3ds_seq_finalize(None, p, 2, 3, 0, p, p, None) == BADSHAPE
  for fn in (L.se3ds_cmap_to_label, L.se3ds_label_to_color):
    assert fn(p, _lib.U8, 10, p, 257, p, None) == BADSHAPE       # K > 256
    assert fn(p, _lib.U8, 10, p, 0, p, None) == BADSHAPE
    assert fn(p, _lib.U8, 0, p, 5, p, None) == BADSHAPE
    assert fn(p, _lib.F32, 10, p, 5, p, None) == BADDTYPE
    assert fn(None, _lib.U8, 10, p, 5, p, None) == BADSHAPE


def test_wrappers_check_shapes_and_dtypes_first():
  z = torch.zeros
  with pytest.raises(ValueError, match='N, H, W'):
    U.nearest_neighbor_inpaint(z((4, 4), dtype=torch.int32))
  for dtype in (torch.int64, torch.float16, torch.bfloat16, torch.float64, torch.bool):
    with pytest.raises(ValueError, match='dtype'):
      U.nearest_neighbor_inpaint(z((1, 4, 4), dtype=dtype))
  for void, dtype in ((256, torch.uint8), (-1, torch.uint8), (0.5, torch.int32), (2 ** 31, torch.int32)):
    with pytest.raises(ValueError, match='void_class'):
      U.nearest_neighbor_inpaint(z((1, 4, 4), dtype=dtype), void)
  with pytest.raises(ValueError):
    U.nearest_neighbor_inpaint(np.zeros((1, 4, 4), np.int32))

  p5, m = z((2, 3, 4, 5, 6)), torch.ones((2, 3))
  for pred, true, mask, spatial in ((p5, z((2, 3, 4, 5, 7)), m, None), (p5, p5[0], m, None),
                                    (p5, p5, torch.ones((3, 2)), None), (p5, p5, torch.ones((2,)), None),
                                    (p5, p5, m, z((2, 3, 4, 6))), (p5, p5, m, z((2, 3, 4, 5, 6))),
                                    (p5, p5, m, z((2, 3, 4, 5), dtype=torch.uint8)),
                                    (p5.double(), p5.double(), m, None), (p5, p5.to(torch.int32), m, None)):
    with pytest.raises(ValueError):
      U.compute_sequence_iou(pred, true, mask, spatial)

  l4 = z((2, 3, 4, 5), dtype=torch.int32)
  for fn in (U.compute_sequence_accuracy, U.sequence_iou_from_labels):
    for pred, gt, mask, spatial in ((l4, z((2, 3, 4, 6), dtype=torch.int32), m, None), (l4, l4[0], m, None),
                                    (l4, l4.to(torch.uint8), m, None), (l4.float(), l4.float(), m, None),
                                    (l4.long(), l4.long(), m, None), (l4, l4, torch.ones((2, 4)), None),
                                    (l4, l4, m, z((2, 3, 5, 4))), (l4, l4, m, z((2, 3, 4, 5), dtype=torch.float64))):
      with pytest.raises(ValueError):
        fn(pred, gt, mask, spatial)

  img = z((4, 4, 3), dtype=torch.uint8)
  with pytest.raises(ValueError, match='K'):
    U.cmap_to_label(img, np.zeros((257, 3), np.int64))
  with pytest.raises(ValueError, match='K'):
    U.label_to_color(img[..., 0], torch.zeros((257, 3), dtype=torch.int32))
  with pytest.raises(ValueError):
    U.cmap_to_label(img, np.zeros((0, 3), np.int64))
  with pytest.raises(ValueError):
    U.cmap_to_label(img, np.zeros((4, 4), np.int64))
  with pytest.raises(ValueError):
    U.cmap_to_label(img, np.zeros((4, 3), np.float32))
  with pytest.raises(ValueError):
    U.cmap_to_label(z((4, 4, 4), dtype=torch.uint8), U.create_label_colormap())
  with pytest.raises(ValueError):
    U.cmap_to_label(img.float(), U.create_label_colormap())
  with pytest.raises(ValueError):
    U.label_to_color(img[..., 0].long(), U.create_label_colormap())


def test_no_cpu_fallback():
  z, cmap = torch.zeros, U.create_label_colormap()
  m = torch.ones((1, 2))
  for dtype in (torch.uint8, torch.int32, torch.float32):
    with pytest.raises(_lib.Se3dsHipError):
      U.nearest_neighbor_inpaint(z((1, 4, 4), dtype=dtype))
  with pytest.raises(_lib.Se3dsHipError):
    U.nearest_neighbor_inpaint(z((1, 4, 4), dtype=torch.int32), return_indices=True)
  with pytest.raises(_lib.Se3dsHipError):
    U.compute_sequence_iou(z((1, 2, 3, 3, 4)), z((1, 2, 3, 3, 4)), m)
  with pytest.raises(_lib.Se3dsHipError):
    U.compute_sequence_iou(z((1, 2, 3, 3, 4)), z((1, 2, 3, 3, 4)), m, torch.ones((1, 2, 3, 3)))
  for fn in (U.compute_sequence_accuracy, U.sequence_iou_from_labels):
    for dtype in (torch.uint8, torch.int32):
      with pytest.raises(_lib.Se3dsHipError):
        fn(z((1, 2, 3, 3), dtype=dtype), z((1, 2, 3, 3), dtype=dtype), m)
    with pytest.raises(_lib.Se3dsHipError):
      fn(z((1, 2, 3, 3), dtype=torch.uint8), z((1, 2, 3, 3), dtype=torch.uint8), m,
         torch.ones((1, 2, 3, 3), dtype=torch.bool))
  with pytest.raises(_lib.Se3dsHipError):
    U.cmap_to_label(z((4, 4, 3), dtype=torch.uint8), cmap)
  with pytest.raises(_lib.Se3dsHipError):
    U.label_to_color(z((4, 4), dtype=torch.int32), cmap)


def test_reference_names_and_argument_order():
  import inspect
  want = {'nearest_neighbor_inpaint': ['image', 'void_class'],
          'compute_sequence_iou': ['one_hot_pred', 'one_hot_true', 'mask', 'spatial_mask'],
          'compute_sequence_accuracy': ['class_pred', 'class_gt', 'mask', 'spatial_mask'],
          'create_label_colormap': [], 'cmap_to_label': ['image', 'cmap']}
  for name, args in want.items():
    got = list(inspect.signature(getattr(U, name)).parameters)
    assert got[:len(args)] == args, (name, got)
  sig = inspect.signature(U.nearest_neighbor_inpaint)
  assert sig.parameters['void_class'].default == 0 and sig.parameters['return_indices'].default is False
  assert inspect.signature(U.compute_sequence_iou).parameters['spatial_mask'].default is None


def test_oracle_tie_ring():
  """The pairwise definition picks the ring's points in the stated order, the centre included."""
  points = list(R.RING)
  for want in R.RING:
    image = R.ring_image(points=points)
    filled, index = R.inpaint_one(image, 0)
    y, x = 5 + want[0], 5 + want[1]
    assert index[5, 5] == y * 11 + x and filled[5, 5] == 1 + y * 11 + x, want
    points.remove(want)
  filled, index = R.inpaint_one(R.ring_image(points=[]), 0)
  assert np.all(index == -1) and np.all(filled == 0)
  # a hand-checked row: ties go left
  filled, index = R.inpaint_one(np.array([[7, 0, 0, 0, 9, 0]], np.int32), 0)
  assert filled.tolist() == [[7, 7, 7, 9, 9, 9]] and index.tolist() == [[0, 0, 0, 4, 4, 4]]
  # floats: -0.0 is void with a 0.0 void class, NaN is not
  image = np.array([[-0.0, np.nan, 0.0]], np.float32)
  filled, index = R.inpaint_one(image, 0.0)
  assert index.tolist() == [[1, 1, 1]] and np.isnan(filled).all()


def test_oracle_label_iou_equals_one_hot_iou():
  rng = np.random.default_rng(11)
  for seed, shape in enumerate(((1, 1, 1, 1), (2, 3, 5, 7), (2, 3, 16, 16))):
    pred = rng.integers(0, 41, shape)
    gt = np.where(rng.random(shape) < 0.5, pred, rng.integers(0, 41, shape))
    mask = (rng.random(shape[:2]) < 0.7).astype(np.float32)
    for spatial in (None, (rng.random(shape) < 0.6), rng.integers(0, 17, shape) / 16.0):
      a_seq, a_mean = R.sequence_iou_from_labels(pred, gt, mask, spatial)
      sp = None if spatial is None else np.asarray(spatial, np.float32)
      b_seq, b_mean = R.sequence_iou(R.one_hot(pred, 41), R.one_hot(gt, 41), mask, sp)
      assert a_seq.tobytes() == b_seq.tobytes() and a_mean.tobytes() == b_mean.tobytes(), (shape, seed)
  # identical maps and a ones mask give exactly 1; a zero mask exactly 0
  seq, mean = R.sequence_iou_from_labels(pred, pred, np.ones(shape[:2], np.float32))
  assert np.all(seq == 1) and mean == 1
  seq, mean = R.sequence_iou_from_labels(pred, gt, np.zeros(shape[:2], np.float32))
  assert np.all(seq == 0) and mean == 0
