"""se3ds_amd.utils.utils on an MI355X (csrc/semantic.hip).  Every comparison is exact equality.

Inpaint: the yardstick is the pairwise definition of tests/_semantic_ref.py (all pairs, int64
distances, first minimum in row-major order), on every case in full: no case is skipped or sampled
and each stays below R.PAIR_CAP pairs.  Source pixels carry 1 + y W + x as int32, so a filled value
names the source that was chosen and a wrong tie shows; the index plane is compared as well.  The
shapes are the smallest that cross each boundary of the kernels: the row pass's segment and the
column pass's tile are read from the library.  uint8 images, which move four pixels per lane, have
a sweep of their own over widths and base alignments.

Sums: inputs on a lattice (p, t multiples of 2^-6, s of 2^-4 in [0, 1]) make every product a multiple
of 2^-16 and every partial sum of fewer than 2^24 terms exact in binary64, so the order of the
device's reduction cannot matter and the float64 NumPy sums, rounded to float32 where the kernel
rounds, have one legal bit pattern; the float32 tail follows in the documented order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _semantic_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import utils as U

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHARES = (0.02, 0.5, 0.97)
CLASSES = 41


def _segment():
  return _lib.lib().se3ds_nn_inpaint_row_segment()


def _tile_rows():
  return _lib.lib().se3ds_nn_inpaint_col_tile_rows()


def _chunk():
  return _lib.lib().se3ds_seq_sums_chunk()


def _shapes():
  s, t = _segment(), _tile_rows()
  return [(1, 1), (1, 9), (7, 5), (13, 17), (16, 33), (3, 63), (3, 64), (3, 65), (2, s - 1), (2, s), (2, s + 1),
          (3, 2 * s + 5), (t + 1, 70)]


def _named(h, w):
  """int32 (h, w): every pixel carries 1 + y W + x."""
  return (1 + np.arange(h * w, dtype=np.int32)).reshape(h, w)


def _holes(h, w, share, seed):
  """int32 image of named pixels, a `share` of them void (0), seeded."""
  rng = np.random.default_rng(seed)
  return np.where(rng.random((h, w)) < share, 0, _named(h, w)).astype(np.int32)


def _run(image, void_class=0):
  out, idx = U.nearest_neighbor_inpaint(torch.from_numpy(image).to(DEV), void_class, return_indices=True)
  assert out.dtype == torch.from_numpy(image).dtype and idx.dtype == torch.int32
  assert out.shape == image.shape and idx.shape == image.shape and out.is_cuda and idx.is_cuda
  return out.cpu().numpy(), idx.cpu().numpy()


def _same_bits(got, want, what):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, what
  if got.tobytes() != want.tobytes():
    view = np.uint8 if got.dtype.itemsize == 1 else np.uint32
    bad = np.argwhere(got.view(view) != want.view(view))
    first = tuple(int(v) for v in bad[0])
    raise AssertionError(f'{what}: {len(bad)} of {got.size} differ, first at {first}: got {got[first]!r} '
                         f'expected {want[first]!r}')


def _check(image, void_class=0, what=''):
  """One call on the (N, H, W) batch against the definition: values and indices."""
  want, want_idx = R.inpaint(image, void_class)
  got, got_idx = _run(image, void_class)
  _same_bits(got_idx, want_idx, f'{what} indices')
  _same_bits(got, want, f'{what} values')
  return got, got_idx


@pytest.mark.parametrize('shape_index', range(13))
def test_inpaint_shapes_and_void_shares(shape_index):
  """N = 3: the three void shares as three different patterns of one call."""
  h, w = _shapes()[shape_index]
  image = np.stack([_holes(h, w, share, 100 * shape_index + k) for k, share in enumerate(SHARES)])
  _check(image, 0, f'{h} x {w}')


def _u8_shapes():
  """uint8 images move four pixels per lane, as a dword where the row's address allows: widths around
  4 and around 4 x 64 pixels of one wavefront, odd widths (every row aligned differently), more rows
  than one tile."""
  return [(1, 1), (2, 3), (3, 4), (7, 5), (5, 8), (13, 17), (3, 255), (3, 256), (6, 257), (2, 260), (5, 515)]


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
@pytest.mark.parametrize('shape_index', range(11))
def test_inpaint_uint8_shapes_and_alignments(shape_index, offset):
  """The uint8 path at every byte offset of the image's base; values 1..255 cannot name a source, the
  index plane does."""
  h, w = _u8_shapes()[shape_index]
  named = (1 + _named(h, w) % 255).astype(np.uint8)
  rng = np.random.default_rng(300 + shape_index)
  image = np.stack([np.where(rng.random((h, w)) < share, 0, named).astype(np.uint8) for share in SHARES])
  want, want_idx = R.inpaint(image, 0)
  flat = torch.zeros((image.size + offset,), dtype=torch.uint8, device=DEV)
  flat[offset:] = torch.from_numpy(image).to(DEV).reshape(-1)
  view = flat[offset:].view(image.shape)
  assert view.data_ptr() % 4 == offset
  out, idx = U.nearest_neighbor_inpaint(view, 0, return_indices=True)
  _same_bits(idx.cpu().numpy(), want_idx, f'{h} x {w} + {offset} indices')
  _same_bits(out.cpu().numpy(), want, f'{h} x {w} + {offset} values')
  assert torch.equal(U.nearest_neighbor_inpaint(view, 0), out)           # without the index plane


def test_inpaint_batch_with_an_empty_and_a_full_image():
  h, w = 13, 17
  image = np.stack([_holes(h, w, 0.5, 1), np.zeros((h, w), np.int32), _named(h, w)])
  got, idx = _check(image, 0, 'batch')
  assert np.all(idx[1] == -1) and np.array_equal(got[1], image[1])            # all void: unchanged
  assert np.array_equal(idx[2], np.arange(h * w).reshape(h, w)) and np.array_equal(got[2], image[2])
  out = U.nearest_neighbor_inpaint(torch.from_numpy(image).to(DEV))            # without the index plane
  assert isinstance(out, torch.Tensor) and np.array_equal(out.cpu().numpy(), got)


def _ring_states(h, w, cy, cx):
  points, states = list(R.RING), []
  for winner in R.RING + [None]:
    states.append(R.ring_image(h, w, cy, cx, points))
    if winner is not None:
      points.remove(winner)
  return np.stack(states)


@pytest.mark.parametrize('place', ['bare', 'offset_2_67', 'across_a_wave', 'across_a_segment'])
def test_inpaint_tie_ring(place):
  """Twelve lattice points at squared distance 25 from the centre; the winner is removed and the
  next one must win, in the stated order.  The thirteen states are one batched call.  The embedded
  rings put the left / right tie across a wavefront's 64 columns and across a row segment."""
  seg = _segment()
  h, w, cy, cx = {'bare': (11, 11, 5, 5), 'offset_2_67': (20, 140, 7, 72), 'across_a_wave': (20, 140, 7, 64),
                  'across_a_segment': (12, seg + 40, 6, seg)}[place]
  states = _ring_states(h, w, cy, cx)
  got, idx = _check(states, 0, 'ring')
  for k, (dy, dx) in enumerate(R.RING):
    flat = (cy + dy) * w + cx + dx
    assert idx[k, cy, cx] == flat and got[k, cy, cx] == 1 + flat, (k, dy, dx)
  assert np.all(idx[12] == -1)


def test_inpaint_sparse_and_far():
  """One site in each corner in turn (one batch), then 8 seeded sites in 512 x 1024: the long outward
  scan, the early exit and distances near the top of what the shapes allow."""
  h, w = 128, 300
  corners = np.zeros((4, h, w), np.int32)
  for k, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
    corners[k, y, x] = 1 + y * w + x
  got, idx = _check(corners, 0, 'corners')
  assert np.all(got[3] == h * w)
  h, w = 512, 1024
  rng = np.random.default_rng(5)
  image = np.zeros((1, h, w), np.int32)
  flat = rng.choice(h * w, 8, replace=False)
  image.reshape(-1)[flat] = 1 + flat
  _check(image, 0, '8 sites')


def test_inpaint_rows_without_sites():
  h, w = 16, 33
  every_second = _holes(h, w, 0.5, 3)
  every_second[::2] = 0
  one_row = np.zeros((h, w), np.int32)
  one_row[11] = _named(h, w)[11]
  one_column = np.zeros((h, w), np.int32)
  one_column[:, 20] = _named(h, w)[:, 20]
  _check(np.stack([every_second, one_row, one_column]), 0, 'rows without sites')


def test_inpaint_dtypes_and_void_values():
  h, w = 13, 17
  rng = np.random.default_rng(9)
  u8 = rng.integers(0, 255, (2, h, w)).astype(np.uint8)
  u8[rng.random((2, h, w)) < 0.5] = 255
  u8[0, 0, 0] = 0                                   # 0 is a value like any other here
  _check(u8, 255, 'uint8 / 255')
  f32 = _named(h, w).astype(np.float32)[None].repeat(2, 0)
  f32[rng.random((2, h, w)) < 0.5] = -1.0
  _check(f32, -1.0, 'float32 / -1.0')
  # a 0.0 void class: -0.0 is void too, a NaN is not and is copied into its neighbours bit for bit
  z = _named(h, w).astype(np.float32)[None].repeat(2, 0)
  hole = rng.random((2, h, w)) < 0.6
  z[hole] = np.where(rng.random(int(hole.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
  nan = np.array([0x7fc00123, 0xffc00001, 0x7fe00055], np.uint32).view(np.float32)
  sites = np.argwhere(~hole)
  for k, at in enumerate(sites[rng.choice(len(sites), 9, replace=False)]):
    z[tuple(at)] = nan[k % 3]
  want, want_idx = R.inpaint(z, 0.0)
  assert np.isnan(want).sum() > 9, 'no NaN was copied: the case checks nothing'
  got, got_idx = _run(z, 0.0)
  _same_bits(got_idx, want_idx, 'float32 / 0.0 indices')
  _same_bits(got.view(np.int32), want.view(np.int32), 'float32 / 0.0 values')
  assert not np.any((got == 0) & (want_idx >= 0))


def test_inpaint_views_with_a_storage_offset():
  h, w = 7, 5
  big = np.stack([_holes(h, w, 0.5, k) for k in range(4)])
  t = torch.from_numpy(big).to(DEV)
  want, want_idx = R.inpaint(big[1:], 0)
  out, idx = U.nearest_neighbor_inpaint(t[1:], 0, return_indices=True)
  _same_bits(out.cpu().numpy(), want, 'slice values')
  _same_bits(idx.cpu().numpy(), want_idx, 'slice indices')
  # uint8 at an odd byte offset
  rng = np.random.default_rng(2)
  u8 = rng.integers(1, 200, (3, 9, 13)).astype(np.uint8)
  u8[rng.random(u8.shape) < 0.5] = 0
  flat = torch.zeros((u8.size + 1,), dtype=torch.uint8, device=DEV)
  flat[1:] = torch.from_numpy(u8).to(DEV).reshape(-1)
  view = flat[1:].view(3, 9, 13)
  assert view.data_ptr() % 2 == 1 and view.is_contiguous()
  want, want_idx = R.inpaint(u8, 0)
  out, idx = U.nearest_neighbor_inpaint(view, 0, return_indices=True)
  _same_bits(out.cpu().numpy(), want, 'odd offset values')
  _same_bits(idx.cpu().numpy(), want_idx, 'odd offset indices')
  out2 = U.nearest_neighbor_inpaint(view.clone(), 0)
  assert torch.equal(out, out2)


def test_inpaint_index_plane_is_consistent():
  image = np.stack([_holes(16, 33, 0.5, 21), _holes(16, 33, 0.97, 22), np.zeros((16, 33), np.int32)])
  t = torch.from_numpy(image).to(DEV)
  out, idx = U.nearest_neighbor_inpaint(t, 0, return_indices=True)
  out, idx = out.cpu().numpy(), idx.cpu().numpy()
  for n in range(3):
    o, i, src = out[n].reshape(-1), idx[n].reshape(-1), image[n].reshape(-1)
    ok = i >= 0
    assert np.array_equal(o[ok], src[i[ok]]) and np.array_equal(o[~ok], src[~ok])
    assert np.all(src[i[ok]] != 0)
  assert np.all(idx[2] == -1) and (idx[:2] >= 0).all()
  # the plane fills a second plane with the same neighbours
  depth = np.random.default_rng(4).random((16, 33)).astype(np.float32)
  assert np.array_equal(depth.reshape(-1)[idx[0].reshape(-1)].reshape(16, 33)[image[0] != 0], depth[image[0] != 0])


def test_inpaint_refuses_what_it_cannot_do():
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    U.nearest_neighbor_inpaint(torch.zeros((1, 0, 4), dtype=torch.int32, device=DEV))
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    U.nearest_neighbor_inpaint(torch.zeros((1, 1, 16385), dtype=torch.uint8, device=DEV))


# ---------------------------------------------------------------------------------------------
# sums

IOU_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 3), (1, 2, 9, 7, 41), (2, 5, 16, 16, 42), (1, 8, 33, 65, 5)]


def _lattice(shape, seed, steps):
  """float32 multiples of 1 / steps in [0, 1], both ends included."""
  a = np.random.default_rng(seed).integers(0, steps + 1, shape).astype(np.float32) / np.float32(steps)
  a.reshape(-1)[:2] = (0.0, 1.0)[:a.size]
  return a


def _masks(n, t, seed):
  mixed = (np.random.default_rng(seed).random((n, t)) < 0.6).astype(np.float32)
  return {'ones': np.ones((n, t), np.float32), 'zeros': np.zeros((n, t), np.float32), 'mixed': mixed}


def _dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pair(result):
  seq, mean = result
  assert seq.dtype == torch.float32 and mean.dtype == torch.float32 and mean.dim() == 0
  return seq.cpu().numpy(), mean.cpu().numpy()


def _same_metric(got, want, what):
  _same_bits(got[0], want[0], f'{what} seq')
  _same_bits(got[1].reshape(()), np.asarray(want[1], np.float32).reshape(()), f'{what} mean')


def _iou_shapes():
  c = _chunk()
  return IOU_SHAPES + [(1, 2, 1, c - 1, 1), (1, 2, 1, c, 1), (1, 3, 1, c + 1, 1), (1, 2, 1, (2 * c + 3) // 3 + 1, 3)]


@pytest.mark.parametrize('shape_index', range(9))
def test_sequence_iou_on_the_lattice(shape_index):
  shape = _iou_shapes()[shape_index]
  n, t, h, w, c = shape
  assert h * w * c < 1 << 24
  p, q = _lattice(shape, 10 + shape_index, 64), _lattice(shape, 50 + shape_index, 64)
  q = np.where(np.random.default_rng(shape_index).random(shape) < 0.3, p, q)
  s = _lattice((n, t, h, w), 90 + shape_index, 16)
  pd, qd, sd = _dev(p), _dev(q), _dev(s)
  for spatial, spatial_dev in ((None, None), (s, sd)):
    i, ss = R.iou_sums(p, q, spatial)
    for name, mask in _masks(n, t, shape_index).items():
      want = R.tail(i, ss, mask)
      got = _pair(U.compute_sequence_iou(pd, qd, _dev(mask), spatial_dev))
      assert got[0].shape == (n, t) and np.all(got[0] >= 0)
      _same_metric(got, want, f'{shape} {name} spatial={spatial is not None}')
      if name == 'zeros':
        assert np.all(got[0] == 0) and got[1] == 0


def test_sequence_iou_operands_of_different_alignment():
  """pred one float behind a 16-byte boundary, true on it: the chunk takes the scalar path; both one
  float behind: a head of three and a tail."""
  shape = (2, 3, 9, 7, 5)
  count = int(np.prod(shape))
  p, q = _lattice(shape, 1, 64), _lattice(shape, 2, 64)
  mask = np.ones(shape[:2], np.float32)
  want = R.sequence_iou(p, q, mask)
  buf_p = torch.zeros((count + 1,), device=DEV)
  buf_q = torch.zeros((count + 1,), device=DEV)
  buf_p[1:] = _dev(p).reshape(-1)
  buf_q[1:] = _dev(q).reshape(-1)
  odd_p, odd_q = buf_p[1:].view(shape), buf_q[1:].view(shape)
  assert odd_p.data_ptr() % 16 == 4
  _same_metric(_pair(U.compute_sequence_iou(odd_p, _dev(q), _dev(mask))), want, 'one operand off')
  _same_metric(_pair(U.compute_sequence_iou(odd_p, odd_q, _dev(mask))), want, 'both operands off')


def test_sequence_metrics_properties():
  """What the reference's own test asks for, with a mask that is not always zero."""
  shape = (2, 5, 16, 16, 42)
  rng = np.random.default_rng(3)
  labels = rng.integers(0, 42, shape[:4])
  hot = _dev(R.one_hot(labels, 42))
  other = _dev(R.one_hot(rng.integers(0, 42, shape[:4]), 42))
  ones, zeros = torch.ones((2, 5), device=DEV), torch.zeros((2, 5), device=DEV)
  seq, mean = _pair(U.compute_sequence_iou(hot, other, ones))
  assert seq.shape == (2, 5) and np.all(seq >= 0) and np.all(seq <= 1) and 0 <= mean <= 1
  seq, mean = _pair(U.compute_sequence_iou(hot, other, zeros))
  assert np.all(seq == 0) and mean.tobytes() == np.float32(0).tobytes()
  seq, mean = _pair(U.compute_sequence_iou(hot, hot, ones))
  assert np.all(seq == 1) and mean == 1
  lab = _dev(labels.astype(np.int32))
  for fn in (U.compute_sequence_accuracy, U.sequence_iou_from_labels):
    seq, mean = _pair(fn(lab, lab, ones))
    assert seq.shape == (2, 5) and np.all(seq == 1) and mean == 1
  seq, mean = _pair(U.sequence_iou_from_labels(lab, lab, zeros))
  assert np.all(seq == 0) and mean == 0
  # the accuracy of a frame does not look at the sequence mask; the mean does (reference, :167-175)
  seq, mean = _pair(U.compute_sequence_accuracy(lab, lab, zeros))
  assert np.all(seq == 1) and mean == 0


def _label_shapes():
  c = _chunk()
  shapes = [s[:4] for s in IOU_SHAPES] + [(1, 2, 1, hw) for hw in (1, 63, 64, 65, 1023, 1025)]
  return shapes + [(1, 2, 1, c - 1), (1, 2, 1, c), (1, 3, 1, c + 1), (1, 2, 3, (2 * c + 17) // 3)]


@pytest.mark.parametrize('dtype', [np.uint8, np.int32], ids=['uint8', 'int32'])
@pytest.mark.parametrize('shape_index', range(15))
def test_label_metrics(shape_index, dtype):
  shape = _label_shapes()[shape_index]
  n, t, h, w = shape
  rng = np.random.default_rng(200 + shape_index)
  pred = rng.integers(0, CLASSES, shape).astype(dtype)
  gt = np.where(rng.random(shape) < 0.5, pred, rng.integers(0, CLASSES, shape)).astype(dtype)
  spatials = {'none': None, 'bool': rng.random(shape) < 0.6, 'uint8': (rng.random(shape) < 0.6).astype(np.uint8),
              'int32': rng.integers(0, 3, shape).astype(np.int32), 'float32': _lattice(shape, shape_index, 16)}
  pd, gd = _dev(pred), _dev(gt)
  for sname, spatial in spatials.items():
    i, s = R.label_sums(pred, gt, spatial)
    for mname, mask in _masks(n, t, shape_index).items():
      what = f'{shape} {sname} {mname}'
      got = _pair(U.compute_sequence_accuracy(pd, gd, _dev(mask), _dev(spatial)))
      assert got[0].shape == (n, t) and np.all(got[0] >= 0)
      _same_metric(got, R.tail(i, s, mask, accuracy=True), 'accuracy ' + what)
      got = _pair(U.sequence_iou_from_labels(pd, gd, _dev(mask), _dev(spatial)))
      _same_metric(got, R.tail(i, 2.0 * s, mask), 'label IoU ' + what)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32], ids=['uint8', 'int32'])
def test_label_iou_equals_the_one_hot_route(dtype):
  shape = (2, 3, 16, 16)
  gen = torch.Generator().manual_seed(8)
  pred = torch.randint(0, CLASSES, shape, generator=gen)
  gt = torch.where(torch.rand(shape, generator=gen) < 0.5, pred, torch.randint(0, CLASSES, shape, generator=gen))
  hot_p = F.one_hot(pred, CLASSES).float().to(DEV)
  hot_g = F.one_hot(gt, CLASSES).float().to(DEV)
  mask = _dev(_masks(2, 3, 1)['mixed'])
  mask[0, 0] = 1
  for spatial in (None, _dev(_lattice(shape, 6, 16))):
    a = _pair(U.sequence_iou_from_labels(pred.to(DEV, dtype), gt.to(DEV, dtype), mask, spatial))
    b = _pair(U.compute_sequence_iou(hot_p, hot_g, mask, spatial))
    _same_metric(a, b, f'labels against one-hot, spatial={spatial is not None}')
    assert a[1] > 0


def test_sums_are_the_same_on_every_run():
  shape = (2, 5, 16, 16, 42)
  gen = torch.Generator().manual_seed(12)
  p = torch.rand(shape, generator=gen).to(DEV)
  q = torch.rand(shape, generator=gen).to(DEV)
  s = torch.rand(shape[:4], generator=gen).to(DEV)
  mask = torch.ones((2, 5), device=DEV)
  first = _pair(U.compute_sequence_iou(p, q, mask, s))
  second = _pair(U.compute_sequence_iou(p, q, mask, s))
  _same_metric(first, second, 'second run')
  lab = torch.randint(0, CLASSES, shape[:4], generator=gen).to(DEV, torch.int32)
  first = _pair(U.compute_sequence_accuracy(lab, lab.roll(1, 3), mask, s))
  second = _pair(U.compute_sequence_accuracy(lab, lab.roll(1, 3), mask, s))
  _same_metric(first, second, 'second run, labels')


# ---------------------------------------------------------------------------------------------
# colours

@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32], ids=['uint8', 'int32'])
def test_colours_round_trip(dtype):
  cmap = U.create_label_colormap()
  rng = np.random.default_rng(6)
  for labels in (rng.integers(0, 256, (3, 5, 7)), np.arange(256).reshape(1, 1, 256)):
    lab = torch.from_numpy(labels).to(DEV, dtype)
    colour = U.label_to_color(lab, cmap)
    assert colour.dtype == torch.uint8 and colour.shape == labels.shape + (3,)
    assert np.array_equal(colour.cpu().numpy(), cmap[labels].astype(np.uint8))
    for image in (colour, colour.to(torch.int32)):
      back = U.cmap_to_label(image, cmap)
      assert back.dtype == torch.int32 and back.shape == labels.shape
      assert np.array_equal(back.cpu().numpy(), labels)
  # a cmap that is a device tensor
  back = U.cmap_to_label(colour, torch.from_numpy(cmap).to(DEV))
  assert np.array_equal(back.cpu().numpy(), labels)


@pytest.mark.parametrize('pixels', [1, 63, 64, 65, 341])
def test_colours_pixel_counts_and_maps(pixels):
  cmap = U.create_label_colormap()
  rng = np.random.default_rng(pixels)
  image = cmap[rng.integers(0, 256, pixels)].astype(np.uint8)
  image[rng.random(pixels) < 0.2] = (1, 2, 3)                      # a colour the map does not hold
  for k in (1, 5, 256):
    want = R.cmap_to_label(image, cmap[:k])
    got = U.cmap_to_label(_dev(image), cmap[:k])
    assert got.shape == (pixels,) and np.array_equal(got.cpu().numpy(), want), k
    got = U.cmap_to_label(_dev(image.astype(np.int32)), cmap[:k])
    assert np.array_equal(got.cpu().numpy(), want), k
  # a duplicated colour gives the first index; an int32 pixel outside 0..255 matches nothing
  dup = cmap[:8].copy()
  dup[6] = dup[2]
  dup[7] = dup[0]
  img = dup[rng.integers(0, 8, pixels)]
  want = R.cmap_to_label(img, dup)
  assert not np.isin(want, (6, 7)).any()
  assert np.array_equal(U.cmap_to_label(_dev(img.astype(np.uint8)), dup).cpu().numpy(), want)
  wild = img.astype(np.int32)
  wild[::2, 1] += 256
  assert np.array_equal(U.cmap_to_label(_dev(wild), dup).cpu().numpy(), R.cmap_to_label(wild, dup))
  # labels outside the map become black
  lab = rng.integers(0, 12, pixels).astype(np.int32)
  lab[0] = -1
  want = np.where(((lab >= 0) & (lab < 8))[:, None], dup[np.clip(lab, 0, 7)], 0).astype(np.uint8)
  assert np.array_equal(U.label_to_color(_dev(lab), dup).cpu().numpy(), want)
