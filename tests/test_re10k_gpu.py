"""RE10KImageDataset on the device: se3ds_re10k_extent and se3ds_re10k_transform bit for bit against
the NumPy restatement tests/_re10k_ref.py -- every load path of the reduction, masks mixed within a
batch, every clamp of the box, the status words, the four modes, the C ABI's refusals, and records
read end to end.  Every comparison is exact equality."""
import ctypes

import numpy as np
import pytest
import torch

import _png_ref
import _re10k_ref
from _records import image_record
from se3ds_amd import _lib
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.utils import tf_records

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32 = np.float32
PLANES = ('image', 'proj_image', 'proj_mask', 'proj_depth', 'depth', 'blurred_mask', 'segmentation')
PADS = (-0.05, 0.0, 0.1)
SIGNS = ((-1, -1), (-1, 1), (1, -1), (1, 1))   # shifts at +-0.5 |pad|: the box leaves on each side


def _masks(h, kind, rng):
  """Batches of five masks at (h, 2h); the kinds are mixed within a batch."""
  w = 2 * h
  z = lambda: np.zeros((h, w), np.uint8)
  out = []
  if kind == 'pixels':   # one visible pixel: the four corners and the centre
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
      m = z()
      m[y, x] = 255
      out.append(m)
  else:
    out.append(np.full((h, w), 1, np.uint8))                       # everything visible
    m = z(); m[:h // 2 + 1, w // 3:] = 255; out.append(m)          # touches the top and the right edge
    m = z(); m[h // 3:, :w // 2 + 1] = 2; out.append(m)            # the bottom and the left edge
    m = z()                                                        # two separate blobs
    m[h // 8:h // 4 + 1, w // 8:w // 4 + 1] = 255
    m[h // 2:3 * h // 4 + 1, 5 * w // 8:7 * w // 8] = 1
    out.append(m)
    m = z()                                                        # visible values 1, 2 and 255
    m[h // 4:3 * h // 4, w // 4:3 * w // 4] = rng.choice(np.array([0, 1, 2, 255], np.uint8),
                                                         (3 * h // 4 - h // 4, 3 * w // 4 - w // 4))
    m[h // 4, w // 4] = m[3 * h // 4 - 1, 3 * w // 4 - 1] = 2
    out.append(m)
  return np.stack(out)


def _raw(rng, masks):
  n, h, w = masks.shape
  return dict(image=rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8),
              proj_image=rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8),
              depth=rng.integers(0, 65536, (n, h, w)).astype(np.uint16),
              proj_depth=rng.integers(0, 65536, (n, h, w)).astype(np.uint16),
              proj_mask=rng.integers(0, 2, (n, h, w), dtype=np.uint8) * np.uint8(255),
              visible_mask=masks,
              segmentation=rng.integers(0, 42, (n, h, w), dtype=np.uint8))


def _upload(raw):
  return {k: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)
          for k, a in raw.items()}


def _draw(idx, h, w):
  """Row `idx` of the sweep pad x shift signs x band masks (12 rows cover pad x signs)."""
  pad = F32(PADS[idx % 3])
  sx, sy = SIGNS[(idx // 3) % 4]
  half = F32(0.5) * np.abs(pad)
  hmask = (None, (1, float(F32(0.3 * w)), float(F32(0.8 * w))),
           (2, float(F32(0.7 * w)), float(F32(0.2 * w))))[(idx // 2) % 3]
  vmask = (float(F32(0.1 * h)), float(F32(0.85 * h))) if idx % 4 < 2 else None
  return dict(hmask=hmask, vmask=vmask, pad=float(pad), x_shift=float(F32(sx) * half),
              y_shift=float(F32(sy) * half))


def _extents(masks):
  n, h, w = masks.shape
  ext = torch.from_numpy(np.tile(np.array([h, -1, w, -1], np.int32), (n, 1))).to(DEV)
  m = torch.from_numpy(masks).to(DEV)
  _lib.check(_lib.lib().se3ds_re10k_extent(_lib.ptr(m), n, h, w, _lib.ptr(ext), _lib.stream()),
             'se3ds_re10k_extent')
  return ext.cpu().numpy()


def _compare(ds, raw, params, crop, bbox=None):
  """One launch against the restatement, example by example; -> the statuses."""
  want, boxes, statuses = _re10k_ref.transform_batch(raw, params, ds.image_size, crop)
  got, pending = ds._launch(_upload(raw), params, bbox)
  assert pending.wait().tolist() == statuses
  host = {k: v.cpu().numpy() for k, v in got.items()}
  for i, w in enumerate(want):
    for k in PLANES:
      g = host[k][i]
      if w is None:
        assert not g.any(), (i, k)
      else:
        assert g.dtype == w[k].dtype and g.shape == w[k].shape, (i, k, g.shape, w[k].shape)
        assert np.array_equal(g, w[k]), (i, k)
    if crop:
      assert host['bbox'][i].tolist() == boxes[i], i
  return statuses


@pytest.mark.parametrize('h0,size', [(8, 4), (20, 4), (72, 8)])
def test_parity_over_masks_and_draws(h0, size):
  """W0 = 16: one 16-byte lane; 40: the byte path; 144: nine lanes.  Two batches of five mixed
  masks, twelve draw rows each, rotated through the examples."""
  rng = np.random.default_rng(h0)
  ds = indoor_datasets.RE10KImageDataset(image_size=size, preprocessed_image_height=h0,
                                         re_10k_crop=True)
  assert _lib.lib().se3ds_re10k_extent_vector_bytes(None, 2 * h0) == (16 if h0 % 8 == 0 else 1)
  seen = []
  for kind in ('pixels', 'areas'):
    masks = _masks(h0, kind, rng)
    assert _extents(masks).tolist() == [list(_re10k_ref.extents(m)) for m in masks]
    raw = _raw(rng, masks)
    for k in range(12):
      seen += _compare(ds, raw, [_draw(k + i, h0, 2 * h0) for i in range(5)], True)
  # the sweep is about crops that can be made; the corner pixels with a negative pad cannot
  assert seen.count(0) > 90 and 1 not in seen


def test_rounding_rows_and_columns():
  """H0 = 100 (byte path), pad = shifts = 0, extents on the rows and columns where
  trunc((i / n) * n) = i - 1 in fp32."""
  rng = np.random.default_rng(100)
  corners = [(53, 53), (59, 59), (53, 105), (59, 106), (53, 117)]
  masks = np.zeros((5, 100, 200), np.uint8)
  for m, (r, c) in zip(masks, corners):
    m[r:90, c:190] = 255
  masks[4, 53:90, 118:190] = 1
  assert _extents(masks).tolist() == [[r, 89, c, 189] for r, c in corners]
  ds = indoor_datasets.RE10KImageDataset(image_size=8, preprocessed_image_height=100,
                                         re_10k_crop=True)
  prm = dict(hmask=None, vmask=None, pad=0.0, x_shift=0.0, y_shift=0.0)
  assert _compare(ds, _raw(rng, masks), [prm] * 5, True) == [0] * 5
  got = ds.device_transform(_upload(_raw(rng, masks)), [prm] * 5)['bbox'].cpu().numpy()
  assert got[:, 1].tolist() == [52, 58, 52, 58, 52]


def test_large_frame_rows_over_workgroups():
  """1024 x 2048, N = 1: two 16-byte loads per lane per row, the rows spread over 32 workgroups."""
  rng = np.random.default_rng(1024)
  masks = np.zeros((1, 1024, 2048), np.uint8)
  masks[0, 301:777, 1100:1931] = rng.integers(0, 2, (476, 831), dtype=np.uint8)
  masks[0, 301, 1500] = masks[0, 776, 1200] = masks[0, 500, 1100] = masks[0, 600, 1930] = 7
  masks[0, 17, 1029] = 1   # alone in its band and in the second segment of its row
  assert _extents(masks).tolist() == [[17, 776, 1029, 1930]]
  masks[0, 17, 1029] = 0
  assert _extents(masks).tolist() == [[301, 776, 1100, 1930]]
  ds = indoor_datasets.RE10KImageDataset(image_size=8, preprocessed_image_height=1024,
                                         re_10k_crop=True)
  assert _compare(ds, _raw(rng, masks), [_draw(5, 1024, 2048)], True) == [0]


def test_one_pixel_crop_resized_up():
  """A negative pad on a one-pixel extent: the box collapses and the `+ 1` fix-up makes a 1 x 1
  crop, which every output pixel then reads."""
  rng = np.random.default_rng(9)
  masks = np.zeros((1, 20, 40), np.uint8)
  masks[0, 9, 17] = 3
  raw = _raw(rng, masks)
  raw['proj_mask'][:] = 255
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=20,
                                         re_10k_crop=True)
  prm = dict(hmask=None, vmask=None, pad=-0.05, x_shift=0.02, y_shift=0.02)
  assert _compare(ds, raw, [prm], True) == [0]
  out = ds.device_transform(_upload(raw), [prm])
  assert out['bbox'].tolist() == [[19, 10, 20, 11]]
  px = torch.from_numpy((raw['image'][0, 10, 19].astype(F32) * F32(1.0 / 255.0))).to(DEV)
  assert torch.equal(out['image'][0], px.expand(4, 8, 3))
  assert out['segmentation'].unique().tolist() == [int(raw['segmentation'][0, 10, 19])]


@pytest.mark.parametrize('re_10k_crop', [False, True])
@pytest.mark.parametrize('random_crop', [False, True])
def test_the_four_modes(re_10k_crop, random_crop):
  rng = np.random.default_rng(4)
  raw = _raw(rng, _masks(20, 'areas', rng))
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=20,
                                         re_10k_crop=re_10k_crop, random_crop=random_crop)
  crop = re_10k_crop and random_crop
  draw = np.random.default_rng(8)
  params = [ds.draw_params(draw, 20, 40) for _ in range(5)]
  assert all((p['pad'] is not None) == re_10k_crop for p in params)
  record_bbox = rng.random((5, 4), dtype=F32)
  _compare(ds, raw, params, crop, record_bbox)
  out = ds.device_transform(_upload(raw), params, record_bbox)
  hw = (4, 8) if crop else (20, 40)
  for k in PLANES:
    assert tuple(out[k].shape) == (5,) + hw + ((3,) if 'image' in k else (1,)), k
  if crop:
    assert out['bbox'].dtype == torch.int32 and tuple(out['bbox'].shape) == (5, 4)
    b = out['bbox'].cpu().numpy()
    assert (b[:, 0] < b[:, 2]).all() and (b[:, 1] < b[:, 3]).all() and b.min() >= 0
  else:
    assert out['bbox'].dtype == torch.float32 and out['bbox'].is_cuda
    assert np.array_equal(out['bbox'].cpu().numpy(), record_bbox)
    with pytest.raises(ValueError, match='bbox'):
      ds.device_transform(_upload(raw), params)
  # transform() draws what draw_params draws
  again = ds.transform(_upload(raw), np.random.default_rng(8), record_bbox)
  assert all(torch.equal(again[k], out[k]) for k in out)


def test_status_words():
  rng = np.random.default_rng(6)
  masks = _masks(20, 'areas', rng)[:4]
  masks[1] = 0                      # blank: status 1
  masks[2] = 0
  masks[2, 19, 5:31] = 255          # the only visible row is 19; pad = -0.05: y_min = 20, y_max = 21
  raw = _raw(rng, masks)
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=20,
                                         re_10k_crop=True)
  prm = dict(hmask=(1, 3.5, 30.25), vmask=None, pad=-0.05, x_shift=0.0, y_shift=0.0)
  # the other examples of the batch equal the restatement, the refused ones are zeros
  assert _compare(ds, raw, [prm] * 4, True) == [0, 1, 2, 0]
  with pytest.raises(ValueError, match='example 1 of the batch: visible_mask has no visible pixel'):
    ds.device_transform(_upload(raw), [prm] * 4)
  with pytest.raises(ValueError, match='example 1 '):
    ds.transform(_upload(raw), np.random.default_rng(0))
  raw2 = {k: v[[0, 3, 2]] for k, v in raw.items()}
  with pytest.raises(ValueError, match='example 2 of the batch: the crop box does not lie inside'):
    ds.device_transform(_upload(raw2), [prm] * 3)
  # without the crop nothing looks at the mask's extents
  plain = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=20)
  assert _compare(plain, raw, [prm] * 4, False, np.zeros((4, 4), F32)) == [0] * 4


def test_c_abi_refuses_bad_shapes_and_nulls():
  L = _lib.lib()
  n, h0, w0, h, w = 2, 8, 16, 4, 8
  u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
  i16 = lambda *s: torch.zeros(s, dtype=torch.int16, device=DEV)
  f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
  i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)
  keep = dict(image=u8(n, h0, w0, 3), proj_image=u8(n, h0, w0, 3), depth=i16(n, h0, w0),
              proj_depth=i16(n, h0, w0), proj_mask=u8(n, h0, w0), visible=u8(n, h0, w0) + 1,
              seg=u8(n, h0, w0), ext=i32(n, 4), ip=i32(n, 3), fp=f32(n, 7), o_image=f32(n, h, w, 3),
              o_proj_image=f32(n, h, w, 3), o_proj_mask=f32(n, h, w), o_proj_depth=f32(n, h, w),
              o_depth=f32(n, h, w), o_blurred=f32(n, h, w), o_seg=i32(n, h, w), o_bbox=i32(n, 4),
              o_status=i32(n))
  order = ['image', 'proj_image', 'depth', 'proj_depth', 'proj_mask', 'visible', 'seg', 'ext', 'ip',
           'fp', 'n', 'h0', 'w0', 'h', 'w', 'o_image', 'o_proj_image', 'o_proj_mask', 'o_proj_depth',
           'o_depth', 'o_blurred', 'o_seg', 'o_bbox', 'o_status']

  def call(**change):
    v = dict({k: _lib.ptr(t) for k, t in keep.items()}, n=n, h0=h0, w0=w0, h=h, w=w)
    v.update(change)
    return L.se3ds_re10k_transform(*[v[k] for k in order], _lib.stream())

  keep['ext'].copy_(torch.tensor([[h0, -1, w0, -1]] * n, dtype=torch.int32))
  assert L.se3ds_re10k_extent(_lib.ptr(keep['visible']), n, h0, w0, _lib.ptr(keep['ext']),
                              _lib.stream()) == 0
  assert call() == 0
  assert call(ext=None, o_bbox=None) == 0            # no crop: they go together
  torch.cuda.synchronize()
  for bad in (dict(n=0), dict(n=-1), dict(h0=0), dict(w0=-4), dict(h=0), dict(w=-1),
              dict(ext=None), dict(o_bbox=None), dict(o_status=None), dict(image=None),
              dict(visible=None), dict(ip=None), dict(fp=None), dict(o_seg=None)):
    assert call(**bad) == -1, bad
  m, e = _lib.ptr(keep['visible']), _lib.ptr(keep['ext'])
  for args in ((m, 0, h0, w0, e), (m, n, -1, w0, e), (m, n, h0, 0, e), (None, n, h0, w0, e),
               (m, n, h0, w0, None)):
    assert L.se3ds_re10k_extent(*args, _lib.stream()) == -1, args
  assert _lib.ABI['SE3DS_E_BADSHAPE'] == -1
  # an unaligned plane takes the byte path, and finds the same extents
  flat = torch.zeros(1 + n * h0 * w0, dtype=torch.uint8, device=DEV)
  flat[1 + 3 * w0 + 5] = 1
  flat[1 + h0 * w0 + 6 * w0 + 15] = 9
  assert L.se3ds_re10k_extent_vector_bytes(flat.data_ptr() + 1, w0) == 1
  assert L.se3ds_re10k_extent_vector_bytes(flat.data_ptr(), w0) == 16
  keep['ext'].copy_(torch.tensor([[h0, -1, w0, -1]] * n, dtype=torch.int32))
  assert L.se3ds_re10k_extent(ctypes.c_void_p(flat.data_ptr() + 1), n, h0, w0, e, _lib.stream()) == 0
  assert keep['ext'].tolist() == [[3, 3, 5, 5], [6, 6, 15, 15]]


@pytest.mark.parametrize('re_10k_crop', [True, False])
def test_input_fn_end_to_end(tmp_path, re_10k_crop):
  """Three records at height 8 in one file, batches of 2 over two epochs: equal to the restatement
  fed the same seed's draws, and inflate='host' equals inflate='device'."""
  rng = np.random.default_rng(31)
  made = []
  for i in range(3):
    mask = np.zeros((8, 16), np.uint8)
    mask[1 + i % 2:6, 3:12 + i] = rng.integers(1, 256, (5 - i % 2, 9 + i), dtype=np.uint8)
    rec, pix = image_record(
        8, rng, dataset_type=np.array([2]), depth_scale=np.array([10.0 + i], np.float32),
        bbox=np.array([i, 1, 2, 3], np.float32),
        **{'image/visible_mask': _png_ref.encode_png(mask, [int(f) for f in rng.integers(0, 5, 8)]),
           'image/blurred_mask': b''})
    del pix['blurred_mask']
    made.append((rec, dict(pix, visible_mask=mask)))
  tf_records.write_records(str(tmp_path / 'train-00000.tfrecord'), [m[0] for m in made])
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=8,
                                         data_dir=str(tmp_path), re_10k_crop=re_10k_crop)
  seed, pipeline = 5, 2
  kw = dict(batch_size=2, seed=seed, input_pipeline_id=pipeline, device=DEV, num_epochs=2)
  host = list(ds.input_fn('train', **kw))
  dev = list(ds.input_fn('train', inflate='device', verify_crc='device', **kw))
  draw = np.random.default_rng(seed + pipeline)
  assert len(host) == len(dev) == 3
  for got, other, ids in zip(host, dev, ([0, 1], [2, 0], [1, 2])):
    raw = {k: np.stack([made[i][1][k] for i in ids]) for k in made[0][1]}
    params = [ds.draw_params(draw, 8, 16) for _ in ids]
    want, boxes, statuses = _re10k_ref.transform_batch(raw, params, 4, re_10k_crop)
    assert statuses == [0, 0]
    assert set(got) == set(other) == set(PLANES) | {'bbox', 'depth_scale'}
    for k in PLANES:
      assert np.array_equal(got[k].cpu().numpy(), np.stack([w[k] for w in want])), k
    if re_10k_crop:
      assert got['bbox'].dtype == torch.int32 and got['bbox'].tolist() == boxes
    else:
      assert got['bbox'].dtype == torch.float32
      assert got['bbox'].tolist() == [[float(i), 1.0, 2.0, 3.0] for i in ids]
    assert got['depth_scale'].tolist() == [10.0 + i for i in ids]
    for k in got:
      assert got[k].dtype == other[k].dtype and torch.equal(got[k], other[k]), k
  # a record without a visible pixel stops the stream when its batch's turn comes
  if re_10k_crop:
    blank, _ = image_record(8, rng, dataset_type=np.array([2]), **{
        'image/visible_mask': _png_ref.encode_png(np.zeros((8, 16), np.uint8), [0] * 8)})
    tf_records.write_records(str(tmp_path / 'val-00000.tfrecord'), [made[0][0], made[1][0], made[2][0], blank])
    for inflate in ('host', 'device'):
      it = ds.input_fn('val', batch_size=2, device=DEV, num_epochs=1, inflate=inflate)
      next(it)
      with pytest.raises(ValueError, match='example 1 of the batch'):
        next(it)
