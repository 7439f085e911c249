"""NumPy restatement of the evaluation input transform (test infrastructure, not product code):
what the reference's R2RVideoDataset._transform_fn (datasets/indoor_datasets.py:734-792) computes
for one batch, written from its behaviour -- tf.image.resize (bilinear for the RGB frames, nearest
for the label and depth planes, half-pixel centres, no antialias, no clip) and the band mask on the
output grid -- with every fp32 operation rounded on its own."""
import numpy as np

from oracle.warp_np import _resize_bilinear, _resize_nearest

F32 = np.float32
PLANES = ('segmentation', 'pathdreamer_segmentation', 'depth', 'pathdreamer_depth')
PASS_THROUGH = ('id', 'mask', 'depth_scale', 'dataset_type')


def band_mask(width, hmask):
  """(width,) fp32 of 0 / 1: None keeps everything, mode 1 keeps start < x < end, mode 2 (the
  band wraps around the seam) keeps x > start or x < end; x is the fp32 column index."""
  if hmask is None:
    return np.ones((width,), F32)
  mode, start, end = hmask
  x = np.arange(width, dtype=F32)
  if mode == 1:
    keep = np.logical_and(x > F32(start), x < F32(end))
  elif mode == 2:
    keep = np.logical_or(x > F32(start), x < F32(end))
  else:
    raise ValueError(mode)
  return keep.astype(F32)


def video_transform(raw, params, image_size):
  """raw: dict of NumPy arrays as `_parse` yields them, batched: image fp32 (N,T,H0,W0,3), planes
  (N,T,H0,W0), position (N,T,4), ...  params: one dict(hmask=None | (mode, start, end)) per
  example.  Returns the output dict of the transform as NumPy arrays."""
  image = np.asarray(raw['image'])
  assert image.dtype == F32
  n, t, h0, w0, _ = image.shape
  h, w = image_size, 2 * image_size
  original = _resize_bilinear(image.reshape(n * t, h0, w0, 3), h, w).reshape(n, t, h, w, 3)
  out = dict(original_image=original)
  if all(p.get('hmask') is None for p in params):
    out['image'] = original
  else:
    mask = np.stack([band_mask(w, p.get('hmask')) for p in params])   # (N, w)
    out['image'] = (original * mask[:, None, None, :, None]).astype(F32)
  for k in PLANES:
    if k in raw:
      v = np.asarray(raw[k])
      out[k] = _resize_nearest(v.reshape(n * t, h0, w0, 1), h, w).reshape(n, t, h, w, 1)
  out['position'] = np.ascontiguousarray(np.asarray(raw['position'])[..., :3])
  out['position_xyz1'] = np.asarray(raw['position'])
  for k in PASS_THROUGH:
    if k in raw:
      out[k] = np.asarray(raw[k])
  return out


def synth_examples(count, t, h0, seed, pathdreamer=True, lo=0.0, hi=1.0):
  """`count` per-example dicts shaped like `_parse` results (T frames of h0 x 2*h0)."""
  rng = np.random.default_rng(seed)
  w0 = 2 * h0
  out = []
  for i in range(count):
    ex = dict(
        id=np.int64(100 + i), dataset_type=np.int64(0),
        image=rng.uniform(lo, hi, (t, h0, w0, 3)).astype(F32),
        position=np.concatenate([(rng.standard_normal((t, 3)) * 0.3).astype(F32),
                                 np.ones((t, 1), F32)], axis=1),
        mask=np.ones((t,), F32),
        segmentation=rng.integers(0, 42, (t, h0, w0)).astype(np.uint8),
        depth=rng.uniform(0.05, 0.95, (t, h0, w0)).astype(F32),
        depth_scale=F32(20.0))
    if pathdreamer:
      ex['pathdreamer_segmentation'] = rng.integers(0, 42, (t, h0, w0)).astype(np.uint8)
      ex['pathdreamer_depth'] = rng.uniform(0.05, 0.95, (t, h0, w0)).astype(F32)
    out.append(ex)
  return out


def decode_png(data):
  """Decodes an 8-bit, non-interlaced grey / RGB PNG whose rows all use filter 0 (what the project's
  writer emits) with zlib by hand: (H,W,C) uint8."""
  import struct
  import zlib
  assert data[:8] == b'\x89PNG\r\n\x1a\n'
  pos, idat, hdr = 8, b'', None
  while pos < len(data):
    length, = struct.unpack('>I', data[pos:pos + 4])
    tag = data[pos + 4:pos + 8]
    body = data[pos + 8:pos + 8 + length]
    crc, = struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])
    assert crc == zlib.crc32(tag + body), tag
    if tag == b'IHDR':
      hdr = struct.unpack('>IIBBBBB', body)
    elif tag == b'IDAT':
      idat += body
    pos += 12 + length
  assert tag == b'IEND'
  w, h, depth, colour, comp, filt, interlace = hdr
  assert depth == 8 and colour in (0, 2) and (comp, filt, interlace) == (0, 0, 0)
  c = 1 if colour == 0 else 3
  rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * c)
  assert not rows[:, 0].any()
  return rows[:, 1:].reshape(h, w, c).copy()
