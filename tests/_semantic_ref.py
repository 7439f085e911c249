"""NumPy restatements of the reference's utils/utils.py, the yardsticks of tests/test_semantic_*.py.
Nothing here looks at the code under test.

Inpaint: the definition.  Every (site, void pixel) pair, int64 squared distances, argmin along the
site axis with the sites in the row-major order np.nonzero lists them, so the first minimum wins:
the smallest row, within it the smallest column.  Void pixels are taken in chunks to bound the memory.

Sums: float64 NumPy, rounded to float32 where the kernel rounds (I and S), followed by the float32
tail in the stated order: t = 0..T-1, then n = 0..N-1."""
import numpy as np

PAIR_CAP = 3 * 10 ** 7   # (sites) x (void pixels) of one inpaint case
_CHUNK_PAIRS = 1 << 22


def inpaint_one(image, void_class):
  """image (H, W) -> (filled (H, W), source index (H, W) int32; own index for a site, -1 when the
  image has no site)."""
  h, w = image.shape
  hole = image == np.asarray(void_class, dtype=image.dtype)
  sy, sx = np.nonzero(~hole)          # row-major
  vy, vx = np.nonzero(hole)
  index = np.arange(h * w, dtype=np.int32).reshape(h, w).copy()
  if sy.size == 0:
    index[...] = -1
    return image.copy(), index
  assert sy.size * vy.size <= PAIR_CAP, f'{sy.size} x {vy.size} pairs exceed the cap'
  sy64, sx64 = sy.astype(np.int64)[:, None], sx.astype(np.int64)[:, None]
  step = max(1, _CHUNK_PAIRS // sy.size)
  for k in range(0, vy.size, step):
    y, x = vy[k:k + step], vx[k:k + step]
    dist = (sy64 - y[None, :].astype(np.int64)) ** 2 + (sx64 - x[None, :].astype(np.int64)) ** 2
    arg = np.argmin(dist, axis=0)
    index[y, x] = (sy[arg] * w + sx[arg]).astype(np.int32)
  filled = image.reshape(-1)[np.maximum(index, 0).reshape(-1)].reshape(h, w)
  filled = np.where(index < 0, image, filled)
  return filled, index


def inpaint(image, void_class):
  """(N, H, W) -> (filled, indices)."""
  both = [inpaint_one(im, void_class) for im in image]
  return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def label_colormap():
  """Bit 7 - j of channel c of label i is bit 3 j + c of i, written label by label."""
  cmap = np.zeros((256, 3), dtype=np.int64)
  for i in range(256):
    for c in range(3):
      v = 0
      for j in range(8):
        v |= ((i >> (3 * j + c)) & 1) << (7 - j)
      cmap[i, c] = v
  return cmap


def cmap_to_label(image, cmap):
  equal = np.all(np.asarray(image)[..., None, :] == np.asarray(cmap), axis=-1)
  return np.argmax(equal, axis=-1)


def _dnn(x, y):
  return np.float32(0) if y == 0 else np.float32(np.float32(x) / np.float32(y))


def tail(i64, s64, mask, accuracy=False):
  """I, S float64 (N, T) -> (seq (N, T) float32, mean float32): the float32 tail in index order."""
  i32, s32 = np.asarray(i64, np.float64).astype(np.float32), np.asarray(s64, np.float64).astype(np.float32)
  mask = np.asarray(mask, dtype=np.float32)
  n, t = mask.shape
  seq = np.zeros((n, t), np.float32)
  total = np.float32(0)
  for b in range(n):
    acc, length = np.float32(0), np.float32(0)
    for k in range(t):
      if accuracy:
        v = _dnn(i32[b, k], s32[b, k])
      else:
        u = np.float32(s32[b, k] - i32[b, k])
        v = _dnn(np.float32(i32[b, k] * mask[b, k]), np.float32(u * mask[b, k]))
      seq[b, k] = v
      acc = np.float32(acc + v)
      length = np.float32(length + mask[b, k])
    total = np.float32(total + _dnn(acc, length))
  return seq, np.float32(total / np.float32(n))


def iou_sums(pred, true, spatial=None):
  """(N, T, H, W, C) float32 -> float64 I, S (N, T)."""
  p, t = np.asarray(pred, np.float64), np.asarray(true, np.float64)
  s = 1.0 if spatial is None else np.asarray(spatial, np.float64)[..., None]
  return (p * t * s).sum(axis=(2, 3, 4)), ((p + t) * s).sum(axis=(2, 3, 4))


def sequence_iou(pred, true, mask, spatial=None):
  i, s = iou_sums(pred, true, spatial)
  return tail(i, s, mask)


def label_sums(pred, gt, spatial=None):
  """(N, T, H, W) labels -> float64 sum [pred == gt] s, sum s (N, T)."""
  eq = (np.asarray(pred) == np.asarray(gt)).astype(np.float64)
  s = np.ones(eq.shape) if spatial is None else np.asarray(spatial).astype(np.float64)
  return (eq * s).sum(axis=(2, 3)), s.sum(axis=(2, 3))


def sequence_accuracy(pred, gt, mask, spatial=None):
  i, s = label_sums(pred, gt, spatial)
  return tail(i, s, mask, accuracy=True)


def sequence_iou_from_labels(pred, gt, mask, spatial=None):
  i, s = label_sums(pred, gt, spatial)
  return tail(i, 2.0 * s, mask)


def one_hot(labels, classes):
  return (np.asarray(labels)[..., None] == np.arange(classes)).astype(np.float32)


RING = [(-5, 0), (-4, -3), (-4, 3), (-3, -4), (-3, 4), (0, -5), (0, 5), (3, -4), (3, 4), (4, -3), (4, 3), (5, 0)]


def ring_image(h=11, w=11, cy=5, cx=5, points=RING):
  """int32 image, void (0) everywhere except the ring's points, which carry 1 + y W + x."""
  image = np.zeros((h, w), np.int32)
  for dy, dx in points:
    image[cy + dy, cx + dx] = 1 + (cy + dy) * w + cx + dx
  return image
