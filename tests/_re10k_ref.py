"""NumPy restatement of what the reference computes for an RE10K training record: the `_parse`
branch (datasets/indoor_datasets.py:232-240), `_transform_fn_re10k` (:377-535) and the batch
transform (:577-585), with the random draws passed in.  fp32 throughout, one rounding per operation,
left to right.  Test infrastructure: the kernels are compared with this, bit for bit."""
import numpy as np

from oracle import input_np, warp_np

F32 = np.float32
OK, BLANK, OUTSIDE = 0, 1, 2


def extents(visible):
  """(r0, r1, c0, c1): first / last row and column of a (H,W) plane holding a visible pixel;
  (H, -1, W, -1) when there is none."""
  h, w = visible.shape
  rows = np.flatnonzero((visible > 0).any(axis=1))
  cols = np.flatnonzero((visible > 0).any(axis=0))
  if rows.size == 0:
    return h, -1, w, -1
  return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def box(r0, r1, c0, c1, height, width, pad, x_shift, y_shift):
  """:445-472 -> ([x_min, y_min, x_max, y_max], status).  Without a visible pixel (r1 < r0) the
  reference fails at :445; the numbers are then those of the same arithmetic on (H, -1, W, -1)."""
  pad, x_shift, y_shift = F32(pad), F32(x_shift), F32(y_shift)
  fh, fw = F32(height), F32(width)
  y_min = F32(F32(F32(r0) / fh) - pad) + y_shift
  y_max = F32(F32(F32(r1) / fh) + pad) + y_shift
  x_min = F32(F32(c0) / fw)
  x_max = F32(F32(c1) / fw)
  new_h = F32(y_max - y_min)
  pad_w = F32(F32(new_h - F32(x_max - x_min)) / F32(2))
  x_max = F32(F32(x_max + pad_w) + x_shift)
  x_min = F32(F32(x_min - pad_w) + x_shift)
  iy0, ix0 = int(np.trunc(F32(y_min * fh))), int(np.trunc(F32(x_min * fw)))
  iy1, ix1 = int(np.trunc(F32(y_max * fh))), int(np.trunc(F32(x_max * fw)))
  iy0, ix0 = max(0, iy0), max(0, ix0)
  iy1, ix1 = min(iy1, height), min(ix1, width)
  iy1, ix1 = max(iy0 + 1, iy1), max(ix0 + 1, ix1)
  status = BLANK if (r1 < r0 or c1 < c0) else OUTSIDE if (iy1 > height or ix1 > width) else OK
  return [ix0, iy0, ix1, iy1], status


def convert_frames(raw):
  """:185-240: the base conversions, then blurred_mask = 1 - clip(visible_mask, 0, 1)."""
  f = input_np.convert_frames(dict(raw, blurred_mask=raw['visible_mask']))
  f['blurred_mask'] = (F32(1) - f['blurred_mask']).astype(F32)
  return f


def transform_example(f, visible, prm, image_size, crop):
  """`_transform_fn_re10k` on one converted example `f` (H0,W0[,C]) with the draws `prm` (hmask,
  vmask, pad, x_shift, y_shift) -> (planes, bbox or None, status).  crop = re_10k_crop and
  random_crop; without it the planes keep their size (:474)."""
  h0, w0 = f['proj_mask'].shape
  proj_mask = f['proj_mask'][..., None]
  if prm.get('hmask') is not None:
    mode, start, end = prm['hmask']
    r = np.arange(w0, dtype=F32)
    m = ((r > F32(start)) | (r < F32(end))) if mode == 2 else ((r > F32(start)) & (r < F32(end)))
    proj_mask = proj_mask * m[None, :, None].astype(F32)
  if prm.get('vmask') is not None:
    start, end = prm['vmask']
    r = np.arange(h0, dtype=F32)
    m = (r > F32(start)) & (r < F32(end))
    proj_mask = proj_mask * m[:, None, None].astype(F32)
  images = f['image']
  semantics = np.concatenate([f['segmentation'][..., None].astype(F32), f['depth'][..., None],
                              f['proj_depth'][..., None], proj_mask, f['blurred_mask'][..., None]],
                             axis=-1)
  proj_image = f['proj_image']
  bbox, status = None, OK
  if crop:
    bbox, status = box(*extents(visible), h0, w0, prm['pad'], prm['x_shift'], prm['y_shift'])
    if status != OK:
      return None, bbox, status
    x0, y0, x1, y1 = bbox
    s = image_size
    cut = lambda a: a[None, y0:y1, x0:x1]
    images = np.clip(warp_np._resize_bilinear(cut(images), s, 2 * s)[0], 0.0, 1.0).astype(F32)
    semantics = warp_np._resize_nearest(cut(semantics), s, 2 * s)[0]
    proj_image = warp_np._resize_nearest(cut(proj_image), s, 2 * s)[0]
  out = dict(image=images, segmentation=semantics[..., 0:1].astype(np.int32),
             depth=semantics[..., 1:2], proj_depth=semantics[..., 2:3], proj_mask=semantics[..., 3:4],
             blurred_mask=semantics[..., 4:5], proj_image=proj_image)
  return out, bbox, status


def transform_batch(raw, params, image_size, crop):
  """Per-example transform and `_train_batch_transform_fn`: -> (list of per-example plane dicts, None
  for an example with a nonzero status; boxes; statuses)."""
  f = convert_frames(raw)
  outs, boxes, statuses = [], [], []
  for i, prm in enumerate(params):
    o, b, st = transform_example({k: v[i] for k, v in f.items()}, raw['visible_mask'][i], prm,
                                 image_size, crop)
    if o is not None:
      o['proj_image'] = (o['proj_image'] * o['proj_mask']).astype(F32)
      o['proj_depth'] = (o['proj_depth'] * o['proj_mask']).astype(F32)
    outs.append(o)
    boxes.append(b)
    statuses.append(st)
  return outs, boxes, statuses
