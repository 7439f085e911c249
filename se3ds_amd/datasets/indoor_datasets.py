"""Device-side half of the reference's datasets/indoor_datasets.py: `augment`
(:34-61) and `R2RImageDataset`'s per-example transform (:263-375) + batch transform (:553-597) as
ONE gather kernel over decoded frames resident in HBM (`se3ds_input_transform`).  TFRecord / PNG
decoding, sharding, shuffling and prefetching stay outside: the caller hands over
uint8 / uint16 frames (what `tf.image.decode_png` yields, :185-228) as CUDA tensors.

Same constructor arguments and gin selectors as the reference (`R2RImageDataset.image_size`, ...).
The random draws follow the statement order of `_transform_fn` and are made on the host with a
NumPy generator (TensorFlow's RNG streams cannot be reproduced without TensorFlow); everything
downstream of the draws is bit-exact against oracle/input_np.py.

`R2RVideoDataset` is the evaluation side (:604-827): the per-example transform of the trajectory
records (`_transform_fn`, :734-792) over all N*T frames of a batch as one gather
(`se3ds_video_transform`), and an `input_fn` that batches parsed examples the way the reference's
tf.data pipeline does (repeat, then batch) and yields what `EvalMetric` consumes."""
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Union

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd import constants
from se3ds_amd import gin_lite as gin

F32 = np.float32
RAW_DTYPES = dict(image=torch.uint8, proj_image=torch.uint8, depth=torch.int16, proj_depth=torch.int16,
                  proj_mask=torch.uint8, blurred_mask=torch.uint8, segmentation=torch.uint8)


def draw_augment(rng: np.random.Generator, width: int, random_roll_range: Optional[int] = None,
                 random_flip: bool = True):
  """The draws of `augment` (:54-60): roll amount in [-range, range), flip with p = 0.5."""
  random_roll_range = random_roll_range or (width // 2)
  roll = int(rng.integers(-random_roll_range, random_roll_range))
  flip = bool(rng.uniform() < 0.5) if random_flip else False
  return roll, flip


@gin.configurable
class R2RImageDataset:
  """Preprocessing of R2R / Matterport panoramas for training (reference :64-120)."""

  def __init__(self, image_size: int = 256, preprocessed_image_height: int = 512, z_dim: int = 64,
               num_classes: int = constants.NUM_MP3D_CLASSES, data_dir: str = 'data/train/',
               return_filename: bool = False, horizontal_mask_ratio: float = 0.5,
               vertical_mask_ratio: float = 0.5, random_roll_and_flip: bool = True,
               random_crop: bool = True, random_resize_max: float = 2.0, pad_minval: float = -0.05,
               pad_maxval: float = 0.1, re_10k_crop: bool = False, **kwargs):
    del kwargs
    self.image_size = image_size
    self.preprocessed_image_height = preprocessed_image_height
    self.z_dim = z_dim
    self.num_classes = num_classes
    self.data_dir = data_dir
    self.return_filename = return_filename
    self.horizontal_mask_ratio = horizontal_mask_ratio
    self.vertical_mask_ratio = vertical_mask_ratio
    self.random_roll_and_flip = random_roll_and_flip
    self.random_crop = random_crop
    self.random_resize_max = random_resize_max
    self.pad_minval = pad_minval
    self.pad_maxval = pad_maxval
    self.re_10k_crop = re_10k_crop

  # ------------------------------------------------------------------------------ the draws
  def draw_params(self, rng: np.random.Generator, height: int, width: int) -> dict:
    """One example's random draws, in the statement order of `_transform_fn` (:272-330)."""
    s = self.image_size
    prm = dict(resize=(s, 2 * s), hmask=None, vmask=None, roll=0, flip=False, crop=(0, 0))
    if self.random_crop:
      mult = F32(rng.uniform(1.0, self.random_resize_max))
      prm['resize'] = (int(F32(s) * mult), int(F32(2 * s) * mult))
    if self.horizontal_mask_ratio > 0:
      mask_ratio = F32(rng.uniform(0, self.horizontal_mask_ratio))
      keep_ratio = F32(1) - mask_ratio
      start = F32(rng.uniform(0, width))
      end = F32(np.mod(start + F32(width) * keep_ratio, F32(width)))
      prm['hmask'] = (2 if start > end else 1, float(start), float(end))
    if self.vertical_mask_ratio > 0:
      mask_ratio = F32(rng.uniform(0, self.vertical_mask_ratio))
      image_height = F32(height) * (F32(1) - mask_ratio)
      start = F32(rng.uniform(0, max(float(F32(height) - image_height), 1e-30)))
      prm['vmask'] = (float(start), float(start + image_height))
    if self.random_roll_and_flip:
      prm['roll'], prm['flip'] = draw_augment(rng, prm['resize'][1],
                                              int(float(s) * 2 * self.random_resize_max))
    if self.random_crop:
      rh, rw = prm['resize']
      prm['crop'] = (int(rng.integers(0, rh - s + 1)), int(rng.integers(0, rw - 2 * s + 1)))
    return prm

  # ------------------------------------------------------------------------- device transform
  def device_transform(self, raw: Dict[str, torch.Tensor], params: List[dict]
                       ) -> Dict[str, torch.Tensor]:
    """raw: decoded frames on the GPU -- image / proj_image uint8 (N,H0,W0,3); depth / proj_depth
    uint16 bit patterns held as int16 (N,H0,W0); proj_mask / blurred_mask / segmentation uint8
    (N,H0,W0).  Returns the step's batch dict (image, proj_image, proj_mask, proj_depth, depth,
    blurred_mask fp32 (N,h,w,C); segmentation int32 (N,h,w,1))."""
    for k, dt in RAW_DTYPES.items():
      _lib.require_cuda(raw[k])
      if raw[k].dtype != dt:
        raise ValueError(f'{k}: expected {dt}, got {raw[k].dtype}')
    n, h0, w0 = raw['proj_mask'].shape
    if len(params) != n:
      raise ValueError(f'{len(params)} parameter rows for a batch of {n}')
    s = self.image_size
    ip = np.zeros((n, 8), np.int32)
    fp = np.zeros((n, 4), F32)
    for i, prm in enumerate(params):
      rh, rw = prm['resize']
      oy, ox = prm.get('crop', (0, 0))
      if oy < 0 or ox < 0 or oy + s > rh or ox + 2 * s > rw:
        raise ValueError(f'crop {oy, ox} of a {rh}x{rw} frame does not hold a {s}x{2 * s} panorama')
      ip[i, :6] = (rh, rw, prm.get('roll', 0), int(bool(prm.get('flip', False))), oy, ox)
      if prm.get('hmask') is not None:
        ip[i, 6], fp[i, 0], fp[i, 1] = prm['hmask']
      if prm.get('vmask') is not None:
        ip[i, 7] = 1
        fp[i, 2], fp[i, 3] = prm['vmask']
    dev = raw['proj_mask'].device
    ipd, fpd = torch.from_numpy(ip).to(dev), torch.from_numpy(fp).to(dev)
    f = lambda c: torch.empty((n, s, 2 * s, c), dtype=torch.float32, device=dev)
    out = dict(image=f(3), proj_image=f(3), proj_mask=f(1), proj_depth=f(1), depth=f(1),
               blurred_mask=f(1),
               segmentation=torch.empty((n, s, 2 * s, 1), dtype=torch.int32, device=dev))
    r = {k: raw[k].contiguous() for k in RAW_DTYPES}
    rc = _lib.lib().se3ds_input_transform(
        _lib.ptr(r['image']), _lib.ptr(r['proj_image']), _lib.ptr(r['depth']),
        _lib.ptr(r['proj_depth']), _lib.ptr(r['proj_mask']), _lib.ptr(r['blurred_mask']),
        _lib.ptr(r['segmentation']), _lib.ptr(ipd), _lib.ptr(fpd), n, h0, w0, s, 2 * s,
        _lib.ptr(out['image']), _lib.ptr(out['proj_image']), _lib.ptr(out['proj_mask']),
        _lib.ptr(out['proj_depth']), _lib.ptr(out['depth']), _lib.ptr(out['blurred_mask']),
        _lib.ptr(out['segmentation']), _lib.stream())
    _lib.check(rc, 'se3ds_input_transform')
    return out

  def transform(self, raw: Dict[str, torch.Tensor], rng: np.random.Generator):
    """Draws + device transform of one batch."""
    n, h0, w0 = raw['proj_mask'].shape
    return self.device_transform(raw, [self.draw_params(rng, h0, w0) for _ in range(n)])


VIDEO_PLANES = dict(segmentation=torch.uint8, pathdreamer_segmentation=torch.uint8,
                    depth=torch.float32, pathdreamer_depth=torch.float32)
VIDEO_OPTIONAL = ('pathdreamer_segmentation', 'pathdreamer_depth')   # older records lack them
VIDEO_PASS_THROUGH = ('id', 'mask', 'depth_scale', 'dataset_type', 'scan_id')


@gin.configurable
class R2RVideoDataset:
  """Preprocessing of R2R trajectories for evaluation (reference :604-827).

  TFRecord parsing stays outside: `raw` / `examples` hold what the reference's `_parse` (:626-719)
  yields.  Not built: `one_hot_mask` of `_eval_transform_fn` (:797-801) -- no model in the reference
  or here reads it (the evaluator rebuilds its own, the image models ignore it) and at 512x1024 it is
  440 MB of fp32 per example -- and the `z` entry (the noise is drawn on the device, as for
  `R2RImageDataset`)."""

  def __init__(self, image_size: int = 256, preprocessed_image_height: int = 512,
               num_classes: int = constants.NUM_MP3D_CLASSES, data_dir: str = 'data/val/',
               return_filename: bool = False, video_length: int = constants.PANO_VIDEO_LENGTH,
               horizontal_mask_ratio: float = 0.0, **kwargs):
    del kwargs
    self.image_size = image_size
    self.preprocessed_image_height = preprocessed_image_height
    self.num_classes = num_classes
    self.data_dir = data_dir
    self.return_filename = return_filename
    self.video_length = video_length
    self.horizontal_mask_ratio = horizontal_mask_ratio

  @property
  def num_examples(self):
    return {'train': 4675, 'val_unseen': 783, 'val_seen': 340}

  def get_file_patterns(self, split: Optional[str] = None, file_pattern: Optional[str] = None):
    """The file pattern of a split (:721-732); string logic only, nothing is opened."""
    if not file_pattern:
      if split not in ('train', 'val_seen', 'val_unseen'):
        raise ValueError(
            f"Expected split to be one of ['train', 'val_seen', 'val_unseen'], got {split}")
      file_pattern = self.data_dir + f'{split}*.tfrecord'
    return file_pattern

  # ------------------------------------------------------------------------------ the draws
  def draw_params(self, rng: np.random.Generator) -> dict:
    """One example's random draws, in the statement order of `_transform_fn` (:753-757), in fp32
    on the host.  hmask = (mode, start, end) on the OUTPUT grid of width 2 * image_size: mode 1
    keeps start < x < end, mode 2 (start > end, the band wraps) keeps x > start or x < end.  The
    generator is not touched when horizontal_mask_ratio is 0."""
    prm = dict(hmask=None)
    if self.horizontal_mask_ratio > 0:
      width = self.image_size * 2
      start = F32(rng.uniform(0, width))
      # width * (1 - ratio) is a Python constant in the reference, rounded to fp32 once
      end = F32(np.mod(start + F32(width * (1 - self.horizontal_mask_ratio)), F32(width)))
      prm['hmask'] = (2 if start > end else 1, float(start), float(end))
    return prm

  # ------------------------------------------------------------------------- device transform
  def device_transform(self, raw: Dict[str, torch.Tensor], params: List[dict]
                       ) -> Dict[str, torch.Tensor]:
    """raw: one batch of parsed examples on the GPU -- image fp32 (N,T,H0,W0,3); segmentation /
    pathdreamer_segmentation uint8 and depth / pathdreamer_depth fp32 (N,T,H0,W0) (the two
    pathdreamer planes may be absent); position fp32 (N,T,4); mask fp32 (N,T); depth_scale (N,);
    dataset_type; id.  params: one draw_params row per example, shared by its T frames.

    Returns the reference's output dict (:769-780) at (h, w) = (image_size, 2 * image_size): image,
    original_image fp32 (N,T,h,w,3), segmentation planes uint8 and depth planes fp32 (N,T,h,w,1),
    the rest passed through.  Two deliberate points:
      * when no row carries a band mask, `image` IS `original_image` (one buffer, one write), as
        the reference returns the same tensor under both keys;
      * `position` is the contiguous (N,T,3) xyz that generated_rollout and _get_image_grid take;
        the fourth component only ever lands in the homogeneous row, which the projection never
        reads (reference utils/pano_utils.py:139).  The 4-vector stays under `position_xyz1`."""
    image = raw['image']
    _lib.require_cuda(image)
    if image.dtype != torch.float32:
      raise ValueError(f'image: expected {torch.float32}, got {image.dtype}')
    if image.dim() != 5 or image.shape[-1] != 3:
      raise ValueError(f'image: expected (N,T,H0,W0,3), got {tuple(image.shape)}')
    n, t, h0, w0, _ = image.shape
    dev = image.device
    planes = {}
    for k, dt in VIDEO_PLANES.items():
      if k not in raw:
        if k in VIDEO_OPTIONAL:
          continue
        raise ValueError(f'{k}: missing from the batch')
      v = raw[k]
      _lib.require_cuda(v)
      if v.dtype != dt:
        raise ValueError(f'{k}: expected {dt}, got {v.dtype}')
      if tuple(v.shape) != (n, t, h0, w0):
        raise ValueError(f'{k}: expected {(n, t, h0, w0)} as the image has, got {tuple(v.shape)}')
      if v.device != dev:
        raise ValueError(f'{k}: on {v.device}, the image is on {dev}')
      planes[k] = v.contiguous()
    position = raw['position']
    _lib.require_cuda(position)
    if position.dtype != torch.float32 or tuple(position.shape) != (n, t, 4):
      raise ValueError(f'position: expected float32 {(n, t, 4)}, got {position.dtype} '
                       f'{tuple(position.shape)}')
    if 'mask' in raw and tuple(raw['mask'].shape) != (n, t):
      raise ValueError(f"mask: expected {(n, t)}, got {tuple(raw['mask'].shape)}")
    if len(params) != n:
      raise ValueError(f'{len(params)} parameter rows for a batch of {n}')
    s = self.image_size
    h, w = s, 2 * s
    hmasks = [prm.get('hmask') for prm in params]
    f = lambda c: torch.empty((n, t, h, w, c), dtype=torch.float32, device=dev)
    u = lambda: torch.empty((n, t, h, w, 1), dtype=torch.uint8, device=dev)
    original = f(3)
    masked = hm = hb = None
    if any(m is not None for m in hmasks):
      mode = np.zeros((n,), np.int32)
      band = np.zeros((n, 2), F32)
      for i, m in enumerate(hmasks):
        if m is not None:
          if m[0] not in (1, 2):
            raise ValueError(f'hmask mode {m[0]} (1: start < x < end, 2: x > start or x < end)')
          mode[i], band[i, 0], band[i, 1] = m
      # one upload: the N modes, then the 2N band bounds as their bit patterns
      rows = torch.from_numpy(np.concatenate([mode, band.reshape(-1).view(np.int32)])).to(dev)
      hm, hb = rows[:n], rows[n:]
      masked = f(3)
    out_planes = {k: (u() if dt == torch.uint8 else f(1)) for k, dt in VIDEO_PLANES.items()
                  if k in planes}
    g = lambda d, k: _lib.ptr(d.get(k))
    rc = _lib.lib().se3ds_video_transform(
        _lib.ptr(image.contiguous()), g(planes, 'segmentation'),
        g(planes, 'pathdreamer_segmentation'), g(planes, 'depth'), g(planes, 'pathdreamer_depth'),
        _lib.ptr(hm), _lib.ptr(hb), n, t, h0, w0, h, w, _lib.ptr(original), _lib.ptr(masked),
        g(out_planes, 'segmentation'), g(out_planes, 'pathdreamer_segmentation'),
        g(out_planes, 'depth'), g(out_planes, 'pathdreamer_depth'), _lib.stream())
    _lib.check(rc, 'se3ds_video_transform')
    out = {k: raw[k] for k in VIDEO_PASS_THROUGH if k in raw}
    out.update(image=original if masked is None else masked, original_image=original,
               position=position[..., :3].contiguous(), position_xyz1=position, **out_planes)
    return out

  def transform(self, raw: Dict[str, torch.Tensor], rng: np.random.Generator):
    """Draws + device transform of one batch."""
    return self.device_transform(raw, [self.draw_params(rng) for _ in range(raw['image'].shape[0])])

  # ---------------------------------------------------------------------------------- input_fn
  @staticmethod
  def batch_examples(examples: Union[Sequence[dict], Callable[[], Iterable[dict]]], batch_size: int,
                     num_epochs: Optional[int] = None) -> Iterator[Dict[str, np.ndarray]]:
    """The host half of input_fn: per-example dicts of NumPy arrays (one `_parse` result each) ->
    stacked batches.  As in the reference's input_fn (datasets/base_dataset.py:119-143) `repeat`
    comes before `batch`: the stream repeats (num_epochs=None: for ever), batches run across the
    epoch boundary and only the tail of a finite stream is dropped.  examples: a sequence, or a
    zero-argument callable that returns a fresh iterator for each epoch."""
    if batch_size <= 0:
      raise ValueError(f'batch_size {batch_size}')
    pending = []
    epoch = 0
    while num_epochs is None or epoch < num_epochs:
      seen = 0
      for ex in (examples() if callable(examples) else examples):
        seen += 1
        pending.append(ex)
        if len(pending) == batch_size:
          yield {k: np.stack([np.asarray(e[k]) for e in pending]) for k in pending[0]}
          pending = []
      if seen == 0:
        raise ValueError('no examples to batch')
      epoch += 1

  def input_fn(self, examples, batch_size: int, seed: int = 0, num_epochs: Optional[int] = None,
               device=None) -> Iterator[Dict[str, torch.Tensor]]:
    """Generator of transformed batches on the device: per batch stack, upload, draw, transform.
    This is the object handed to EvalMetric(ds=...), which draws eval_num // batch_size + 1
    batches per pass and makes several passes, so the default stream never ends.  String-valued
    entries (scan_id with return_filename) stay on the host."""
    dev = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
    rng = np.random.default_rng(seed)
    for batch in self.batch_examples(examples, batch_size, num_epochs):
      if not self.return_filename:
        batch.pop('scan_id', None)
      raw = {k: (v if v.dtype.kind in 'USO' else torch.from_numpy(v).to(dev))
             for k, v in batch.items()}
      yield self.transform(raw, rng)
