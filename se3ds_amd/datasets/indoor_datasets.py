"""Device-side half of the reference's datasets/indoor_datasets.py: `augment`
(:34-61) and `R2RImageDataset`'s per-example transform (:263-375) + batch transform (:553-597) as
ONE gather kernel over decoded frames resident in HBM (`se3ds_input_transform`), fed either by the
caller (uint8 / uint16 frames, what `tf.image.decode_png` yields, :185-228, as CUDA tensors) or
straight from the published TFRecord files: `R2RImageDataset._parse` (:125-247) reads a record with
utils/tf_records.py, `input_fn` (datasets/base_dataset.py:105-150) lists, repeats, shuffles and
batches them, and utils/png.py decodes the seven PNGs of every example -- inflate on a small host
thread pool (or, with inflate='device', in one launch of `se3ds_png_inflate`), reconstruction of the
whole batch in one launch (`se3ds_png_unfilter`).  TensorFlow is
not needed.  `RE10KImageDataset` reads the RE10K records (`visible_mask`, :232-240) and runs
`_transform_fn_re10k` (:377-535): the extents of the visible pixels are reduced on the device
(`se3ds_re10k_extent`) and the crop box is evaluated inside the gather (`se3ds_re10k_transform`).
Not built: sharding over several input pipelines beyond the seed offset, `cache`, batches that mix
MP3D and RE10K records.

Same constructor arguments and gin selectors as the reference (`R2RImageDataset.image_size`, ...).
The random draws follow the statement order of `_transform_fn` and are made on the host with a
NumPy generator (TensorFlow's RNG streams cannot be reproduced without TensorFlow); everything
downstream of the draws is bit-exact against oracle/input_np.py.

`R2RVideoDataset` is the evaluation side (:604-827): the per-example transform of the trajectory
records (`_transform_fn`, :734-792) over all N*T frames of a batch as one gather
(`se3ds_video_transform`), and an `input_fn` that batches parsed examples the way the reference's
tf.data pipeline does (repeat, then batch) and yields what `EvalMetric` consumes;
`examples_from_tfrecords` parses the trajectory records (:626-719) into those examples."""
import concurrent.futures
import enum
import glob
import os
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Union

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd import constants
from se3ds_amd import gin_lite as gin
from se3ds_amd.utils import png
from se3ds_amd.utils._staging import Readback, cuda_device
from se3ds_amd.utils import tf_records
from se3ds_amd.utils.tf_records import FixedLenFeature

F32 = np.float32
RAW_DTYPES = dict(image=torch.uint8, proj_image=torch.uint8, depth=torch.int16, proj_depth=torch.int16,
                  proj_mask=torch.uint8, blurred_mask=torch.uint8, segmentation=torch.uint8)

# plane -> (feature of the record, channels, bit depth) as `_parse` decodes it (:185-228)
IMAGE_PLANES = dict(image=('image/encoded', 3, 8), proj_image=('proj/encoded', 3, 8),
                    depth=('image/depth', 1, 16), proj_depth=('proj/depth', 1, 16),
                    proj_mask=('proj/mask', 1, 8), blurred_mask=('image/blurred_mask', 1, 8),
                    segmentation=('image/segmentation/class/encoded', 1, 8))


class DatasetType(enum.Enum):
  MP3D = 0
  GIBSON = 1  # Unused
  RE10K = 2


def _record_files(file_pattern: str) -> List[str]:
  """The sorted files of a pattern.  No match raises ValueError with the reference's message; the
  reference raises it as AssertionError (`assert tf.io.gfile.glob(...)`, base_dataset.py:59), which
  would vanish under `python -O`."""
  files = sorted(glob.glob(file_pattern))
  if not files:
    raise ValueError(f'No data files matched {file_pattern}')
  return files


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

  # what `_parse` decodes and `input_fn` batches; RE10KImageDataset has its own tables
  RAW_DTYPES = RAW_DTYPES
  IMAGE_PLANES = IMAGE_PLANES

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

  def _transform_examples(self, examples: List[dict], raw: Dict[str, torch.Tensor],
                          params: List[dict]):
    """input_fn's transform of one decoded batch: -> (batch, status).  status: None, or an object
    whose `check()` waits for a per-example status the launch left on the device and raises
    ValueError -- input_fn calls it just before it yields the batch."""
    del examples
    return self.device_transform(raw, params), None

  # --------------------------------------------------------------------------- TFRecord input
  def _features(self) -> Dict[str, FixedLenFeature]:
    """The feature spec of the reference's `_parse` (:149-178)."""
    s = lambda: FixedLenFeature([], 'string', '')
    return {
        'scan_id': s(),
        'dataset_type': FixedLenFeature([], 'int64', 0),
        'depth_scale': FixedLenFeature([], 'float32', 10.0),
        'image/encoded': s(), 'image/filename': s(), 'image/depth': s(), 'image/visible_mask': s(),
        'image/blurred_mask': s(), 'image/segmentation/class/encoded': s(), 'proj/encoded': s(),
        'proj/depth': s(), 'proj/mask': s(),
        'bbox': FixedLenFeature([4], 'float32', [0.0, 0.0, 0.0, 0.0]),
    }

  def _parse(self, record: bytes, inflate: str = 'host') -> dict:
    """One serialized tf.train.Example -> the host half of the reference's `_parse` (:125-247): the
    seven planes of RAW_DTYPES as `png.PngPlane`s (container parsed, IDAT inflated, NOT yet
    reconstructed -- `png.decode_png_batch` does that for a whole batch on the device), plus
    dataset_type, depth_scale, bbox and, with return_filename, filename and scan_id.  With
    inflate='device' the planes are `png.PngStream`s: the container is walked, nothing is inflated.

    A plane that is not (preprocessed_image_height, 2 * preprocessed_image_height) raises
    ValueError, as `set_shape` does; so does one of another kind than the reference decodes it to
    (RGB for the two images, 16-bit grey for the two depths, 8-bit grey for the rest: no channel
    conversion is built).  `segmentation_valid` (:222-223) is left out: nothing in the reference's
    trainer or here reads it.  Records of DatasetType.RE10K raise NotImplementedError
    (`RE10KImageDataset` reads them)."""
    ex = tf_records.apply_features(tf_records.parse_example(record), self._features())
    if ex['dataset_type'] == DatasetType.RE10K.value:
      raise NotImplementedError('RE10K records (visible_mask, _transform_fn_re10k) are not supported')
    return self._parsed(ex, inflate)

  def _parsed(self, ex: dict, inflate: str) -> dict:
    """The planes of self.IMAGE_PLANES and the scalars of one Example that `_features` was applied
    to: the body of `_parse`."""
    h, w = self.preprocessed_image_height, 2 * self.preprocessed_image_height
    out = dict(dataset_type=np.int64(ex['dataset_type']))
    for name, (feature, channels, depth) in self.IMAGE_PLANES.items():
      try:
        plane = (png.parse_png if inflate == 'host' else png.parse_png_container)(ex[feature])
      except (ValueError, NotImplementedError) as e:
        raise type(e)(f'{feature}: {e}') from None
      if (plane.height, plane.width) != (h, w):
        raise ValueError(f'{feature}: a {plane.height}x{plane.width} plane, the dataset is '
                         f'preprocessed to {h}x{w}')
      if (plane.channels, plane.bit_depth) != (channels, depth):
        raise ValueError(f'{feature}: {plane.channels} channel(s) at bit depth {plane.bit_depth}, '
                         f'expected {channels} at {depth}')
      out[name] = plane
    out['depth_scale'] = np.float32(ex['depth_scale'])
    out['bbox'] = ex['bbox']
    if self.return_filename:
      out['filename'] = ex['image/filename']
      out['scan_id'] = ex['scan_id']
    return out

  def get_file_patterns(self, split: Optional[str] = None, file_pattern: Optional[str] = None):
    """The file pattern of a split (:249-261), with the reference's strings and errors."""
    if not file_pattern:
      if split not in ('train', 'val', 'val_unseen', 'val_seen', 'test'):
        raise ValueError(f"Expected split to be one of ['train', 'val'], got {split}")
      file_pattern = os.path.join(self.data_dir, f'{split}*.tfrecord')
    return file_pattern

  def _records(self, files: List[str], num_epochs: Optional[int], shuffle: bool,
               shuffle_buffer_size: int, rng: np.random.Generator,
               verify_crc=False) -> Iterator[bytes]:
    """files in order, records in file order, repeat, then tf.data's shuffle buffer: fill to
    `shuffle_buffer_size`, then emit a uniformly drawn slot and refill it; drain at the end."""
    def stream():
      epoch = 0
      while num_epochs is None or epoch < num_epochs:
        seen = 0
        for path in files:
          for rec in tf_records.read_records(path, verify=verify_crc):
            seen += 1
            yield rec
        if seen == 0:
          raise ValueError(f'no records in {files}')
        epoch += 1
    if not shuffle:
      yield from stream()
      return
    if shuffle_buffer_size < 1:
      raise ValueError(f'shuffle_buffer_size {shuffle_buffer_size}')
    buf = []
    for rec in stream():
      if len(buf) < shuffle_buffer_size:
        buf.append(rec)
        continue
      i = int(rng.integers(len(buf)))
      out, buf[i] = buf[i], rec
      yield out
    while buf:
      yield buf.pop(int(rng.integers(len(buf))))

  def input_fn(self, split: Optional[str] = None, batch_size: int = 1,
               num_epochs: Optional[int] = None, shuffle: bool = False,
               shuffle_buffer_size: int = 1000, file_pattern: Optional[str] = None, seed: int = 1,
               input_pipeline_id: int = 0, device=None, decode_threads: int = 4,
               verify_crc=False, inflate: str = 'host') -> Iterator[Dict[str, torch.Tensor]]:
    """Generator of step batches on the device, from TFRecord files: the dict `device_transform`
    returns plus `depth_scale` fp32 (N,) (and, with return_filename, the host lists `filename` and
    `scan_id`).  This is what GANManager.train(train_ds=...) takes.

    The order is that of the reference's input_fn (datasets/base_dataset.py:105-150): files sorted,
    records in file order, repeat(num_epochs), the shuffle buffer, batch with the remainder dropped
    (batches run across the epoch boundary), decode, `draw_params` per example in batch order,
    `device_transform`.  Two NumPy generators, both seeded seed + input_pipeline_id, make the
    shuffle buffer's draws and the transform's draws (TensorFlow's streams cannot be reproduced).
    The records of the NEXT batch are parsed and inflated on `decode_threads` workers (capped at
    16) while the caller runs the current step; reconstruction is one launch per batch.

    `verify_crc` is off by default.  True checks both checksums of every record with
    utils/tf_bundle.crc32c, a Python byte loop of about 5 MB/s that holds the GIL -- a few hundred
    ms per 512 x 1024 record of seven PNGs on the generator's own thread, where no prefetch hides
    it: for auditing a file once.  'device' checks them with the CRC-32C kernel (utils/crc32c.py,
    `tf_records.read_records(verify='device')`): the records are uploaded in batches of 64 MiB and
    checked with one call per batch, at memory speed; whether it becomes the default
    is decided from measurements, not here.  With the default, damage still surfaces in part:
    every PNG chunk carries a CRC-32 that parse_png checks with zlib (C code), a broken protobuf or
    a wrong geometry raises, and a lost record boundary ends in `truncated record`.

    inflate='device': the workers walk the PNG containers only and the IDAT streams are inflated on
    the device (`png.decode_png_batch_async`).  The upload, inflate, reconstruction and transform of
    the NEXT batch are queued on the current stream before the current batch is yielded, and a
    batch's status words are waited for just before it is yielded -- the overlap the host path gets
    from its pool.  A stream that does not inflate raises ValueError naming plane, index and
    reason.  The batches are the same bit for bit."""
    if batch_size <= 0:
      raise ValueError(f'batch_size {batch_size}')
    png.check_inflate_mode(inflate)
    dev = cuda_device(device, 'input_fn', 'decodes and transforms')
    files = _record_files(self.get_file_patterns(split, file_pattern))
    local_seed = seed + input_pipeline_id
    draw_rng = np.random.default_rng(local_seed)
    records = self._records(files, num_epochs, shuffle, shuffle_buffer_size,
                            np.random.default_rng(local_seed), verify_crc)
    threads = max(1, min(int(decode_threads), png.MAX_THREADS))
    h0, w0 = self.preprocessed_image_height, 2 * self.preprocessed_image_height

    def submit(pool):
      futures = []
      for rec in records:
        futures.append(pool.submit(self._parse, rec, inflate))
        if len(futures) == batch_size:
          return futures
      return None   # the remainder is dropped

    def finish(examples, raw):
      """-> the batch and its unchecked status (`_transform_examples`)."""
      params = [self.draw_params(draw_rng, h0, w0) for _ in examples]
      batch, status = self._transform_examples(examples, raw, params)
      batch['depth_scale'] = torch.from_numpy(
          np.array([e['depth_scale'] for e in examples], F32)).to(dev)
      if self.return_filename:
        batch['filename'] = [e['filename'] for e in examples]
        batch['scan_id'] = [e['scan_id'] for e in examples]
      return batch, status

    def enqueue(futures):
      """A batch queued on the device with its inflate unchecked, or the exception that stopped it
      (raised when the batch's turn comes, as on the host path)."""
      if futures is None:
        return None
      try:
        examples = [f.result() for f in futures]
        raw, check = png.decode_png_batch_async(
            {k: [e[k] for e in examples] for k in self.RAW_DTYPES}, dev)
        return finish(examples, raw), check
      except Exception as e:   # noqa: BLE001  re-raised below
        return e

    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
      pending = submit(pool)
      if inflate == 'device':
        queued = enqueue(pending)
        while queued is not None:
          if isinstance(queued, Exception):
            raise queued
          following = enqueue(submit(pool))   # queued behind this batch, ahead of the caller's step
          (batch, status), check = queued
          check.check()
          if status is not None:
            status.check()
          yield batch
          queued = following
        return
      while pending is not None:
        examples = [f.result() for f in pending]
        pending = submit(pool)   # inflates under the step that consumes the batch below
        raw = png.decode_png_batch({k: [e[k] for e in examples] for k in self.RAW_DTYPES}, dev,
                                   threads)
        batch, status = finish(examples, raw)
        if status is not None:
          status.check()
        yield batch


# RAW_DTYPES / IMAGE_PLANES of an RE10K record: `visible_mask` where `blurred_mask` stood (:232-240)
RE10K_RAW_DTYPES = dict(image=torch.uint8, proj_image=torch.uint8, depth=torch.int16,
                        proj_depth=torch.int16, proj_mask=torch.uint8, visible_mask=torch.uint8,
                        segmentation=torch.uint8)
RE10K_IMAGE_PLANES = dict(image=('image/encoded', 3, 8), proj_image=('proj/encoded', 3, 8),
                          depth=('image/depth', 1, 16), proj_depth=('proj/depth', 1, 16),
                          proj_mask=('proj/mask', 1, 8), visible_mask=('image/visible_mask', 1, 8),
                          segmentation=('image/segmentation/class/encoded', 1, 8))
RE10K_STATUS = {1: 'visible_mask has no visible pixel',
                2: 'the crop box does not lie inside the frame'}


class PendingCrop(Readback):
  """The status words of one `se3ds_re10k_transform` launch on their way to the host: `check()`
  waits for them and raises ValueError for the first example whose crop could not be made.  The
  batch counts only once it has returned."""

  def check(self) -> None:
    words = self.wait()
    bad = np.flatnonzero(words)
    if bad.size:
      i = int(bad[0])
      reason = RE10K_STATUS.get(int(words[i]), f'status {int(words[i])}')
      raise ValueError(f'example {i} of the batch: {reason}')


@gin.configurable
class RE10KImageDataset(R2RImageDataset):
  """Preprocessing of RealEstate10K records for training: the reference's `_parse` branch for
  DatasetType.RE10K (:232-240) and `_transform_fn_re10k` (:377-535), whose call the reference has
  commented out (:538-546).  Here the dispatch is this class, not `dataset_type`: R2RImageDataset
  goes on refusing such records.  Same constructor arguments, defaults and gin selectors as
  R2RImageDataset (`re_10k_crop` is off by default, as in the reference).

  With `re_10k_crop and random_crop` every plane is cropped to a padded, shifted box around the
  visible pixels and resized to (image_size, 2 * image_size); otherwise the outputs keep the raw
  size and hold conversion, band masks and the batch transform only (:474).  The extents of the
  visible pixels are found on the device (`se3ds_re10k_extent`) and the box is evaluated inside
  the gather (`se3ds_re10k_transform`, csrc/re10k_box_core.h): the host never sees the mask.

  `input_fn` is R2RImageDataset's, signature and order of the records included; its batches carry
  `bbox` as well.  The device leaves one status word per example (0 ok, 1 no visible pixel, 2 the
  box does not lie inside the frame); input_fn reads a batch's words just before it yields the
  batch, behind the launches of the next one with inflate='device', and raises ValueError naming
  the example."""

  RAW_DTYPES = RE10K_RAW_DTYPES
  IMAGE_PLANES = RE10K_IMAGE_PLANES

  def _parse(self, record: bytes, inflate: str = 'host') -> dict:
    """As R2RImageDataset._parse, with the plane `visible_mask` (`image/visible_mask`, 8-bit grey,
    frame size) in place of `blurred_mask`.  `image/blurred_mask` is not read: the reference decodes
    it and then overwrites it with 1 - visible_mask (:238), so it may be empty here.  A record of
    another dataset_type, and a missing or wrong-kind `image/visible_mask`, raise ValueError."""
    ex = tf_records.apply_features(tf_records.parse_example(record), self._features())
    if ex['dataset_type'] != DatasetType.RE10K.value:
      raise ValueError(f"dataset_type {int(ex['dataset_type'])}: RE10KImageDataset reads records of "
                       f'DatasetType.RE10K ({DatasetType.RE10K.value}) only')
    return self._parsed(ex, inflate)

  # ------------------------------------------------------------------------------ the draws
  def draw_params(self, rng: np.random.Generator, height: int, width: int) -> dict:
    """One example's random draws, in the statement order of `_transform_fn_re10k` (:389-443), each
    rounded to fp32: hmask and vmask as in R2RImageDataset.draw_params, then, only with
    re_10k_crop, pad in [pad_minval, pad_maxval) and x_shift, y_shift in +-0.5 |pad|.  No resize,
    roll, flip or crop offset is drawn; the generator is not touched for a part that is off."""
    prm = dict(hmask=None, vmask=None, pad=None, x_shift=None, y_shift=None)
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
    if self.re_10k_crop:
      pad = F32(rng.uniform(self.pad_minval, self.pad_maxval))
      half = F32(0.5) * np.abs(pad)
      prm['pad'] = float(pad)
      prm['x_shift'] = float(F32(rng.uniform(-half, half)))
      prm['y_shift'] = float(F32(rng.uniform(-half, half)))
    return prm

  # ------------------------------------------------------------------------- device transform
  def _launch(self, raw: Dict[str, torch.Tensor], params: List[dict], bbox=None):
    """Both launches of one batch, nothing waited for: -> (batch, PendingCrop)."""
    for k, dt in RE10K_RAW_DTYPES.items():
      _lib.require_cuda(raw[k])
      if raw[k].dtype != dt:
        raise ValueError(f'{k}: expected {dt}, got {raw[k].dtype}')
    n, h0, w0 = raw['proj_mask'].shape
    for k in RE10K_RAW_DTYPES:
      if tuple(raw[k].shape[:3]) != (n, h0, w0):
        raise ValueError(f'{k}: {tuple(raw[k].shape)}, proj_mask is {(n, h0, w0)}')
    if len(params) != n:
      raise ValueError(f'{len(params)} parameter rows for a batch of {n}')
    crop = bool(self.re_10k_crop and self.random_crop)
    h, w = (self.image_size, 2 * self.image_size) if crop else (h0, w0)
    ext = np.tile(np.array([h0, -1, w0, -1], np.int32), (n, 1))
    ip = np.zeros((n, 3), np.int32)
    fp = np.zeros((n, 7), F32)
    for i, prm in enumerate(params):
      if prm.get('hmask') is not None:
        if prm['hmask'][0] not in (1, 2):
          raise ValueError(f"hmask mode {prm['hmask'][0]} (1: start < x < end, 2: x > start or x < end)")
        ip[i, 0], fp[i, 0], fp[i, 1] = prm['hmask']
      if prm.get('vmask') is not None:
        ip[i, 1] = 1
        fp[i, 2], fp[i, 3] = prm['vmask']
      if crop:
        if prm.get('pad') is None:
          raise ValueError(f'parameter row {i} has no pad / x_shift / y_shift draw')
        ip[i, 2] = 1
        fp[i, 4:7] = (prm['pad'], prm['x_shift'], prm['y_shift'])
    dev = raw['proj_mask'].device
    if bbox is None:
      if not crop:
        raise ValueError("bbox: the record's bbox is needed unless re_10k_crop and random_crop")
    elif not crop:
      bbox = torch.as_tensor(bbox, dtype=torch.float32).to(dev)
      if tuple(bbox.shape) != (n, 4):
        raise ValueError(f'bbox: expected {(n, 4)}, got {tuple(bbox.shape)}')
    with torch.cuda.device(dev):
      # one upload: the initial extents, the integer rows, the fp32 rows as their bit patterns
      rows = torch.from_numpy(np.concatenate(
          [ext.reshape(-1), ip.reshape(-1), fp.reshape(-1).view(np.int32)])).to(dev)
      extd, ipd, fpd = rows[:4 * n], rows[4 * n:7 * n], rows[7 * n:].view(torch.float32)
      f = lambda c: torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
      out = dict(image=f(3), proj_image=f(3), proj_mask=f(1), proj_depth=f(1), depth=f(1),
                 blurred_mask=f(1),
                 segmentation=torch.empty((n, h, w, 1), dtype=torch.int32, device=dev))
      status = torch.empty((n,), dtype=torch.int32, device=dev)
      r = {k: raw[k].contiguous() for k in RE10K_RAW_DTYPES}
      L = _lib.lib()
      if crop:
        out['bbox'] = torch.empty((n, 4), dtype=torch.int32, device=dev)
        rc = L.se3ds_re10k_extent(_lib.ptr(r['visible_mask']), n, h0, w0, _lib.ptr(extd), _lib.stream())
        _lib.check(rc, 'se3ds_re10k_extent')
      else:
        out['bbox'] = bbox
      rc = L.se3ds_re10k_transform(
          _lib.ptr(r['image']), _lib.ptr(r['proj_image']), _lib.ptr(r['depth']),
          _lib.ptr(r['proj_depth']), _lib.ptr(r['proj_mask']), _lib.ptr(r['visible_mask']),
          _lib.ptr(r['segmentation']), _lib.ptr(extd) if crop else None, _lib.ptr(ipd),
          _lib.ptr(fpd), n, h0, w0, h, w, _lib.ptr(out['image']), _lib.ptr(out['proj_image']),
          _lib.ptr(out['proj_mask']), _lib.ptr(out['proj_depth']), _lib.ptr(out['depth']),
          _lib.ptr(out['blurred_mask']), _lib.ptr(out['segmentation']),
          _lib.ptr(out['bbox']) if crop else None, _lib.ptr(status), _lib.stream())
      _lib.check(rc, 'se3ds_re10k_transform')
      return out, PendingCrop(status)

  def device_transform(self, raw: Dict[str, torch.Tensor], params: List[dict], bbox=None
                       ) -> Dict[str, torch.Tensor]:
    """raw: R2RImageDataset.device_transform's dict with `visible_mask` uint8 (N,H0,W0) in place of
    `blurred_mask`.  Returns the step's batch dict (`blurred_mask` = 1 - visible) plus `bbox`:
      * re_10k_crop and random_crop: outputs at (image_size, 2 * image_size); bbox int32 (N,4) =
        [x_min, y_min, x_max, y_max] as the device found it (:520);
      * otherwise: outputs at the raw (H0, W0); bbox is the argument, the records' fp32 (N,4).
    One small download checks the per-example status; an example without a visible pixel, or
    whose box does not lie inside the frame, raises ValueError naming it."""
    out, status = self._launch(raw, params, bbox)
    status.check()
    return out

  def transform(self, raw: Dict[str, torch.Tensor], rng: np.random.Generator, bbox=None):
    """Draws + device transform of one batch."""
    n, h0, w0 = raw['proj_mask'].shape
    return self.device_transform(raw, [self.draw_params(rng, h0, w0) for _ in range(n)], bbox)

  def _transform_examples(self, examples, raw, params):
    return self._launch(raw, params, np.stack([np.asarray(e['bbox'], F32) for e in examples]))


VIDEO_PLANES = dict(segmentation=torch.uint8, pathdreamer_segmentation=torch.uint8,
                    depth=torch.float32, pathdreamer_depth=torch.float32)
VIDEO_OPTIONAL = ('pathdreamer_segmentation', 'pathdreamer_depth')   # older records lack them
VIDEO_PASS_THROUGH = ('id', 'mask', 'depth_scale', 'dataset_type', 'scan_id')


@gin.configurable
class R2RVideoDataset:
  """Preprocessing of R2R trajectories for evaluation (reference :604-827).

  `raw` / `examples` hold what the reference's `_parse` (:626-719) yields; `examples_from_tfrecords`
  makes them from the published files.  Not built: `one_hot_mask` of `_eval_transform_fn` (:797-801) -- no model in the reference
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

  # --------------------------------------------------------------------------- TFRecord input
  def _features(self) -> Dict[str, FixedLenFeature]:
    """The feature spec of the reference's `_parse` (:648-671), and the two `pathdreamer_*` planes
    it reads as optional strings (older records lack them, VIDEO_OPTIONAL)."""
    s = lambda: FixedLenFeature([], 'string', '')
    return {
        'id': FixedLenFeature([], 'int64', 0),
        'scan_id': s(),
        'dataset_type': FixedLenFeature([], 'int64', 0),
        'depth_scale': FixedLenFeature([], 'float32', constants.DEPTH_SCALE),
        'video/num_frames': FixedLenFeature([], 'int64'),
        'video/rgb': s(), 'video/segmentations': s(), 'video/depth': s(), 'video/position': s(),
        'video/mask': s(), 'video/pathdreamer_segmentations': s(), 'video/pathdreamer_depth': s(),
    }

  def _parse(self, record: bytes) -> Dict[str, np.ndarray]:
    """One serialized trajectory Example -> the dict of NumPy arrays the reference's `_parse`
    (:626-719) yields and `input_fn(examples=...)` takes: image fp32 (T,H0,W0,3), position fp32
    (T,4), mask fp32 (T,), segmentation uint8 and depth fp32 (T,H0,W0), the two pathdreamer planes
    when the record has them (segmentation stored int32, cast to uint8 as in :699-704), id,
    dataset_type, depth_scale and, with return_filename, scan_id.  T = PANO_VIDEO_LENGTH; a plane
    of another shape raises ValueError, as `ensure_shape` does."""
    ex = tf_records.apply_features(tf_records.parse_example(record), self._features())
    t = constants.PANO_VIDEO_LENGTH
    shape = (t, self.preprocessed_image_height, 2 * self.preprocessed_image_height)
    out = dict(id=np.int64(ex['id']), dataset_type=np.int64(ex['dataset_type']))

    def tensor(feature, dtype, want):
      a = tf_records.parse_tensor(ex[feature], dtype)
      if a.shape != want:
        raise ValueError(f'{feature}: shape {a.shape}, expected {want}')
      return a
    out['image'] = tensor('video/rgb', np.float32, shape + (3,))
    out['position'] = tensor('video/position', np.float32, (t, 4))
    out['mask'] = tensor('video/mask', np.float32, (t,))
    out['segmentation'] = tensor('video/segmentations', np.uint8, shape)
    if ex['video/pathdreamer_segmentations']:
      out['pathdreamer_segmentation'] = tensor('video/pathdreamer_segmentations', np.int32,
                                               shape).astype(np.uint8)
    out['depth'] = tensor('video/depth', np.float32, shape)
    if ex['video/pathdreamer_depth']:
      out['pathdreamer_depth'] = tensor('video/pathdreamer_depth', np.float32, shape)
    out['depth_scale'] = np.float32(ex['depth_scale'])
    if self.return_filename:
      out['scan_id'] = ex['scan_id']
    return out

  def examples_from_tfrecords(self, split: Optional[str] = None, file_pattern: Optional[str] = None,
                              verify_crc=False) -> Callable[[], Iterator[dict]]:
    """The parsed examples of a split's TFRecord files (sorted, records in file order) as a
    zero-argument callable that returns a fresh iterator -- what `input_fn(examples=...)` and
    GANManager.test(eval_examples=...) take; one example is in memory at a time.

    `verify_crc` is off by default, as in R2RImageDataset.input_fn.  Unlike the PNG planes,
    `tensor_content` carries no checksum of its own, so with the default only the framing, the
    protobuf structure, the dtypes and the shapes are checked.  True audits a file with the Python
    CRC-32C (a 512 x 1024 trajectory is roughly 100 MB of fp32: tens of seconds per record);
    'device' checks every record with the CRC-32C kernel (utils/crc32c.py) at memory speed."""
    files = _record_files(self.get_file_patterns(split, file_pattern))

    def examples():
      for path in files:
        for rec in tf_records.read_records(path, verify=verify_crc):
          yield self._parse(rec)
    return examples

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
               device=None, inflate: str = 'host') -> Iterator[Dict[str, torch.Tensor]]:
    """Generator of transformed batches on the device: per batch stack, upload, draw, transform.
    This is the object handed to EvalMetric(ds=...), which draws eval_num // batch_size + 1
    batches per pass and makes several passes, so the default stream never ends.  String-valued
    entries (scan_id with return_filename) stay on the host.

    `inflate` ('host' or 'device') is R2RImageDataset.input_fn's argument, accepted so that one
    configuration serves both datasets; the trajectory records carry serialized tensors, not PNGs,
    so there is nothing to inflate and both values give the same batches."""
    png.check_inflate_mode(inflate)
    dev = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
    rng = np.random.default_rng(seed)
    for batch in self.batch_examples(examples, batch_size, num_epochs):
      if not self.return_filename:
        batch.pop('scan_id', None)
      raw = {k: (v if v.dtype.kind in 'USO' else torch.from_numpy(v).to(dev))
             for k, v in batch.items()}
      yield self.transform(raw, rng)
