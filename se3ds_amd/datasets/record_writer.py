"""Writing R2R records: `train*.tfrecord` files that `R2RImageDataset.input_fn` reads bit for bit, built
on the device from the tensors that are already there, and evaluation trajectories for
`R2RVideoDataset`.  The reference tells its users to bring "data in the expected TFRecords format"
(README.md) and publishes no writer; this is the inverse of its `_parse`
(datasets/indoor_datasets.py:125-247 and :626-719), from the formats utils/tf_records.py documents.

  R2RRecordWriter      panoramas, depths and guidance planes in the raw dtypes of
                       `indoor_datasets.RAW_DTYPES` -> a record file.  Per flush: the seven planes of
                       every pending example are filtered and deflated in one call
                       (`se3ds_png_encode_planes`, 16-bit grey included), the sizes come back (the first
                       synchronisation), the host lays the file out -- every byte that has no width:
                       PNG signature, IHDR, IEND, IDAT framing and Adler-32, protobuf keys and varints,
                       record lengths -- and uploads those literals with the tables; then
                       `se3ds_assemble_segments` puts literals and streams in place,
                       `se3ds_crc32z_multi` + `se3ds_patch_crc` fill in the IDAT CRCs,
                       `se3ds_crc32c_multi` + `se3ds_patch_crc` the records' masked CRC-32C, and one
                       download (the second synchronisation) brings the finished bytes to the file.
  guidance_planes      the three stored guidance planes of an example from the previous panorama
  record_planes        the fp32 results of the warp -> stored planes (`se3ds_record_planes`)
  encode_records_host  the same layout in Python from PNG files already encoded: the tests' reference
  encode_trajectory_example   an evaluation record, written with
                       `tf_records.write_records(checksums='device')`

There is no CPU fallback on the product path: a non-CUDA tensor raises Se3dsHipError."""
import os
import struct
import time
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from se3ds_amd import _lib, constants
from se3ds_amd.datasets.indoor_datasets import IMAGE_PLANES, RAW_DTYPES
from se3ds_amd.utils import jpeg, png, tf_records
from se3ds_amd.utils._staging import Readback, cuda_device, upload
from se3ds_amd.utils.tf_bundle import _get_varint, _pb_bytes, _put_varint, crc32c, mask_crc

# the order in which an Example's planes are written; `_parse` reads them by name
_PLANE_ORDER = ('image', 'depth', 'blurred_mask', 'segmentation', 'proj_image', 'proj_depth', 'proj_mask')


class _Ref(NamedTuple):
  """A range of the encoder's compact output (source 1 of the assembly)."""
  offset: int
  length: int


class _Mark(NamedTuple):
  """A zero-width position the layout reports: 'idat' = the IDAT chunk's type field, 'idat_crc' =
  where its CRC goes."""
  kind: str


Piece = Union[bytes, _Ref, _Mark]


def _size(pieces: Sequence[Piece]) -> int:
  return sum(len(p) if isinstance(p, bytes) else p.length if isinstance(p, _Ref) else 0 for p in pieces)


def _wrap(field: int, pieces: List[Piece]) -> List[Piece]:
  """`_pb_bytes(field, ...)` around pieces: the key and the length varint in front."""
  return [_put_varint((field << 3) | 2) + _put_varint(_size(pieces))] + pieces


def _bytes_feature(key: str, value: List[Piece]) -> List[Piece]:
  """The map entry of a bytes_list Feature with one value, as `tf_records.encode_example` writes it."""
  feature = _wrap(1, _wrap(1, value))
  return _wrap(1, [_pb_bytes(1, key.encode())] + _wrap(2, feature))


def example_features(example: dict) -> Dict[str, object]:
  """The features of one training Example in the order this module writes them, for
  `tf_records.encode_example`: `example` maps the plane names of IMAGE_PLANES to encoded PNG files
  and may hold scan_id, filename, depth_scale, dataset_type and bbox (defaults: those of `add`)."""
  feats = {'scan_id': bytes(example.get('scan_id', b'')),
           'dataset_type': np.array([int(example.get('dataset_type', 0))], np.int64),
           'depth_scale': np.array([example.get('depth_scale', 10.0)], np.float32)}
  for name in _PLANE_ORDER:
    feats[IMAGE_PLANES[name][0]] = example[name]
    if name == 'image':
      feats['image/filename'] = bytes(example.get('filename', b''))
  feats['bbox'] = np.asarray(example.get('bbox', (0, 0, 0, 0)), np.float32).reshape(4)
  return feats


def _example_pieces(example: dict) -> List[Piece]:
  """The payload of one record: `tf_records.encode_example(example_features(example))`, where a
  plane may be a list of pieces instead of bytes."""
  entries: List[Piece] = []
  for key, value in example_features(example).items():
    if isinstance(value, list):
      entries += _bytes_feature(key, value)
    else:
      # encode_example of one feature is field 1 (Features) around its map entry: take the entry
      one = tf_records.encode_example({key: value})
      entries.append(one[_get_varint(one, 1)[1]:])
  return _wrap(1, entries)


def _png_pieces(height: int, row_bytes: int, bpp: int, at: int, size: int, adler: int) -> List[Piece]:
  """`png.png_container` around a deflate stream that stays on the device: everything but the stream
  and the IDAT chunk's CRC."""
  depth, channels, width = (16, 1, row_bytes // 2) if bpp == 2 else (8, bpp, row_bytes // bpp)
  ihdr = struct.pack('>IIBBBBB', width, height, depth, 0 if channels == 1 else 2, 0, 0, 0)
  return [png.SIGNATURE + png._chunk(b'IHDR', ihdr) + struct.pack('>I', 2 + size + 4), _Mark('idat'),
          b'IDAT\x78\x01', _Ref(at, size), struct.pack('>I', adler), _Mark('idat_crc'),
          b'\0\0\0\0' + png._chunk(b'IEND', b'')]


class _Layout:
  """A file of framed records from their payloads' pieces: the literals joined into one buffer
  (source 0), the segment table of `se3ds_assemble_segments`, and where the checksums go."""

  def __init__(self, payloads: Sequence[List[Piece]], max_segment: int):
    self.literals = bytearray()
    self.segments: List[Tuple[int, int, int, int]] = []
    self.idat: List[Tuple[int, int, int]] = []       # type field at, bytes of type + data, CRC at
    self.frames: List[Tuple[int, int]] = []          # record at, payload bytes
    self._max = max_segment
    pos = 0
    for pieces in payloads:
      n = _size(pieces)
      self.frames.append((pos, n))
      pos = self._place([struct.pack('<Q', n) + b'\0\0\0\0'] + list(pieces) + [b'\0\0\0\0'], pos)
    self.total = pos

  def _segment(self, source, at, to, length):
    while length > 0:
      part = min(length, self._max)
      self.segments.append((source, at, to, part))
      at, to, length = at + part, to + part, length - part

  def _place(self, pieces, pos):
    run_at, run_to, idat_at = len(self.literals), pos, None
    for p in pieces:
      if isinstance(p, bytes):
        self.literals += p
        pos += len(p)
        continue
      if isinstance(p, _Ref):
        self._segment(0, run_at, run_to, len(self.literals) - run_at)   # the literal run in front
        self._segment(1, p.offset, pos, p.length)
        pos += p.length
        run_at, run_to = len(self.literals), pos
      elif p.kind == 'idat':
        idat_at = pos
      else:
        self.idat.append((idat_at, pos - idat_at, pos))
    self._segment(0, run_at, run_to, len(self.literals) - run_at)
    return pos


def encode_records_host(examples: Sequence[dict]) -> bytes:
  """The record file of `examples` built in Python: each a dict of the plane names of IMAGE_PLANES ->
  encoded PNG file, plus optional scan_id, filename, depth_scale, dataset_type, bbox
  (`example_features`).  The layout is the one R2RRecordWriter assembles on the device; both CRC-32C
  are the Python loop's.  Equal to `frame_record(encode_example(example_features(e)))` joined."""
  out = bytearray()
  for e in examples:
    layout = _Layout([_example_pieces({k: [bytes(v)] if k in IMAGE_PLANES else v
                                       for k, v in e.items()})], 1 << 62)
    rec = bytearray(layout.literals)   # one literal run: no references
    n = layout.frames[0][1]
    rec[8:12] = struct.pack('<I', mask_crc(crc32c(bytes(rec[:8]))))
    rec[12 + n:] = struct.pack('<I', mask_crc(crc32c(bytes(rec[12:12 + n]))))
    out += rec
  return bytes(out)


# ------------------------------------------------------------------------------ device planes
def record_planes(proj_rgb: Optional[torch.Tensor] = None, proj_depth: Optional[torch.Tensor] = None,
                  proj_mask: Optional[torch.Tensor] = None):
  """fp32 results of the warp -> the planes a record stores (`se3ds_record_planes`), any subset:
  proj_rgb (..., 3) with void class -1 -> uint8 (truncated, saturated; void, negative, NaN -> 0);
  proj_depth (...) in [0, 1] -> int16 bit patterns of uint16 = floor(d * 65535 + 0.5) in binary64,
  saturated, NaN -> 0 (also for a float target depth); proj_mask (...) -> uint8, 255 where it is 1.
  Returns the given ones in this order (one tensor if only one was given)."""
  given = [t for t in (proj_rgb, proj_depth, proj_mask) if t is not None]
  if not given:
    raise ValueError('record_planes: nothing to convert')
  _lib.require_cuda(*given)
  dev = given[0].device
  pixels = None
  for t, last in ((proj_rgb, 3), (proj_depth, None), (proj_mask, None)):
    if t is None:
      continue
    if t.dtype != torch.float32 or t.device != dev or (last and (t.dim() < 1 or t.shape[-1] != last)):
      raise ValueError(f'record_planes: float32 tensors on one device, RGB (..., 3); got {t.dtype} '
                       f'{tuple(t.shape)} on {t.device}')
    count = t.numel() // (last or 1)
    if pixels is not None and count != pixels:
      raise ValueError(f'record_planes: planes of {pixels} and {count} pixels')
    pixels = count
  c = lambda t: None if t is None else t.contiguous()
  proj_rgb, proj_depth, proj_mask = c(proj_rgb), c(proj_depth), c(proj_mask)
  e = lambda t, dt: None if t is None else torch.empty(t.shape, dtype=dt, device=dev)
  rgb, depth, mask = e(proj_rgb, torch.uint8), e(proj_depth, torch.int16), e(proj_mask, torch.uint8)
  with torch.cuda.device(dev):
    rc = _lib.lib().se3ds_record_planes(_lib.ptr(proj_rgb), _lib.ptr(proj_depth), _lib.ptr(proj_mask),
                                        pixels, _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(mask),
                                        _lib.stream())
  _lib.check(rc, 'se3ds_record_planes')
  out = [t for t in (rgb, depth, mask) if t is not None]
  return out[0] if len(out) == 1 else tuple(out)


def guidance_planes(prev_rgb: torch.Tensor, prev_depth: torch.Tensor, prev_position: torch.Tensor,
                    position: torch.Tensor, depth_scale: float, mask_blurred: bool = True
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """The stored guidance planes (proj/encoded uint8 (N,H,W,3), proj/depth int16 bit patterns
  (N,H,W), proj/mask uint8 (N,H,W)) of examples whose target is seen from `position` (N,3), given the
  previous panorama prev_rgb (N,H,W,3) uint8 or int32, its depth prev_depth (N,H,W) fp32 in [0,1]
  and its position (N,3).

  The reference's preprocessing, which made the proj/* planes of the published records, is
  unpublished.  This definition is the project's own: the guidance the generator sees at inference.
  It runs the calls of `SE3DSModel.add_to_memory` and `__call__` (models/models.py:180-293) on a
  memory of one observation -- `mask_pano` (with mask_blurred: rows outside [H / 8, H - H / 8] become void and
  never enter the warp), `equirectangular_to_pointcloud(..., 'bilinear', prev_position)`,
  `compact_valid_points`, `project_feats_to_equirectangular(offset=position, with_mask=True)` -- and
  then the planes kernel.  No model and no weights are constructed."""
  from se3ds_amd.models.models import _quantize
  from se3ds_amd.utils import pano_utils, point_cloud_utils
  _lib.require_cuda(prev_rgb, prev_depth, prev_position, position)
  if prev_rgb.dtype not in (torch.uint8, torch.int32):
    raise ValueError(f'guidance_planes: prev_rgb uint8 or int32, got {prev_rgb.dtype}')
  n, h, w, _ = prev_rgb.shape
  void = constants.INVALID_RGB_VALUE
  if prev_rgb.dtype != torch.int32:
    prev_rgb = _quantize(prev_rgb, torch.int32, lo=0, hi=255)
  if mask_blurred:
    prev_rgb = pano_utils.mask_pano(prev_rgb, masked_region_value=void)
  xyz1, feats = pano_utils.equirectangular_to_pointcloud(
      prev_rgb, prev_depth, void, depth_scale, interpolation_method='bilinear',
      position=prev_position.to(torch.float32))
  f_xyz1, f_rgb = pano_utils.compact_valid_points(xyz1, feats, void)
  f_rgb = f_rgb.to(torch.int32)
  point_cloud_utils.propagate_int_range(f_rgb, prev_rgb, extra=(void,))
  proj_depth, proj_rgb, proj_mask = pano_utils.project_feats_to_equirectangular(
      f_rgb, f_xyz1, h, w, void, depth_scale, offset=position.to(torch.float32), with_mask=True,
      mask_void=void)
  return record_planes(proj_rgb, proj_depth, proj_mask)


def assemble_segments(sources: Sequence[torch.Tensor], segments, out: torch.Tensor) -> None:
  """`se3ds_assemble_segments` on its own: copies rows (source index, source offset, destination
  offset, length) of `segments` from the uint8 device tensors `sources` into the uint8 device tensor
  `out`, on the current stream.  Destinations ascend and are disjoint; a range longer than one
  workgroup's share is split here.  The writer's flush uploads its table with the literals instead."""
  _lib.require_cuda(out, *sources)
  L = _lib.lib()
  limit = int(L.se3ds_assemble_max_segment_bytes())
  rows = []
  for which, at, to, length in np.asarray(segments, np.int64).reshape(-1, 4).tolist():
    rows.append((which, at, to, min(length, limit)))   # (a bad length stays one row: the library rejects it)
    while length > limit:
      at, to, length = at + limit, to + limit, length - limit
      rows.append((which, at, to, min(length, limit)))
  table = np.array(rows, np.int64).reshape(-1, 4)
  for t in tuple(sources) + (out,):
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.device != out.device:
      raise ValueError('assemble_segments takes contiguous torch.uint8 tensors on one device')
  src = np.array([[t.data_ptr(), t.numel()] for t in sources], np.int64).reshape(-1, 2)
  with torch.cuda.device(out.device):
    table_dev = torch.from_numpy(table).to(out.device)
    _lib.check(L.se3ds_assemble_segments(src.ctypes.data, len(src), _lib.ptr(table_dev), table.ctypes.data,
                                         len(table), out.data_ptr(), out.numel(), _lib.stream()),
               'se3ds_assemble_segments')


def patch_crc(out: torch.Tensor, crcs: torch.Tensor, patches) -> None:
  """`se3ds_patch_crc` on its own: rows (index into `crcs`, byte offset in `out`, form) of `patches`;
  form 0 writes crcs[index] big-endian, form 1 TFRecord's masked form little-endian.  crcs: int32 or
  uint32 device tensor (the results of utils.crc32c's kernels), out: uint8 device tensor."""
  _lib.require_cuda(out, crcs)
  if out.dtype != torch.uint8 or crcs.element_size() != 4 or not out.is_contiguous() or \
      not crcs.is_contiguous():
    raise ValueError('patch_crc takes a contiguous uint8 buffer and 32-bit CRC words')
  table = np.ascontiguousarray(np.asarray(patches, np.int64).reshape(-1, 3))
  with torch.cuda.device(out.device):
    table_dev = torch.from_numpy(table).to(out.device)
    _lib.check(_lib.lib().se3ds_patch_crc(crcs.data_ptr(), crcs.numel(), _lib.ptr(table_dev),
                                          table.ctypes.data, len(table), out.data_ptr(), out.numel(),
                                          _lib.stream()), 'se3ds_patch_crc')


# ------------------------------------------------------------------------------ the writer
class R2RRecordWriter:
  """Context manager that writes training Examples to `path` (a `train*.tfrecord` file of
  `R2RImageDataset`), encoded and assembled on `device`.  `add` queues an example; every
  `examples_per_flush` of them, and the rest on exit, are flushed as the module text describes: two
  synchronisations per flush.  filters: as `png.encode_png_batch` (one value for all planes).  The
  file is written as `<path>.tmp` and renamed on a clean exit; on an error the temporary file is
  removed and nothing is left under `path`; a writer that is dropped without `close`, `abort` or a
  `with` block aborts when it is collected.  `timings` (profile=True only: every group of launches is
  then followed by a synchronisation) holds one dict of host-clock seconds per flush."""

  def __init__(self, path: str, device, filters='adaptive', examples_per_flush: int = 8,
               profile: bool = False):
    dev = cuda_device(device, 'R2RRecordWriter', 'encodes')
    if examples_per_flush < 1:
      raise ValueError(f'examples_per_flush {examples_per_flush}')
    self.path, self.device, self.examples_per_flush = path, dev, int(examples_per_flush)
    self._mode = png._filter_mode(filters)
    self._pending: List[dict] = []
    self._profile = profile
    self.timings: List[Dict[str, float]] = []
    self.examples = 0
    self.bytes_written = 0
    self._tmp = path + '.tmp'
    self._file = open(self._tmp, 'wb')

  def __enter__(self):
    return self

  def __exit__(self, exc_type, exc, tb):
    if exc_type is None:
      self.close()
    else:
      self.abort()
    return False

  def __del__(self):
    try:
      self.abort()
    except Exception:   # noqa: BLE001  (interpreter teardown: modules may be gone)
      pass

  def abort(self):
    """Drops what is pending and removes the temporary file."""
    self._pending = []
    if getattr(self, '_file', None) is not None:
      self._file.close()
      self._file = None
      if os.path.exists(self._tmp):
        os.remove(self._tmp)

  def close(self):
    """Flushes what is pending and renames the temporary file to `path`."""
    if self._file is None:
      return
    try:
      self.flush()
      self._file.close()
      self._file = None
      os.replace(self._tmp, self.path)
    except BaseException:
      self.abort()
      raise

  def add(self, image, depth, proj_image, proj_depth, proj_mask, blurred_mask=None, segmentation=None,
          scan_id: bytes = b'', filename: bytes = b'', depth_scale: float = 10.0, dataset_type: int = 0,
          bbox=(0, 0, 0, 0)):
    """Queues one example: device tensors in the raw dtypes of RAW_DTYPES -- image / proj_image uint8
    (H,W,3); depth / proj_depth int16 bit patterns of uint16 (H,W); proj_mask / blurred_mask /
    segmentation uint8 (H,W).  An absent blurred_mask or segmentation is zeros.  `image` may also be
    `bytes` holding a baseline JPEG file (utils/jpeg.py): its header is parsed here (ValueError unless
    it decodes to (H,W,3) with depth's H, W) and the pixels are decoded at the flush, all pending
    JPEGs in one `decode_jpeg_batch`, in front of the plane encode.  The tensors are
    copied into row-major order, so views of any strides (a permuted CHW image, a transposed plane)
    are taken as they index and the caller may reuse them.  The features written are those `R2RImageDataset._parse`
    reads (reference :149-178), under the names of IMAGE_PLANES."""
    if self._file is None:
      raise ValueError('R2RRecordWriter: the writer is closed')
    planes = dict(image=image, depth=depth, proj_image=proj_image, proj_depth=proj_depth,
                  proj_mask=proj_mask, blurred_mask=blurred_mask, segmentation=segmentation)
    scan = None
    if isinstance(image, (bytes, bytearray, memoryview)):
      # a JPEG file: the header is read now, the pixels are decoded with the flush's other JPEGs
      scan = jpeg.parse_jpeg(bytes(image))
      del planes['image']
    _lib.require_cuda(*planes.values())
    h, w = int(proj_mask.shape[0]), int(proj_mask.shape[1])
    stored = {'image': scan} if scan is not None else {}
    for name, t in planes.items():
      channels = IMAGE_PLANES[name][1]
      if t is None:
        stored[name] = torch.zeros((h, w, 1), dtype=RAW_DTYPES[name], device=self.device)
        continue
      if t.dtype != RAW_DTYPES[name] or t.device != self.device:
        raise ValueError(f'{name}: expected {RAW_DTYPES[name]} on {self.device}, got {t.dtype} on '
                         f'{t.device}')
      if tuple(t.shape) not in ((h, w, channels),) + (((h, w),) if channels == 1 else ()):
        raise ValueError(f'{name}: shape {tuple(t.shape)}, expected {(h, w, channels)}')
      # a dense copy in row-major order, whatever the strides of what came in: the encoder reads
      # height x row_bytes bytes from the pointer
      stored[name] = t.reshape(h, w, channels).clone(memory_format=torch.contiguous_format)
    if scan is not None and (scan.height, scan.width, scan.components) != (h, w, 3):   # (depth is (h, w))
      raise ValueError(f'image: a JPEG that decodes to {(scan.height, scan.width, scan.components)}, '
                       f'expected {(h, w, 3)}')
    self._pending.append(dict(planes=stored, scan_id=bytes(scan_id), filename=bytes(filename),
                              depth_scale=float(depth_scale), dataset_type=int(dataset_type),
                              bbox=tuple(float(b) for b in bbox)))
    if len(self._pending) >= self.examples_per_flush:
      self.flush()

  def flush(self):
    """Encodes, assembles, checksums and writes the pending examples.  Images that came as JPEG files
    are decoded first; if one of them does not decode, ValueError names it (its index among the pending
    JPEGs), nothing is written and the pending examples stay queued."""
    if not self._pending:
      return
    dev = self.device
    decode_seconds = 0.0
    encoded = [e for e in self._pending if isinstance(e['planes']['image'], jpeg.JpegScan)]
    if encoded:
      # 0: all in one decode, in front of taking the examples over (its status check synchronises)
      t0 = time.perf_counter()
      decoded = jpeg.decode_jpeg_batch([e['planes']['image'] for e in encoded], dev, channels=3)
      for e, pixels in zip(encoded, decoded):
        e['planes']['image'] = pixels
      decode_seconds = time.perf_counter() - t0
    pending, self._pending = self._pending, []
    L = _lib.lib()
    clock = {'jpeg_decode': decode_seconds} if encoded else {}
    t0 = time.perf_counter()

    def lap(name):
      nonlocal t0
      if self._profile:
        torch.cuda.current_stream().synchronize()
        now = time.perf_counter()
        clock[name] = clock.get(name, 0.0) + now - t0
        t0 = now

    with torch.cuda.device(dev):
      # 1-2: every plane of every example in one encode; the sizes come back
      tensors = [e['planes'][name] for e in pending for name in _PLANE_ORDER]
      # (the planes include 16-bit depth, so launch_encode takes se3ds_png_encode_planes, always)
      table, result, head = png.launch_encode(tensors, [self._mode] * len(tensors))
      sizes = result[:8 * len(tensors)].cpu().numpy().view(np.uint32).reshape(-1, 2)   # waits
      lap('encode')
      # 3: the layout, from sizes alone
      payloads, k = [], 0
      for e in pending:
        example = {key: value for key, value in e.items() if key != 'planes'}
        for name in _PLANE_ORDER:
          row = table[k]
          example[name] = _png_pieces(int(row[1]), int(row[2]), int(row[3]), int(row[6]),
                                      int(sizes[k, 0]), int(sizes[k, 1]))
          k += 1
        payloads.append(_example_pieces(example))
      layout = _Layout(payloads, int(L.se3ds_assemble_max_segment_bytes()))
      seg = np.array(layout.segments, np.int64).reshape(-1, 4)
      idat = np.array(layout.idat, np.int64).reshape(-1, 3)
      n_idat, n_rec = len(idat), len(layout.frames)
      crcz_table = np.ascontiguousarray(np.stack([idat[:, 0], idat[:, 1], np.zeros(n_idat, np.int64)], 1))
      patchz_table = np.ascontiguousarray(np.stack([np.arange(n_idat), idat[:, 2],
                                                    np.zeros(n_idat, np.int64)], 1).astype(np.int64))
      frames = np.array(layout.frames, np.int64).reshape(-1, 2)
      crcc_table = np.zeros((2 * n_rec, 2), np.int64)       # the 8 length bytes, the payload
      crcc_table[0::2] = np.stack([frames[:, 0], np.full(n_rec, 8)], 1)
      crcc_table[1::2] = np.stack([frames[:, 0] + 12, frames[:, 1]], 1)
      patchc_table = np.zeros((2 * n_rec, 3), np.int64)
      patchc_table[:, 0] = np.arange(2 * n_rec)
      patchc_table[0::2, 1] = frames[:, 0] + 8
      patchc_table[1::2, 1] = frames[:, 0] + 12 + frames[:, 1]
      patchc_table[:, 2] = 1
      # one upload: the literals, then the five tables, each 16-byte aligned
      uploaded, offsets = upload([layout.literals, seg, crcz_table, patchz_table, crcc_table,
                                  patchc_table], dev)
      base = uploaded.data_ptr()
      out = torch.empty((layout.total,), dtype=torch.uint8, device=dev)
      crcs = torch.empty((max(n_idat, 2 * n_rec),), dtype=torch.int32, device=dev)
      stream = _lib.stream()
      lap('layout_upload')
      # 4: assemble
      sources = np.array([[base, len(layout.literals)],
                          [result.data_ptr() + head, result.numel() - head]], np.int64)
      _lib.check(L.se3ds_assemble_segments(sources.ctypes.data, 2, base + offsets[1], seg.ctypes.data,
                                           len(seg), out.data_ptr(), layout.total, stream),
                 'se3ds_assemble_segments')
      lap('assemble')
      # 5-6: the IDAT chunks' CRC-32 over type + data, patched in big-endian
      ws_bytes = max(int(L.se3ds_crc32z_workspace_bytes(int(idat[:, 1].sum()), n_idat)),
                     int(L.se3ds_crc32c_workspace_bytes(int(crcc_table[:, 1].sum()), 2 * n_rec)))
      ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
      _lib.check(L.se3ds_crc32z_multi(out.data_ptr(), layout.total, base + offsets[2],
                                      crcz_table.ctypes.data, n_idat, crcs.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream), 'se3ds_crc32z_multi')
      _lib.check(L.se3ds_patch_crc(crcs.data_ptr(), n_idat, base + offsets[3], patchz_table.ctypes.data,
                                   n_idat, out.data_ptr(), layout.total, stream), 'se3ds_patch_crc')
      lap('idat_crc')
      # 7-8: the records' CRC-32C, patched in masked
      _lib.check(L.se3ds_crc32c_multi(out.data_ptr(), layout.total, base + offsets[4],
                                      crcc_table.ctypes.data, 2 * n_rec, crcs.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream), 'se3ds_crc32c_multi')
      _lib.check(L.se3ds_patch_crc(crcs.data_ptr(), 2 * n_rec, base + offsets[5],
                                   patchc_table.ctypes.data, 2 * n_rec, out.data_ptr(), layout.total,
                                   stream), 'se3ds_patch_crc')
      lap('record_crc')
      # 9: the finished bytes
      done = Readback(out).wait()
      if self._profile:
        now = time.perf_counter()
        clock['download'] = now - t0
        t0 = now
    self._file.write(done.data)
    if self._profile:
      clock['file_write'] = time.perf_counter() - t0
      self.timings.append(clock)
    self.examples += len(pending)
    self.bytes_written += layout.total


# --------------------------------------------------------------------------- trajectories
def encode_trajectory_example(arrays: Dict[str, np.ndarray]) -> bytes:
  """A serialized evaluation Example for `R2RVideoDataset._parse` (reference :626-719) from the
  arrays that method yields: image fp32 (T,H,W,3), position fp32 (T,4), mask fp32 (T,),
  segmentation uint8 and depth fp32 (T,H,W); optional pathdreamer_segmentation (stored as int32, as
  the published records hold it), pathdreamer_depth, id, scan_id, dataset_type, depth_scale.  The
  planes are serialized tensors, so nothing is encoded on the device; a file of such records is
  written with `tf_records.write_records(path, records, checksums='device')`."""
  image = np.asarray(arrays['image'], np.float32)
  feats = {'id': np.array([int(arrays.get('id', 0))], np.int64),
           'video/num_frames': np.array([image.shape[0]], np.int64),
           'scan_id': bytes(arrays.get('scan_id', b'')),
           'video/rgb': tf_records.serialize_tensor(image),
           'video/position': tf_records.serialize_tensor(np.asarray(arrays['position'], np.float32)),
           'video/mask': tf_records.serialize_tensor(np.asarray(arrays['mask'], np.float32)),
           'video/segmentations': tf_records.serialize_tensor(np.asarray(arrays['segmentation'], np.uint8)),
           'video/depth': tf_records.serialize_tensor(np.asarray(arrays['depth'], np.float32))}
  if arrays.get('pathdreamer_segmentation') is not None:
    feats['video/pathdreamer_segmentations'] = tf_records.serialize_tensor(
        np.asarray(arrays['pathdreamer_segmentation']).astype(np.int32))
  if arrays.get('pathdreamer_depth') is not None:
    feats['video/pathdreamer_depth'] = tf_records.serialize_tensor(
        np.asarray(arrays['pathdreamer_depth'], np.float32))
  if 'dataset_type' in arrays:
    feats['dataset_type'] = np.array([int(arrays['dataset_type'])], np.int64)
  if 'depth_scale' in arrays:
    feats['depth_scale'] = np.array([arrays['depth_scale']], np.float32)
  return tf_records.encode_example(feats)
