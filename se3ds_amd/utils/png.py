"""PNG decoding without an imaging package: the container on the host, the reconstruction
(un-filtering) of every plane of a batch on the device in one launch (`se3ds_png_unfilter`,
csrc/png.hip), and the zlib inflate between them either on the host (the default: `zlib` on a small
thread pool) or, with inflate='device', on the device as well (`se3ds_png_inflate`,
csrc/inflate.hip, one wavefront per plane in front of the reconstruction).  This is
tf.image.decode_png as the reference's `R2RImageDataset._parse` uses it
(datasets/indoor_datasets.py:185-228): 8-bit RGB, 8-bit grey and 16-bit grey, non-interlaced.
Written from the PNG specification (ISO/IEC 15948, sections 5, 9, 11).  There is no CPU fallback for
the reconstruction, and none for the device inflate."""
import concurrent.futures
import enum
import struct
import zlib
from typing import Dict, List, NamedTuple, Sequence, Tuple, Union

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd.utils._staging import Readback, aligned, cuda_device, layout, upload

SIGNATURE = b'\x89PNG\r\n\x1a\n'
MAX_THREADS = 16
_COLOUR_KINDS = {0: 'greyscale', 2: 'truecolour', 3: 'palette', 4: 'greyscale with alpha',
                 6: 'truecolour with alpha'}
_VALID_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


class PngPlane(NamedTuple):
  """A parsed and inflated, not yet reconstructed PNG: `filtered` holds height scan lines of one
  filter-type byte + width * channels * bit_depth / 8 filtered bytes."""
  height: int
  width: int
  bit_depth: int
  channels: int
  filtered: bytes

  @property
  def bytes_per_pixel(self):
    return self.channels * self.bit_depth // 8

  @property
  def row_bytes(self):
    return self.width * self.bytes_per_pixel


class PngStream(NamedTuple):
  """A parsed, NOT inflated PNG: `compressed` is the zlib stream of the joined IDAT chunks, which
  inflates to height scan lines of one filter-type byte + row_bytes filtered bytes."""
  height: int
  width: int
  bit_depth: int
  channels: int
  compressed: bytes

  @property
  def bytes_per_pixel(self):
    return self.channels * self.bit_depth // 8

  @property
  def row_bytes(self):
    return self.width * self.bytes_per_pixel


def _walk(buf: bytes) -> Tuple[int, int, int, int, bytes]:
  """The container half of parse_png and parse_png_container: signature, chunk walk with CRC check,
  IHDR and kind checks -> height, width, bit depth, channels, the joined IDAT chunks."""
  buf = bytes(buf)
  if buf[:8] != SIGNATURE:
    raise ValueError('not a PNG: bad signature')
  pos, ihdr, idat, ended = 8, None, [], False
  while pos < len(buf):
    if len(buf) - pos < 12:
      raise ValueError(f'PNG: truncated chunk header at offset {pos}')
    length, = struct.unpack_from('>I', buf, pos)
    tag = buf[pos + 4:pos + 8]
    if len(buf) - pos - 12 < length:
      raise ValueError(f'PNG: truncated {tag!r} chunk at offset {pos}')
    data = buf[pos + 8:pos + 8 + length]
    crc, = struct.unpack_from('>I', buf, pos + 8 + length)
    if zlib.crc32(tag + data) != crc:
      raise ValueError(f'PNG: CRC mismatch in the {tag!r} chunk at offset {pos}')
    pos += 12 + length
    if ihdr is None and tag != b'IHDR':
      raise ValueError(f'PNG: first chunk is {tag!r}, not IHDR')
    if tag == b'IHDR':
      if ihdr is not None or length != 13:
        raise ValueError('PNG: bad IHDR')
      ihdr = struct.unpack('>IIBBBBB', data)
    elif tag == b'IDAT':
      idat.append(data)
    elif tag == b'IEND':
      ended = True
      break
    elif not tag[0] & 0x20:   # an upper-case first letter marks a critical chunk
      if tag == b'PLTE':
        continue              # the colour type decides below
      raise ValueError(f'PNG: unknown critical chunk {tag!r}')
  if ihdr is None:
    raise ValueError('PNG: no IHDR chunk')
  if not ended:
    raise ValueError('PNG: no IEND chunk')
  width, height, depth, colour, compression, filter_method, interlace = ihdr
  if width == 0 or height == 0:
    raise ValueError(f'PNG: {width} x {height} image')
  if colour not in _COLOUR_KINDS or depth not in _VALID_DEPTHS[colour]:
    raise ValueError(f'PNG: colour type {colour} at bit depth {depth} is not a PNG kind')
  if compression != 0 or filter_method != 0 or interlace not in (0, 1):
    raise ValueError(f'PNG: compression {compression}, filter method {filter_method}, '
                     f'interlace {interlace}')
  kind = f'{_COLOUR_KINDS[colour]} at bit depth {depth}'
  if interlace:
    raise NotImplementedError(f'PNG kind not supported: interlaced (Adam7) {kind}')
  if (colour, depth) not in ((0, 8), (0, 16), (2, 8)):
    raise NotImplementedError(f'PNG kind not supported: {kind}')
  if not idat:
    raise ValueError('PNG: no IDAT chunk')
  return height, width, depth, 3 if colour == 2 else 1, b''.join(idat)


def parse_png_container(buf: bytes) -> PngStream:
  """parse_png without the inflate: the same chunk walk, CRC and kind checks with the same
  messages.  What the stream inflates to is checked where it is inflated: on the device, by
  decode_png_batch(..., inflate='device')."""
  return PngStream(*_walk(buf))


def parse_png(buf: bytes) -> PngPlane:
  """Signature, chunk walk with CRC check, IHDR, the concatenated IDAT chunks inflated.  Supported:
  colour type 0 at bit depth 8 or 16 and colour type 2 at bit depth 8, non-interlaced; any other
  legal kind raises NotImplementedError naming it, every malformed input ValueError -- including a
  filter-type byte above 4, so that the kernel never sees one."""
  height, width, depth, channels, compressed = _walk(buf)
  row_bytes = width * channels * depth // 8
  try:
    filtered = zlib.decompress(compressed)
  except zlib.error as e:
    raise ValueError(f'PNG: the IDAT stream does not inflate: {e}') from None
  if len(filtered) != height * (1 + row_bytes):
    raise ValueError(f'PNG: {len(filtered)} inflated bytes, {height} x (1 + {row_bytes}) expected')
  types = np.frombuffer(filtered, np.uint8)[::1 + row_bytes]
  if int(types.max()) > 4:
    raise ValueError(f'PNG: filter type {int(types.max())} in row {int(np.argmax(types > 4))}')
  return PngPlane(height, width, depth, channels, filtered)


def _as_plane(item: Union[bytes, PngPlane]) -> PngPlane:
  return item if isinstance(item, PngPlane) else parse_png(item)


def _plan(bufs_by_key, dev, parse):
  """The front both decoders share: -> (out, rows).  `parse` turns the items of all keys, in key
  order, into PngPlanes or PngStreams; geometry is checked within each key; out[key] is allocated on
  `dev`; rows holds (key, index within the key, parsed item, address of its plane in out[key])."""
  if not bufs_by_key or any(len(v) == 0 for v in bufs_by_key.values()):
    raise ValueError('decode_png_batch: nothing to decode')
  items = parse([item for bufs in bufs_by_key.values() for item in bufs])
  out, rows = {}, []
  for k, bufs in bufs_by_key.items():
    group = items[len(rows):len(rows) + len(bufs)]
    p0 = group[0]
    for p in group:
      if p[:4] != p0[:4]:
        raise ValueError(f'{k}: a {p.height}x{p.width} PNG of {p.channels} channels at bit depth '
                         f'{p.bit_depth} in a batch of {p0.height}x{p0.width}, {p0.channels}, '
                         f'{p0.bit_depth}')
    shape = (len(group), p0.height, p0.width) + ((3,) if p0.channels == 3 else ())
    out[k] = torch.empty(shape, dtype=torch.int16 if p0.bit_depth == 16 else torch.uint8, device=dev)
    plane_bytes = p0.height * p0.row_bytes
    rows += [(k, i, p, out[k].data_ptr() + i * plane_bytes) for i, p in enumerate(group)]
  return out, rows


def decode_png_batch(bufs_by_key: Dict[str, Sequence[Union[bytes, PngPlane, PngStream]]], device,
                     threads: int = 4, inflate: str = 'host') -> Dict[str, torch.Tensor]:
  """{key: the N PNGs of one plane of a batch} -> {key: CUDA tensor}: uint8 (N,H,W,3) for RGB,
  uint8 (N,H,W) for 8-bit grey, 16-bit grey values as int16 (N,H,W) bit patterns (the convention of
  datasets.indoor_datasets.RAW_DTYPES).  An item is an encoded PNG, or a PngPlane that parse_png
  already made.  Geometry is equal within a key (ValueError otherwise).

  inflate='device': the IDAT streams are inflated on the device too -- decode_png_batch_async
  followed by its wait; an item is then an encoded PNG or a PngStream, and a stream that does not
  inflate raises ValueError naming key, index within the key and reason.  The rest of this text is
  the default, inflate='host'.

  Encoded items are parsed and inflated on a thread pool of `threads` workers (zlib releases the
  GIL); `threads` is capped at 16.  The descriptor table and all filtered streams go into one pinned
  host buffer, one asynchronous copy on the current stream takes it to the device, and one launch
  reconstructs every plane of every key.  A non-CUDA device raises Se3dsHipError."""
  if check_inflate_mode(inflate) == 'device':
    out, pending = decode_png_batch_async(bufs_by_key, device)
    pending.check()
    return out
  dev = cuda_device(device, 'decode_png_batch', 'reconstructs')
  threads = max(1, min(int(threads), MAX_THREADS))

  def parse(flat):
    if all(isinstance(item, PngPlane) for item in flat):
      return flat
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
      return list(pool.map(_as_plane, flat))

  out, rows = _plan(bufs_by_key, dev, parse)
  L = _lib.lib()
  table = np.zeros((len(rows), L.se3ds_png_unfilter_fields()), np.int64)
  # the device buffer starts with the table, and the table's offsets count from its base
  offsets, _ = layout([table.nbytes] + [len(p.filtered) for _, _, p, _ in rows])
  for i, (_, _, p, to) in enumerate(rows):
    table[i] = (offsets[1 + i], to, p.height, p.row_bytes, p.bytes_per_pixel, int(p.bit_depth == 16))
  with torch.cuda.device(dev):
    device_buf, _ = upload([table] + [p.filtered for _, _, p, _ in rows], dev)
    rc = L.se3ds_png_unfilter(_lib.ptr(device_buf), device_buf.numel(), _lib.ptr(device_buf),
                              table.ctypes.data, len(rows), _lib.stream())
    _lib.check(rc, 'se3ds_png_unfilter')
  return out


# ------------------------------------------------------------------------------ device inflate
class InflateStatus(enum.IntEnum):
  """The status word's low byte (csrc/inflate_core.h, enum class Status: the same names)."""
  OK = 0
  TRUNCATED = 1
  BAD_HEADER = 2
  BAD_BLOCK_TYPE = 3
  BAD_STORED_LENGTH = 4
  BAD_COUNTS = 5
  OVER_SUBSCRIBED = 6
  INCOMPLETE = 7
  BAD_REPEAT = 8
  NO_END_OF_BLOCK = 9
  BAD_CODE = 10
  BAD_DISTANCE = 11
  TOO_LONG = 12
  TOO_SHORT = 13
  BAD_ADLER = 14
  BAD_FILTER = 15


_INFLATE_REASONS = {
    InflateStatus.TRUNCATED: 'incomplete or truncated stream',
    InflateStatus.BAD_HEADER: 'incorrect zlib header',
    InflateStatus.BAD_BLOCK_TYPE: 'invalid block type',
    InflateStatus.BAD_STORED_LENGTH: 'invalid stored block lengths',
    InflateStatus.BAD_COUNTS: 'too many length or distance symbols',
    InflateStatus.OVER_SUBSCRIBED: 'over-subscribed set of code lengths',
    InflateStatus.INCOMPLETE: 'incomplete set of code lengths',
    InflateStatus.BAD_REPEAT: 'invalid bit length repeat',
    InflateStatus.NO_END_OF_BLOCK: 'missing end-of-block code',
    InflateStatus.BAD_CODE: 'invalid literal/length or distance code',
    InflateStatus.BAD_DISTANCE: 'distance beyond the start of the output',
    InflateStatus.BAD_ADLER: 'incorrect data check',
}


def check_inflate_mode(inflate: str) -> str:
  if inflate not in ('host', 'device'):
    raise ValueError(f"inflate: 'host' or 'device', got {inflate!r}")
  return inflate


def inflate_failure(word: int, stream: PngStream) -> str:
  """The message of a non-zero status word of se3ds_png_inflate for `stream`."""
  code = InflateStatus(word & 0xff)
  if code in _INFLATE_REASONS:
    return f'the IDAT stream does not inflate: {_INFLATE_REASONS[code]}'
  if code == InflateStatus.BAD_FILTER:
    return f'filter type {(word >> 8) & 0xff} in row {word >> 16}'
  more = 'more' if code == InflateStatus.TOO_LONG else 'fewer'
  return f'{more} inflated bytes than {stream.height} x (1 + {stream.row_bytes})'


class PendingDecode(Readback):
  """The device inflate of one batch in flight: `check()` waits for the status words and raises
  ValueError for the first plane that failed.  The output tensors are valid (and may be read on the
  stream the batch was launched on) only if check() returns."""

  def __init__(self, status: torch.Tensor, names: List[Tuple[str, int]], streams: List[PngStream]):
    super().__init__(status)   # the status words on the device: their copy and its event are queued
    self._names, self._streams = names, streams

  def check(self) -> None:
    words = self.wait()
    bad = np.flatnonzero(words)
    if bad.size:
      i = int(bad[0])
      key, index = self._names[i]
      raise ValueError(f'{key}[{index}]: {inflate_failure(int(words[i]), self._streams[i])}')


def _as_stream(item: Union[bytes, PngStream]) -> PngStream:
  if isinstance(item, PngStream):
    return item
  if isinstance(item, PngPlane):
    raise ValueError("a PngPlane is already inflated: decode it with inflate='host'")
  return parse_png_container(item)


def decode_png_batch_async(bufs_by_key: Dict[str, Sequence[Union[bytes, PngStream]]], device
                           ) -> Tuple[Dict[str, torch.Tensor], PendingDecode]:
  """decode_png_batch with the inflate on the device, without the wait: -> (out, pending).  An item
  is an encoded PNG or a PngStream of parse_png_container.  Both descriptor tables and all
  compressed streams go into one pinned host buffer and one asynchronous copy; then, on the current
  stream, `se3ds_png_inflate` (one wavefront per plane) writes the filtered scan lines into a device
  workspace, `se3ds_png_unfilter` reconstructs from it, and the status words are copied back with an
  event behind them.  `pending.check()` waits on that event and raises ValueError naming key, index
  within the key and reason for the first plane whose stream did not inflate to its geometry; `out`
  counts only once it has returned.  A non-CUDA device raises Se3dsHipError."""
  dev = cuda_device(device, 'decode_png_batch', 'inflates and reconstructs')
  out, rows = _plan(bufs_by_key, dev, lambda flat: [_as_stream(item) for item in flat])
  streams = [p for _, _, p, _ in rows]

  L = _lib.lib()
  n = len(rows)
  inflate_table = np.zeros((n, L.se3ds_png_inflate_fields()), np.int64)
  unfilter_table = np.zeros((n, L.se3ds_png_unfilter_fields()), np.int64)
  unfilter_at = inflate_table.nbytes               # the device buffer starts with the inflate table,
  offsets, _ = layout([unfilter_at + unfilter_table.nbytes] +      # then the other, then the
                      [len(p.compressed) for p in streams])        # streams
  inflated = [p.height * (1 + p.row_bytes) for p in streams]
  workspace_at, workspace_bytes = layout(inflated)   # 16-byte aligned: the flush stores 16 bytes a lane
  for i, (_, _, p, to) in enumerate(rows):
    inflate_table[i] = (offsets[1 + i], len(p.compressed), workspace_at[i], inflated[i], 1 + p.row_bytes)
    unfilter_table[i] = (workspace_at[i], to, p.height, p.row_bytes, p.bytes_per_pixel,
                         int(p.bit_depth == 16))

  with torch.cuda.device(dev):
    tables = np.concatenate([inflate_table.reshape(-1), unfilter_table.reshape(-1)])
    device_buf, _ = upload([tables] + [p.compressed for p in streams], dev)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    rc = L.se3ds_png_inflate(_lib.ptr(device_buf), device_buf.numel(), _lib.ptr(workspace),
                             workspace_bytes, inflate_table.ctypes.data, n, _lib.ptr(status),
                             _lib.stream())
    _lib.check(rc, 'se3ds_png_inflate')
    rc = L.se3ds_png_unfilter(_lib.ptr(workspace), workspace_bytes, _lib.ptr(device_buf) + unfilter_at,
                              unfilter_table.ctypes.data, n, _lib.stream())
    _lib.check(rc, 'se3ds_png_unfilter')
    return out, PendingDecode(status, [(k, i) for k, i, _, _ in rows], streams)


# ------------------------------------------------------------------------------ encoding
ADAPTIVE = 5   # the filter field of se3ds_png_encode: 0..4 = that PNG filter type on every row
_FILTER_NAMES = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': ADAPTIVE}


def _filter_mode(f) -> int:
  mode = _FILTER_NAMES.get(f.lower()) if isinstance(f, str) else (int(f) if 0 <= int(f) <= 4 else None)
  if mode is None:
    raise ValueError(f"filters: 'adaptive', a PNG filter type 0..4 or its name, got {f!r}")
  return mode


def _filter_modes(filters, n: int) -> List[int]:
  if isinstance(filters, (list, tuple)):
    if len(filters) != n:
      raise ValueError(f'filters: {len(filters)} entries for {n} images')
    return [_filter_mode(f) for f in filters]
  return [_filter_mode(filters)] * n


def _chunk(tag: bytes, data: bytes) -> bytes:
  return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data))


def png_container(height: int, width: int, channels: int, zlib_stream: bytes, bit_depth: int = 8
                  ) -> bytes:
  """Signature, IHDR (8-bit grey or RGB, or 16-bit grey with bit_depth=16; non-interlaced), one IDAT
  chunk, IEND."""
  if bit_depth not in (8, 16) or (bit_depth == 16 and channels != 1):
    raise ValueError(f'png_container: {channels} channel(s) at bit depth {bit_depth}')
  ihdr = struct.pack('>IIBBBBB', width, height, bit_depth, 0 if channels == 1 else 2, 0, 0, 0)
  return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib_stream) + _chunk(b'IEND', b'')


def strip_rows(row_bytes: int) -> int:
  """Rows per strip of se3ds_png_encode: a strip's filtered bytes fit one stored block."""
  return max(1, 65535 // (1 + row_bytes))


def encode_table(pointers: Sequence[int], geometries: Sequence[Tuple[int, int, int]],
                 modes: Sequence[int]) -> np.ndarray:
  """The descriptor table of se3ds_png_encode (include/se3ds_hip.h) for images at device addresses
  `pointers` with (height, row_bytes, bytes per pixel) `geometries`: int64 (n, 8)."""
  table = np.zeros((len(pointers), 8), np.int64)
  strips = out = slots = 0
  for i, (p, (h, rb, bpp), mode) in enumerate(zip(pointers, geometries, modes)):
    table[i] = (p, h, rb, bpp, mode, strips, out, slots)
    per = strip_rows(rb)
    s = -(-h // per)
    strips += s
    out += 10 * s + h * (1 + rb)
    slots += s * ((10 + min(per, h) * (1 + rb) + 7) & ~7)
  return table


_SAMPLES_16 = tuple(t for t in (torch.int16, getattr(torch, 'uint16', None), np.dtype(np.uint16))
                    if t is not None)


def _is_16bit(dtype) -> bool:
  return dtype in _SAMPLES_16


def _check_pixels(shape, dtype, what):
  ok = len(shape) == 3 and shape[0] >= 1 and shape[1] >= 1
  if ok and _is_16bit(dtype):
    ok = shape[2] == 1
  elif ok:
    ok = dtype in (torch.uint8, np.dtype(np.uint8)) and shape[2] in (1, 3)
  if not ok:
    raise ValueError(f'{what}: uint8 (H,W,1) or (H,W,3), or 16-bit (H,W,1), expected, got {dtype} '
                     f'{tuple(shape)}')


def plane_geometry(x) -> Tuple[int, int, int]:
  """(height, row_bytes, field 3 of the encoder's table) of an (H,W,C) image: bytes per pixel 1 or
  3 for uint8, 2 for a 16-bit grey plane (se3ds_png_encode_planes)."""
  if _is_16bit(x.dtype):
    return int(x.shape[0]), 2 * int(x.shape[1]), 2
  return int(x.shape[0]), int(x.shape[1]) * int(x.shape[2]), int(x.shape[2])


def launch_encode(images: Sequence[torch.Tensor], modes: Sequence[int], fill: int = None
                  ) -> Tuple[np.ndarray, torch.Tensor, int]:
  """Queues the encode of contiguous (H,W,C) device tensors of one device on its current stream:
  -> (table, result, head).  table: the descriptor table (encode_table); result: the uint8 device
  buffer that will hold 8 bytes per image (uint32 bytes of its deflate stream, Adler-32 of its
  filtered bytes) and, from `head` on, the compact streams, image i's at table[i, 6].  One upload
  (the table) and the entry's two launches; nothing is waited for.  A 16-bit plane has 2 in field 3
  of its row and sends the whole batch through se3ds_png_encode_planes; a batch of uint8 images
  takes se3ds_png_encode.  fill: as encode_streams."""
  L = _lib.lib()
  n = len(images)
  dev = images[0].device
  geometries = [plane_geometry(x) for x in images]
  table = encode_table([x.data_ptr() for x in images], geometries, modes)
  assert table.shape[1] == L.se3ds_png_encode_fields()
  entry = 'se3ds_png_encode_planes' if any(g[2] == 2 for g in geometries) else 'se3ds_png_encode'
  workspace_bytes = getattr(L, entry + '_workspace_bytes')(table.ctypes.data, n)
  out_bytes = getattr(L, entry + '_out_bytes')(table.ctypes.data, n)
  head = aligned(8 * n)   # the sizes lead the result buffer
  with torch.cuda.device(dev):
    table_dev, _ = upload([table], dev)
    workspace = torch.empty((max(workspace_bytes, 16),), dtype=torch.uint8, device=dev)
    result = torch.empty((head + out_bytes,), dtype=torch.uint8, device=dev)
    if fill is not None:
      result.fill_(fill)
    rc = getattr(L, entry)(_lib.ptr(table_dev), table.ctypes.data, n, _lib.ptr(workspace),
                           workspace_bytes, _lib.ptr(result) + head, out_bytes, _lib.ptr(result), 3,
                           _lib.stream())
    _lib.check(rc, entry)
  return table, result, head


def encode_streams(images: Sequence[torch.Tensor], filters='adaptive', fill: int = None
                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
  """The device half of encode_png_batch: -> (table, sizes, streams).  table: the descriptor table
  (encode_table); sizes: uint32 (n, 2) = bytes of each image's deflate stream, Adler-32 of its
  filtered bytes; streams: the downloaded compact buffer, image i's stream at table[i, 6].  fill:
  the output buffer is set to this byte before the launches (tests look at what stays untouched).
  A 16-bit plane is (H,W,1) torch.int16 holding the bit patterns of uint16, the convention of
  datasets.indoor_datasets.RAW_DTYPES, or torch.uint16.  launch_encode, one download of the whole
  result, one synchronisation."""
  images = list(images)
  _lib.require_cuda(*images)
  dev = images[0].device
  for x in images:
    _check_pixels(x.shape, x.dtype, 'encode_png_batch')
    if x.device != dev:
      raise ValueError(f'encode_png_batch: a tensor on {x.device} in a batch on {dev}')
  images = [x.contiguous() for x in images]
  n = len(images)
  table, result, head = launch_encode(images, _filter_modes(filters, n), fill)
  buf = Readback(result).wait()
  return table, buf[:8 * n].view(np.uint32).reshape(n, 2), buf[head:]


def encode_png_batch(images: Sequence[torch.Tensor], filters='adaptive', device=None) -> List[bytes]:
  """uint8 device tensors (H,W,1|3) and 16-bit grey ones (H,W,1) (torch.int16 bit patterns of
  uint16, or torch.uint16), any mix of sizes -> their PNG files, encoded on the device:
  one upload (the descriptor table), se3ds_png_encode's two launches (csrc/png_encode.hip: filter
  and deflate every strip of every image, one wavefront each; pack the strips), one download (the
  sizes and the packed streams).  The host adds what has no width: signature, IHDR, the zlib
  framing of IDAT (78 01 + stream + Adler-32), IEND and the chunk CRCs.
  filters: 'adaptive' (per row the filter type with the smallest sum of |int8(residual)|), a PNG
  filter type 0..4 or its name, or a sequence with one of these per image.  device: where the
  tensors must be (None: where the first one is).  A non-CUDA tensor raises Se3dsHipError:
  encode_png_host is the CPU encoder."""
  images = list(images)
  if not images:
    return []
  if device is not None:
    dev = torch.device(device)
    for x in images:
      if x.device.type != dev.type or (dev.index is not None and x.device.index != dev.index):
        raise ValueError(f'encode_png_batch: a tensor on {x.device}, device={dev}')
  table, sizes, streams = encode_streams(images, filters)
  files = []
  for row, (size, adler) in zip(table, sizes):
    at, h, rb, bpp = int(row[6]), int(row[1]), int(row[2]), int(row[3])
    stream = b'\x78\x01' + streams[at:at + int(size)].tobytes() + struct.pack('>I', int(adler))
    files.append(png_container(h, rb // bpp, 1, stream, 16) if bpp == 2 else
                 png_container(h, rb // bpp, bpp, stream))
  return files


def _paeth_predictor(a, b, c):
  p = a + b - c
  pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
  return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows_host(pixels: np.ndarray, mode: int) -> np.ndarray:
  """uint8 (H,W,C) -> the filtered scan lines uint8 (H, 1 + W*C) under the device encoder's rule.
  uint16 (H,W,1): the same rule on the big-endian bytes PNG stores, 2 bytes per pixel -> (H, 1 + 2W)."""
  if pixels.dtype == np.uint16:
    pixels = np.ascontiguousarray(pixels.astype('>u2')).view(np.uint8).reshape(
        pixels.shape[0], pixels.shape[1], 2)
  h, w, c = pixels.shape
  cur = pixels.reshape(h, w * c).astype(np.int32)
  left = np.zeros_like(cur)
  left[:, c:] = cur[:, :-c]
  up = np.zeros_like(cur)
  up[1:] = cur[:-1]
  upleft = np.zeros_like(cur)
  upleft[:, c:] = up[:, :-c]
  if mode == ADAPTIVE:
    res = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1),
                    cur - _paeth_predictor(left, up, upleft)]) & 0xff
    types = np.argmin(np.where(res < 128, res, 256 - res).sum(axis=2), axis=0)
    rows = res[types, np.arange(h)]
  else:
    pred = (0, left, up, (left + up) >> 1, None)[mode]
    rows = (cur - (_paeth_predictor(left, up, upleft) if mode == 4 else pred)) & 0xff
    types = np.full((h,), mode)
  return np.concatenate([types[:, None], rows], axis=1).astype(np.uint8)


def encode_png_host(pixels: np.ndarray, filters='adaptive') -> bytes:
  """The CPU encoder: the same filters in NumPy, then zlib with Z_RLE (distance-1 matches only,
  as the device encoder).  The file decodes to the same pixels as encode_png_batch's; its bytes
  need not be equal.  A uint16 (H,W,1) array becomes a 16-bit greyscale file."""
  pixels = np.ascontiguousarray(pixels)
  _check_pixels(pixels.shape, pixels.dtype, 'encode_png_host')
  filtered = filter_rows_host(pixels, _filter_mode(filters))
  z = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
  h, w, c = pixels.shape
  return png_container(h, w, c, z.compress(filtered.tobytes()) + z.flush(),
                       16 if pixels.dtype == np.uint16 else 8)
