"""Animated GIF (GIF89a) for roll-outs: files that play, and the encoded_image_string TensorBoard's
image dashboard animates.  The format is fixed in DESIGN.md 3.18: one global palette of 256 entries
per video (grey: the identity, lossless; colour: median cut over a 32 768-bin histogram), ordered
8 x 8 dither, LZW coded in independent strips of whole rows that are joined at bit granularity.
`encode_gif_batch` runs histogram, look-up table, index plane, LZW and pack on the device
(csrc/gif.hip); `encode_gif_host` writes the same bytes in NumPy and Python, so that a CPU-only
process can write videos.  Inter-frame transparency, local colour tables, per-frame delays,
error-diffusion dither and GIF decode on the device are out of scope."""
import struct
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd.utils._staging import Readback, aligned, upload

BINS = 32768
STRIP_PIXELS = 16384
_CLEAR, _END, _FIRST_FREE, _MAX_CODES = 256, 257, 258, 4096


def strip_rows(width: int) -> int:
  """Rows of one LZW strip of a frame `width` pixels wide: the whole rows that reach 16 384 pixels."""
  return max(1, (STRIP_PIXELS + int(width) - 1) // int(width))


def delay_cs(fps: float) -> int:
  """The frame delay in hundredths of a second; players treat less than 2 as 10."""
  if not fps > 0:
    raise ValueError(f'fps: a positive rate, got {fps!r}')
  return max(2, int(100 / fps + 0.5))


def _bayer8() -> np.ndarray:
  y, x = np.mgrid[0:8, 0:8]
  a, b = x ^ y, y
  return ((a & 1) << 5 | (b & 1) << 4 | (a & 2) << 2 | (b & 2) << 1 | (a & 4) >> 1 | (b & 4) >> 2).astype(np.int64)


def grey_palette() -> np.ndarray:
  return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def histogram(video: np.ndarray) -> np.ndarray:
  """(T,H,W,3) uint8 -> uint32 [32768], bin = (r>>3)<<10 | (g>>3)<<5 | (b>>3)."""
  v = video.reshape(-1, 3).astype(np.int64) >> 3
  return np.bincount(v[:, 0] << 10 | v[:, 1] << 5 | v[:, 2], minlength=BINS).astype(np.uint32)


def median_cut(hist) -> Tuple[np.ndarray, int]:
  """uint32 [32768] -> (palette uint8 (256,3), n_used).  Boxes of non-empty bins are split, the box
  with the most pixels first (lowest index on a tie), along the channel of the largest 5-bit extent
  (g, r, b on a tie), at the weighted median of the bins ordered by (coordinate, bin); an entry is
  the rounded weighted mean of its box's bin centres in exact integers; unused entries are black."""
  hist = np.asarray(hist).astype(np.int64).reshape(-1)
  if hist.size != BINS:
    raise ValueError(f'hist: {BINS} bins expected, got {hist.size}')
  bins = np.flatnonzero(hist)
  if bins.size == 0:
    raise ValueError('hist: no pixel counted')
  boxes = [bins]                       # ascending bin order
  totals = [int(hist[bins].sum())]     # a box of one bin cannot be split: -1 once it is known
  if bins.size < 2:
    totals[0] = -1
  while len(boxes) < 256:
    pick = int(np.argmax(totals))      # the first of equals
    if totals[pick] < 0:
      break
    box = boxes[pick]
    coords = np.stack([box >> 5 & 31, box >> 10, box & 31])   # g, r, b: argmax keeps the first of equals
    axis = int(np.argmax(coords.max(axis=1) - coords.min(axis=1)))
    box = box[np.lexsort((box, coords[axis]))]
    counts = hist[box]
    total = int(counts.sum())
    k = int(np.searchsorted(np.cumsum(counts), (total + 1) // 2)) + 1
    k = min(max(k, 1), box.size - 1)
    for at, part in ((pick, box[:k]), (len(boxes), box[k:])):
      part_total = int(hist[part].sum()) if part.size >= 2 else -1
      if at == len(boxes):
        boxes.append(part)
        totals.append(part_total)
      else:
        boxes[at], totals[at] = part, part_total
  palette = np.zeros((256, 3), np.uint8)
  for i, box in enumerate(boxes):
    counts = hist[box]
    total = int(counts.sum())
    for ch, coord in enumerate((box >> 10, box >> 5 & 31, box & 31)):
      palette[i, ch] = (int((counts * (8 * coord + 4)).sum()) + total // 2) // total
  return palette, len(boxes)


def nearest_lut(palette: np.ndarray, n_used: int) -> np.ndarray:
  """-> uint8 [32768]: for every bin centre (8r+4, 8g+4, 8b+4) the entry among the first `n_used`
  with the least squared distance, the lowest index on a tie."""
  if not 1 <= int(n_used) <= 256:
    raise ValueError(f'n_used: 1..256, got {n_used!r}')
  pal = np.asarray(palette)[:int(n_used)].astype(np.int32)
  axis = 8 * np.arange(32, dtype=np.int32) + 4
  lut = np.empty((32, 32 * 32), np.uint8)
  gb = ((axis[:, None, None] - pal[None, None, :, 1]) ** 2 + (axis[None, :, None] - pal[None, None, :, 2]) ** 2)
  for r in range(32):
    d = gb + (axis[r] - pal[:, 0]) ** 2
    lut[r] = d.reshape(1024, -1).argmin(axis=1)
  return lut.reshape(-1)


def index_plane(video: np.ndarray, lut: np.ndarray, dither: int = 32) -> np.ndarray:
  """(T,H,W,3) uint8 -> (T,H,W) uint8: v' = clamp(v + ((B8[y&7][x&7] * A) >> 6) - (A >> 1)), lut[bin(v')]."""
  _, h, w, _ = video.shape
  d = _bayer8()[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7]
  off = ((d * int(dither)) >> 6) - (int(dither) >> 1)
  v = np.clip(video.astype(np.int64) + off[None, :, :, None], 0, 255) >> 3
  return np.asarray(lut)[v[..., 0] << 10 | v[..., 1] << 5 | v[..., 2]]


class _Bits:
  """LSB-first bit string: whole bytes are set aside 64 at a time, the rest waits in an integer."""

  def __init__(self):
    self.acc, self.bits, self.parts = 0, 0, []

  def emit(self, code, width):
    self.acc |= code << self.bits
    self.bits += width
    if self.bits >= 512:
      self.parts.append((self.acc & ((1 << 512) - 1)).to_bytes(64, 'little'))
      self.acc >>= 512
      self.bits -= 512

  def bytes(self):
    return b''.join(self.parts) + self.acc.to_bytes((self.bits + 7) // 8, 'little')


def _lzw_strip(px, first: bool, last: bool, out: _Bits):
  """One strip from a fresh table; the entry counted behind the strip's last code is the one the
  decoder adds there, which keeps both at the same width for the closing code."""
  width, nxt, table = 9, _FIRST_FREE, {}
  if first:
    out.emit(_CLEAR, 9)
  it = iter(px.tolist())
  prefix = next(it)
  for c in it:
    key = prefix << 8 | c
    code = table.get(key)
    if code is not None:
      prefix = code
      continue
    out.emit(prefix, width)
    if nxt < _MAX_CODES:
      table[key] = nxt
      if nxt == 1 << width and width < 12:
        width += 1
      nxt += 1
    else:
      out.emit(_CLEAR, width)
      table.clear()
      width, nxt = 9, _FIRST_FREE
    prefix = c
  out.emit(prefix, width)
  if nxt < _MAX_CODES and nxt == 1 << width and width < 12:
    width += 1
  out.emit(_END if last else _CLEAR, width)


def lzw_frame(index: np.ndarray) -> bytes:
  """(H,W) uint8 palette indices -> the frame's LZW data (before it is cut into sub-blocks)."""
  h, w = index.shape
  rows = strip_rows(w)
  out = _Bits()
  for r in range(0, h, rows):
    _lzw_strip(index[r:r + rows].reshape(-1), r == 0, r + rows >= h, out)
  return out.bytes()


def sub_blocks(data: bytes) -> bytes:
  """Sub-blocks of 255 bytes, the last one shorter, and the terminator."""
  parts = []
  for at in range(0, len(data), 255):
    part = data[at:at + 255]
    parts += [bytes([len(part)]), part]
  return b''.join(parts) + b'\x00'


def gif_container(width: int, height: int, palette: np.ndarray, frames: Sequence[bytes], fps: float = 10,
                  loop: Optional[int] = 0) -> bytes:
  """frames: per frame its sub-blocks with the terminator.  loop: the NETSCAPE2.0 repeat count
  (0 = for ever), None = no loop extension (play once)."""
  if not (1 <= width <= 65535 and 1 <= height <= 65535):
    raise ValueError(f'size: 1..65535 each way, got {width} x {height}')
  if loop is not None and not 0 <= int(loop) <= 65535:
    raise ValueError(f'loop: None or 0..65535, got {loop!r}')
  palette = np.ascontiguousarray(palette, np.uint8)
  if palette.shape != (256, 3):
    raise ValueError(f'palette: (256,3) expected, got {palette.shape}')
  out = [b'GIF89a', struct.pack('<HH', width, height), b'\xf7\x00\x00', palette.tobytes()]
  if loop is not None:
    out.append(b'\x21\xff\x0bNETSCAPE2.0\x03\x01' + struct.pack('<H', int(loop)) + b'\x00')
  control = b'\x21\xf9\x04\x04' + struct.pack('<H', delay_cs(fps)) + b'\x00\x00'
  descriptor = b'\x2c\x00\x00\x00\x00' + struct.pack('<HH', width, height) + b'\x00\x08'
  for blocks in frames:
    out += [control, descriptor, blocks]
  out.append(b'\x3b')
  return b''.join(out)


class GifFile(NamedTuple):
  """What parse_gif finds: frames holds, per frame, the LZW data with the sub-block framing removed."""
  width: int
  height: int
  palette: np.ndarray
  loop: Optional[int]
  delays: List[int]
  frames: List[bytes]


def parse_gif(buf: bytes) -> GifFile:
  """A container walk over the files this module writes (global colour table of 256, no local
  tables, full-size frames); ValueError naming the offset for anything else."""
  buf = bytes(buf)

  def fail(p, what):
    raise ValueError(f'GIF: {what} at byte {p}')

  if buf[:6] != b'GIF89a' or len(buf) < 13 + 768 + 1:
    fail(0, 'no GIF89a header with a 256-entry global colour table')
  width, height = struct.unpack('<HH', buf[6:10])
  if buf[10] != 0xf7:
    fail(10, 'no 256-entry global colour table')
  palette = np.frombuffer(buf, np.uint8, 768, 13).reshape(256, 3).copy()
  p, loop, delays, frames = 13 + 768, None, [], []
  while True:
    if p >= len(buf):
      fail(p, 'no trailer')
    if buf[p] == 0x3b:
      if p != len(buf) - 1:
        fail(p, 'bytes behind the trailer')
      return GifFile(width, height, palette, loop, delays, frames)
    if buf[p] == 0x21:
      if buf[p + 1:p + 3] == b'\xf9\x04':
        delays.append(struct.unpack('<H', buf[p + 4:p + 6])[0])
      elif buf[p + 1:p + 14] == b'\xff\x0bNETSCAPE2.0' and buf[p + 14:p + 16] == b'\x03\x01':
        loop, = struct.unpack('<H', buf[p + 16:p + 18])
      p += 2
      while p < len(buf) and buf[p]:
        p += 1 + buf[p]
      p += 1
    elif buf[p] == 0x2c:
      if struct.unpack('<HHHH', buf[p + 1:p + 9]) != (0, 0, width, height) or buf[p + 9] != 0 or buf[p + 10] != 8:
        fail(p, 'a frame that is not full-size, has a local colour table or a code size other than 8')
      p += 11
      data = []
      while p < len(buf) and buf[p]:
        data.append(buf[p + 1:p + 1 + buf[p]])
        p += 1 + buf[p]
      p += 1
      frames.append(b''.join(data))
    else:
      fail(p, f'unknown block 0x{buf[p]:02x}')


def _check_video(shape, dtype, name='video'):
  if len(shape) != 4 or shape[3] not in (1, 3) or str(dtype).split('.')[-1] != 'uint8':
    raise ValueError(f'{name}: uint8 (T,H,W,1|3) expected, got {str(dtype)} {tuple(shape)}')
  t, h, w, _ = (int(s) for s in shape)
  if t < 1 or not (1 <= h <= 65535 and 1 <= w <= 65535):
    raise ValueError(f'{name}: T >= 1 and 1 <= H, W <= 65535 expected, got {tuple(shape)}')


def _check_dither(dither) -> int:
  if int(dither) != dither or not 0 <= int(dither) <= 255:
    raise ValueError(f'dither: an amplitude 0..255, got {dither!r}')
  return int(dither)


def quantise_host(video: np.ndarray, dither: int = 32) -> Tuple[np.ndarray, np.ndarray]:
  """(T,H,W,1|3) uint8 -> (palette (256,3), index plane (T,H,W))."""
  if video.shape[3] == 1:
    return grey_palette(), np.ascontiguousarray(video[..., 0])
  palette, used = median_cut(histogram(video))
  return palette, index_plane(video, nearest_lut(palette, used), dither)


def encode_gif_host(video: np.ndarray, fps: float = 10, loop: Optional[int] = 0, dither: int = 32) -> bytes:
  """uint8 (T,H,W,1|3) NumPy array -> the GIF file encode_gif_batch writes for it, byte for byte,
  without a device: NumPy for the palette and the index plane, a Python loop for LZW."""
  video = np.asarray(video)
  _check_video(video.shape, video.dtype)
  palette, index = quantise_host(video, _check_dither(dither))
  return gif_container(video.shape[2], video.shape[1], palette, [sub_blocks(lzw_frame(f)) for f in index], fps, loop)


class GifBatch:
  """Table, workspace and output buffer of one batch on the current stream of the videos' device.
  The stages are queued apart (`histogram` .. `pack`; tools/gif_encode_bench.py times them so);
  `region(i)` is the workspace from region i of se3ds_gif_workspace_offset on."""

  def __init__(self, videos, dither: int = 32):
    L = _lib.lib()
    self.videos, self.device, n = videos, videos[0].device, len(videos)
    table = np.zeros((n, L.se3ds_gif_fields()), np.int64)
    for i, v in enumerate(videos):
      table[i, :6] = (v.data_ptr(), v.shape[0], v.shape[1], v.shape[2], v.shape[3], dither)
    _lib.check(L.se3ds_gif_plan(table.ctypes.data, n), 'se3ds_gif_plan')
    self.table = table
    self.workspace_bytes = L.se3ds_gif_workspace_bytes(table.ctypes.data, n)
    self.out_bytes = L.se3ds_gif_out_bytes(table.ctypes.data, n)
    self.offsets = [L.se3ds_gif_workspace_offset(table.ctypes.data, n, r) for r in range(7)]
    self.frames = int(sum(v.shape[0] for v in videos))
    with torch.cuda.device(self.device):
      self.table_dev, _ = upload([table], self.device)
      self.workspace = torch.empty((self.workspace_bytes,), dtype=torch.uint8, device=self.device)
      self.out = torch.empty((self.out_bytes,), dtype=torch.uint8, device=self.device)

  def _stage(self, name, *extra):
    with torch.cuda.device(self.device):
      rc = getattr(_lib.lib(), name)(_lib.ptr(self.table_dev), self.table.ctypes.data, len(self.table), *extra,
                                     _lib.ptr(self.workspace), self.workspace_bytes, _lib.stream())
    _lib.check(rc, name)

  def region(self, i):
    return self.workspace[self.offsets[i]:self.offsets[i + 1]]

  def histogram(self):
    self._stage('se3ds_gif_histogram')

  def histograms(self):
    """uint32 (n, 32768) device view; rows of grey videos are zero."""
    return self.region(0)[:len(self.table) * BINS * 4].view(torch.int32).view(len(self.table), BINS)

  def lut(self, palettes: np.ndarray, used: np.ndarray):
    """palettes uint8 (n,256,3), used int32 (n,) with 0 for a grey video: one upload, one launch."""
    both, at = upload([np.ascontiguousarray(palettes, np.uint8), np.ascontiguousarray(used, np.int32)], self.device)
    self._tables = both   # alive until the stream has used them
    self._stage('se3ds_gif_lut', both[at[0]:].data_ptr(), both[at[1]:].data_ptr())

  def index(self):
    self._stage('se3ds_gif_index')

  def lzw(self):
    self._stage('se3ds_gif_lzw')

  def pack(self):
    with torch.cuda.device(self.device):
      rc = _lib.lib().se3ds_gif_pack(_lib.ptr(self.table_dev), self.table.ctypes.data, len(self.table),
                                     _lib.ptr(self.workspace), self.workspace_bytes, _lib.ptr(self.out),
                                     self.out_bytes, _lib.stream())
    _lib.check(rc, 'se3ds_gif_pack')

  def frame_blocks(self) -> List[List[bytes]]:
    """Per video, per frame: the sub-blocks with the terminator.  One read-back: the frame sizes lie
    in front of the frame areas in one buffer."""
    host = Readback(self.out).wait()
    sizes = host[:self.frames * 8].view(np.int64)
    areas = host[aligned(self.frames * 8):]
    out = []
    for row in self.table:
      frames, first, at, step = int(row[1]), int(row[6]), int(row[10]), int(row[11])
      out.append([areas[at + f * step:at + f * step + int(sizes[first + f])].tobytes() for f in range(frames)])
    return out


def encode_gif_batch(videos, fps: float = 10, loop: Optional[int] = 0, dither: int = 32, device=None) -> List[bytes]:
  """uint8 device tensors (T,H,W,1|3), any mix of sizes and channel counts -> their animated GIF
  files, the bytes encode_gif_host writes.  One upload (the table), then one launch per stage for
  the whole batch (csrc/gif.hip): histogram, look-up table, index plane, LZW (a wave per strip),
  pack (two launches).  Host synchronisations per call: two.  The first is the histogram download
  (128 KB a colour video), because the median cut runs on the host in NumPy; a batch of grey videos
  skips it, and histogram, look-up table and index plane with it.  The second is the frame sizes
  together with the packed bytes, one buffer.  That buffer is sized for the worst case (1.5 bytes a
  pixel and the sub-block framing) and comes back whole.
  fps: one rate for the file, delay = max(2, int(100 / fps + 0.5)) hundredths of a second.  loop: the
  repeat count, 0 = for ever, None = play once.  dither: the amplitude of the ordered dither, 0 =
  off; grey videos are not dithered.  device: where the tensors must be (None: where the first one
  is).  Bad arguments raise ValueError; a non-CUDA tensor raises Se3dsHipError: the CPU encoder is
  encode_gif_host."""
  videos = list(videos)
  if not videos:
    return []
  for i, v in enumerate(videos):
    if not isinstance(v, torch.Tensor):
      raise ValueError(f'videos[{i}]: a device tensor expected, got {type(v).__name__}')
    _check_video(v.shape, v.dtype, f'videos[{i}]')
  dither = _check_dither(dither)
  delay_cs(fps)
  if loop is not None and not 0 <= int(loop) <= 65535:
    raise ValueError(f'loop: None or 0..65535, got {loop!r}')
  dev = videos[0].device if device is None else torch.device(device)
  for v in videos:
    if v.device.type != dev.type or (dev.index is not None and v.device.index != dev.index):
      raise ValueError(f'videos: a tensor on {v.device} in a batch on {dev}')
  _lib.require_cuda(*videos)
  batch = GifBatch([v.contiguous() for v in videos], dither)
  n = len(videos)
  palettes = np.zeros((n, 256, 3), np.uint8)
  used = np.zeros((n,), np.int32)
  colour = [i for i, v in enumerate(videos) if v.shape[3] == 3]
  if colour:
    batch.histogram()
    hists = Readback(batch.histograms()).wait().view(np.uint32)
    for i in colour:
      palettes[i], used[i] = median_cut(hists[i])
    batch.lut(palettes, used)
    batch.index()
  for i in range(n):
    if i not in colour:
      palettes[i] = grey_palette()
  batch.lzw()
  batch.pack()
  return [gif_container(int(v.shape[2]), int(v.shape[1]), palettes[i], blocks, fps, loop)
          for i, (v, blocks) in enumerate(zip(videos, batch.frame_blocks()))]
