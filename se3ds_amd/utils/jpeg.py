"""Baseline JPEG files <-> uint8 pixels on the device, without TensorFlow or an image library: the
`tf.image.decode_jpeg(rgb.jpeg)` the VLN augmentation notebook starts from, the container
Matterport panoramas are distributed in, and the files the augmentation writes back.

  parse_jpeg         the container on the host (NumPy): SOF0 / SOF1 at 8 bits, DQT, DHT, DRI, one
                     interleaved SOS; the entropy segments are found, nothing is decoded.
  decode_jpeg_batch  files of any mix of geometries -> one upload, one `se3ds_jpeg_decode`
                     (csrc/jpeg.hip: speculative parallel Huffman decode per restart interval,
                     slow-integer inverse DCT, fancy upsampling, colour), tensors (H, W, C) uint8.
  encode_jpeg_batch  uint8 tensors of any mix of sizes -> the files libjpeg's default encoder writes
                     (Pillow's Image.save at the same quality and subsampling), byte for byte: one
                     `se3ds_jpeg_encode` (csrc/jpeg_encode.hip), the container (`jpeg_container`,
                     `quality_tables`) on the host.

The arithmetic is libjpeg's defaults (JDCT_ISLOW, fancy upsampling), which `tf.image.decode_jpeg`
documents as its defaults too; the tests pin it against Pillow.  Where a sample leaves [0, 255]
before the clamp by more than a decoder's look-up table covers, this decoder saturates.

There is no CPU fallback: a non-CUDA device raises Se3dsHipError."""
import enum
import struct
from typing import List, NamedTuple, Sequence, Tuple, Union

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd.utils._staging import Readback, cuda_device, layout, upload

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34,
                   27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44,
                   51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

_SOF_KINDS = {0xC2: 'progressive', 0xC3: 'lossless', 0xC5: 'differential sequential',
              0xC6: 'differential progressive', 0xC7: 'differential lossless',
              0xC9: 'arithmetic-coded sequential', 0xCA: 'arithmetic-coded progressive',
              0xCB: 'arithmetic-coded lossless', 0xCD: 'arithmetic-coded differential sequential',
              0xCE: 'arithmetic-coded differential progressive',
              0xCF: 'arithmetic-coded differential lossless'}


class JpegScan(NamedTuple):
  """A parsed baseline JPEG: geometry, tables and where the entropy segments lie in `data`."""
  height: int
  width: int
  components: int                 # 1 or 3
  h0: int                         # sampling of the first component (the others are 1 x 1); grey: 1, 1
  v0: int
  quant: np.ndarray               # (components, 64) uint16, row-major order
  huffman: np.ndarray             # (4, 272) uint8: DC 0, DC 1, AC 0, AC 1; 16 counts + 256 values
  tables: int                     # bit c: DC table of component c; bit 4 + c: its AC table
  restart_interval: int           # MCUs per segment, 0 = one segment
  segments: Tuple[Tuple[int, int], ...]   # (offset in data, length): the RSTn markers are not inside
  data: bytes

  @property
  def mcus_x(self):
    return -(-self.width // (8 * self.h0))

  @property
  def mcus_y(self):
    return -(-self.height // (8 * self.v0))

  @property
  def blocks_per_mcu(self):
    return 1 if self.components == 1 else self.h0 * self.v0 + 2


def _segment(buf, p, what):
  if p + 2 > len(buf):
    raise ValueError(f'JPEG: the file ends inside {what}')
  n = (buf[p] << 8) | buf[p + 1]
  if n < 2 or p + n > len(buf):
    raise ValueError(f'JPEG: the length of {what} leaves the file')
  return buf[p + 2:p + n], p + n


def parse_jpeg(buf: bytes) -> JpegScan:
  """The container walk.  ValueError: not a well-formed file.  NotImplementedError naming the kind:
  a well-formed file this decoder does not read."""
  buf = bytes(buf)
  if buf[:2] != b'\xff\xd8':
    raise ValueError('JPEG: no SOI marker')
  p, qt, ht, dri, frame, adobe = 2, {}, {}, 0, None, None
  while True:
    if p + 2 > len(buf):
      raise ValueError('JPEG: no SOS marker' if frame else 'JPEG: no SOF marker')
    if buf[p] != 0xFF:
      raise ValueError(f'JPEG: no marker at byte {p}')
    m = buf[p + 1]
    if m == 0xFF:   # fill byte
      p += 1
      continue
    p += 2
    if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
      continue
    if m == 0xD9:
      raise ValueError('JPEG: no SOS marker' if frame else 'JPEG: no SOF marker')
    if m in _SOF_KINDS:
      raise NotImplementedError(f'JPEG: {_SOF_KINDS[m]} frames are not supported (baseline only)')
    if m in (0xC0, 0xC1):
      s, p = _segment(buf, p, 'SOF')
      if frame is not None:
        raise ValueError('JPEG: two SOF markers')
      if len(s) < 6 or len(s) != 6 + 3 * s[5]:
        raise ValueError('JPEG: the length of SOF does not fit its component count')
      if s[0] == 12:
        raise NotImplementedError('JPEG: 12-bit samples are not supported')
      if s[0] != 8:
        raise ValueError(f'JPEG: sample precision {s[0]}')
      height, width, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
      if height == 0 or width == 0 or nc == 0:
        raise ValueError(f'JPEG: zero size ({height} x {width}, {nc} components)')
      comps = [(s[6 + 3 * i], s[7 + 3 * i] >> 4, s[7 + 3 * i] & 15, s[8 + 3 * i]) for i in range(nc)]
      if nc == 4:
        raise NotImplementedError('JPEG: four components (CMYK / YCCK) are not supported')
      if nc not in (1, 3):
        raise NotImplementedError(f'JPEG: {nc} components are not supported')
      if any(h == 0 or v == 0 or h > 4 or v > 4 or tq > 3 for _, h, v, tq in comps):
        raise ValueError('JPEG: sampling factor or table number out of range in SOF')
      frame = (height, width, comps)
    elif m == 0xDB:
      s, p = _segment(buf, p, 'DQT')
      i = 0
      while i < len(s):
        pq, tq = s[i] >> 4, s[i] & 15
        n = 128 if pq == 1 else 64
        if pq > 1 or tq > 3 or i + 1 + n > len(s):
          raise ValueError('JPEG: malformed DQT')
        raw = np.frombuffer(s, np.uint8, n, i + 1)
        vals = raw.astype(np.uint16) if pq == 0 else (raw[0::2].astype(np.uint16) << 8) | raw[1::2]
        table = np.zeros(64, np.uint16)
        table[ZIGZAG] = vals
        qt[tq] = table
        i += 1 + n
    elif m == 0xC4:
      s, p = _segment(buf, p, 'DHT')
      i = 0
      while i < len(s):
        if i + 17 > len(s):
          raise ValueError('JPEG: malformed DHT')
        tc, th = s[i] >> 4, s[i] & 15
        counts = np.frombuffer(s, np.uint8, 16, i + 1)
        n, code = int(counts.sum()), 0
        for l in range(16):
          code += int(counts[l])
          if code > (2 << l):
            raise ValueError('JPEG: DHT counts that no prefix code has')
          code <<= 1
        if tc > 1 or th > 3 or n > 256 or i + 17 + n > len(s):
          raise ValueError('JPEG: malformed DHT')
        row = np.zeros(272, np.uint8)
        row[:16] = counts
        row[16:16 + n] = np.frombuffer(s, np.uint8, n, i + 17)
        ht[(tc, th)] = row
        i += 17 + n
    elif m == 0xDD:
      s, p = _segment(buf, p, 'DRI')
      if len(s) != 2:
        raise ValueError('JPEG: malformed DRI')
      dri = (s[0] << 8) | s[1]
    elif m == 0xEE:
      s, p = _segment(buf, p, 'APP14')
      if len(s) >= 12 and s[:5] == b'Adobe':
        adobe = s[11]
    elif m == 0xDA:
      s, p = _segment(buf, p, 'SOS')
      break
    else:   # APPn, COM, DNL, ...: skipped
      s, p = _segment(buf, p, f'marker {m:02X}')
  if frame is None:
    raise ValueError('JPEG: no SOF marker in front of SOS')
  height, width, comps = frame
  nc = len(comps)
  if len(s) < 1 or len(s) != 4 + 2 * s[0]:
    raise ValueError('JPEG: malformed SOS')
  if s[0] != nc:
    raise NotImplementedError('JPEG: more than one scan (non-interleaved components) is not supported')
  sel = [(s[1 + 2 * i], s[2 + 2 * i] >> 4, s[2 + 2 * i] & 15) for i in range(nc)]
  if [c for c, _, _ in sel] != [c[0] for c in comps]:
    raise ValueError('JPEG: the components of SOS are not those of SOF')
  if tuple(s[1 + 2 * nc:]) != (0, 63, 0):
    raise ValueError('JPEG: spectral selection or approximation in a sequential scan')
  if nc == 3 and (adobe == 0 or bytes(c[0] for c in comps) == b'RGB'):
    raise NotImplementedError('JPEG: Adobe APP14 transform 0 (RGB components) is not supported')
  if nc == 1:
    h0 = v0 = 1   # one component: the scan is not interleaved, an MCU is one block
  else:
    h0, v0 = comps[0][1], comps[0][2]
    if (h0, v0) not in ((1, 1), (2, 1), (2, 2)) or any((h, v) != (1, 1) for _, h, v, _ in comps[1:]):
      kinds = ', '.join(f'{h}x{v}' for _, h, v, _ in comps)
      raise NotImplementedError(f'JPEG: sampling {kinds} is not supported (4:4:4, 4:2:2 as 2x1 and '
                                '4:2:0 as 2x2 are)')
  quant = np.zeros((nc, 64), np.uint16)
  for i, (_, _, _, tq) in enumerate(comps):
    if tq not in qt:
      raise ValueError(f'JPEG: quantisation table {tq} is missing')
    quant[i] = qt[tq]
  huffman, tables = np.zeros((4, 272), np.uint8), 0
  for tc in (0, 1):
    used = []
    for i, one in enumerate(sel):
      th = one[1 + tc]
      if (tc, th) not in ht:
        raise ValueError(f"JPEG: {'AC' if tc else 'DC'} Huffman table {th} is missing")
      if th not in used:
        used.append(th)
      tables |= used.index(th) << (4 * tc + i) if used.index(th) < 2 else 0
    if len(used) > 2:
      raise NotImplementedError(f"JPEG: more than two {'AC' if tc else 'DC'} Huffman tables in one scan "
                                'are not supported')
    for slot, th in enumerate(used):
      huffman[2 * tc + slot] = ht[(tc, th)]

  # the entropy segments: an FF that no 00 follows is a marker
  a = np.frombuffer(buf, np.uint8)
  marks = np.flatnonzero((a[p:-1] == 0xFF) & (a[p + 1:] != 0)) + p
  segments, start, end, expect, closed = [], p, None, 0, False
  for pos in marks.tolist():
    m = buf[pos + 1]
    if end is None:
      end = pos
    if m == 0xFF:
      continue
    if 0xD0 <= m <= 0xD7:
      if m - 0xD0 != expect:
        raise ValueError(f'JPEG: RST{m - 0xD0} where RST{expect} is due')
      expect = (expect + 1) & 7
      segments.append((start, end - start))
      start, end = pos + 2, None
    elif m == 0xD9:
      segments.append((start, end - start))
      closed = True
      break
    elif m in (0xDA, 0xC4, 0xDB, 0xDD):
      raise NotImplementedError('JPEG: more than one scan is not supported')
    else:
      raise ValueError(f'JPEG: marker {m:02X} inside the scan')
  if not closed:
    raise ValueError('JPEG: no EOI marker')
  mcus = -(-width // (8 * h0)) * -(-height // (8 * v0))
  want = -(-mcus // dri) if dri else 1
  if len(segments) != want:
    raise ValueError(f'JPEG: {len(segments)} entropy segments where the geometry and DRI = {dri} give {want}')
  return JpegScan(height, width, nc, h0, v0, quant, huffman, tables, dri, tuple(segments), buf)


# --------------------------------------------------------------------------------- the device
class JpegStatus(enum.IntEnum):
  """`enum class Status` of csrc/jpeg_core.h."""
  OK = 0
  TRUNCATED = 1
  BAD_CODE = 2
  BAD_RUN = 3
  BAD_DC = 4
  TOO_LONG = 5


_REASONS = {
    JpegStatus.TRUNCATED: 'the entropy-coded bits end before the last block',
    JpegStatus.BAD_CODE: 'bits that are no Huffman code word',
    JpegStatus.BAD_RUN: 'a zero run past coefficient 63',
    JpegStatus.BAD_DC: 'a DC difference category above 11',
    JpegStatus.TOO_LONG: 'entropy-coded bytes behind the last block',
}


def jpeg_failure(word: int) -> str:
  """The message of a non-zero status code of se3ds_jpeg_decode."""
  return f'the scan does not decode: {_REASONS[JpegStatus(word & 0xff)]}'


def status_rounds(words) -> np.ndarray:
  """The round counts in the status words of se3ds_jpeg_decode."""
  return (np.asarray(words).astype(np.int64) >> 8) & 0x7fffff


class PendingJpegDecode(Readback):
  """One batch in flight: `check()` waits for the status words and raises ValueError for the first
  image with a segment that failed.  The tensors count only once it has returned.  `words` (after
  check or wait): the status word of every segment; `segment_image`: the image of each."""

  def __init__(self, status: torch.Tensor, segment_image):
    super().__init__(status)   # the status words on the device: their copy and its event are queued
    self.segment_image = segment_image

  @property
  def words(self) -> np.ndarray:
    return self.wait()

  def check(self) -> None:
    words = self.wait()
    bad = np.flatnonzero(words & 0xff)
    if bad.size:
      s = int(bad[0])
      raise ValueError(f'image {int(self.segment_image[s])}: {jpeg_failure(int(words[s]))}')


def output_channels(scan: JpegScan, channels: int) -> int:
  if channels not in (0, 1, 3):
    raise ValueError(f'channels: 0 (the file\'s), 1 or 3, got {channels!r}')
  return channels or scan.components


class JpegBatch:
  """The tables, the uploaded bytes, the workspace and the output tensors of one batch, on the current
  stream of `device`: `launch(phases)` queues `se3ds_jpeg_decode` on them (the timing tool launches
  more than once), `pending()` queues the copy of the status words."""

  def __init__(self, scans: Sequence[JpegScan], dev, channels: int = 0):
    out_c = [output_channels(s, channels) for s in scans]
    L = _lib.lib()
    n = len(scans)
    fields, seg_fields = L.se3ds_jpeg_decode_fields(), L.se3ds_jpeg_decode_segment_fields()
    n_seg = sum(len(s.segments) for s in scans)
    images = np.zeros((n, fields), np.int64)
    segments = np.zeros((n_seg, seg_fields), np.int64)
    image_bytes = images.view(np.uint8).reshape(n, fields * 8)
    # the segments of a file lie in it one behind the other, RSTn markers between: one span a file,
    # behind the two tables
    spans = [memoryview(s.data)[s.segments[0][0]:s.segments[-1][0] + s.segments[-1][1]] for s in scans]
    offsets, self.buf_bytes = layout([images.nbytes + segments.nbytes] + [len(b) for b in spans])
    coef_sizes, plane_sizes, at = [], [], 0
    for i, s in enumerate(scans):
      images[i, :5] = (s.width, s.height, s.components, s.h0, s.v0)
      images[i, 6] = out_c[i]
      images[i, 9:14] = (at, len(s.segments), s.mcus_x, s.mcus_y, s.tables)
      image_bytes[i, 128:128 + 128 * s.components] = s.quant.view(np.uint8).reshape(-1)
      image_bytes[i, 512:] = s.huffman.reshape(-1)
      coef_sizes.append(s.mcus_x * s.mcus_y * s.blocks_per_mcu * 128)
      planes = s.mcus_x * s.h0 * 8 * s.mcus_y * s.v0 * 8
      if s.components == 3:
        planes += 2 * s.mcus_x * 8 * s.mcus_y * 8
      plane_sizes.append(planes)
      first = s.segments[0][0]
      mcus, step, mcu = s.mcus_x * s.mcus_y, s.restart_interval or s.mcus_x * s.mcus_y, 0
      for k, (seg_at, seg_len) in enumerate(s.segments):
        segments[at + k] = (i, offsets[1 + i] + seg_at - first, seg_len, mcu, min(step, mcus - mcu))
        mcu += step
      at += len(s.segments)
    # the workspace: every image's coefficients, then every image's planes
    workspace_at, self.workspace_bytes = layout(coef_sizes + plane_sizes)
    images[:, 7], images[:, 8] = workspace_at[:n], workspace_at[n:]
    self.images, self.segments, self.device = images, segments, dev
    with torch.cuda.device(dev):
      self.out = [torch.empty((s.height, s.width, c), dtype=torch.uint8, device=dev)
                  for s, c in zip(scans, out_c)]
      images[:, 5] = [t.data_ptr() for t in self.out]
      need = L.se3ds_jpeg_decode_workspace_bytes(images.ctypes.data, n)   # 0: the launch says why
      assert need in (0, self.workspace_bytes), f'workspace layout: {self.workspace_bytes}, library {need}'
      tables = np.concatenate([images.reshape(-1), segments.reshape(-1)])
      self.device_buf, _ = upload([tables] + spans, dev)
      self.workspace = torch.empty((max(self.workspace_bytes, 16),), dtype=torch.uint8, device=dev)
      self.status = torch.zeros((n_seg,), dtype=torch.int32, device=dev)

  def launch(self, phases: int = 7) -> None:
    with torch.cuda.device(self.device):
      rc = _lib.lib().se3ds_jpeg_decode(
          _lib.ptr(self.device_buf), self.buf_bytes, _lib.ptr(self.workspace), self.workspace_bytes,
          self.images.ctypes.data, len(self.images), self.segments.ctypes.data, len(self.segments),
          _lib.ptr(self.status), phases, _lib.stream())
    _lib.check(rc, 'se3ds_jpeg_decode')

  def pending(self) -> PendingJpegDecode:
    return PendingJpegDecode(self.status, self.segments[:, 0].copy())


def decode_jpeg_batch(bufs: Sequence[Union[bytes, JpegScan]], device, channels: int = 0,
                      check: bool = True):
  """Encoded JPEG files (or JpegScans of parse_jpeg) -> a list of uint8 tensors (H, W, C) on `device`,
  the shape tf.image.decode_jpeg gives.  channels: 0 = the file's, 3 replicates a grey file, 1 gives
  the Y plane of a colour file at full size.  Mixed geometries share the call: the tables and the
  entropy bytes of all files go up in one pinned buffer and one copy, and `se3ds_jpeg_decode` queues
  a memset and three launches on the current stream.  check=True reads the status words back (one
  synchronisation) and raises ValueError naming the image and the reason; check=False returns
  (tensors, PendingJpegDecode)."""
  dev = cuda_device(device, 'decode_jpeg_batch', 'decodes')
  if len(bufs) == 0:
    raise ValueError('decode_jpeg_batch: nothing to decode')
  batch = JpegBatch([b if isinstance(b, JpegScan) else parse_jpeg(b) for b in bufs], dev, channels)
  batch.launch(7)
  pending = batch.pending()
  if not check:
    return batch.out, pending
  pending.check()
  return batch.out


# ------------------------------------------------------------------------------ encoding
# ITU-T T.81 Annex K.1, K.2: the quantisation tables libjpeg scales, row-major order
_LUMA_QUANT = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                        69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55,
                        64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103,
                        99], np.int64)
_CHROMA_QUANT = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                          99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
# Annex K.3: (counts per code length 1..16, values) of DC luma, AC luma, DC chroma, AC chroma
_AC_VALUES = (
    '01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 '
    '82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 '
    '5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 '
    'a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 '
    'e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa',
    '00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 '
    '0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 '
    '59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a '
    'a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da '
    'e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa')
HUFFMAN_TABLES = (
    (0x00, bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0x10, bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), bytes.fromhex(_AC_VALUES[0])),
    (0x01, bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0x11, bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), bytes.fromhex(_AC_VALUES[1])),
)
_SUBSAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}


def quality_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
  """(luma, chroma) quantisation tables, int64 (64,) in row-major order, of libjpeg's
  jpeg_set_quality(quality, force_baseline=TRUE): the Annex K tables times 5000 / q percent below
  50 and 200 - 2 q percent from 50 on, rounded, clamped to 1..255."""
  q = _quality(quality)
  scale = 5000 // q if q < 50 else 200 - 2 * q
  return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (_LUMA_QUANT, _CHROMA_QUANT))


def _quality(q) -> int:
  if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= int(q) <= 100:
    raise ValueError(f'quality: an int 1..100, got {q!r}')
  return int(q)


def _marker_segment(marker: int, body: bytes) -> bytes:
  return bytes([0xFF, marker]) + struct.pack('>H', 2 + len(body)) + body


def jpeg_container(height: int, width: int, components: int, h0: int, v0: int, tables, restart_interval: int,
                   entropy_coded: bytes) -> bytes:
  """The file around the entropy-coded bytes of se3ds_jpeg_encode, as libjpeg lays it out: SOI, APP0
  (JFIF 1.01, density 1 x 1 without unit, no thumbnail), one DQT per table, SOF0 (components 1, 2,
  3; luma h0 x v0, chroma 1 x 1 on table 1), DHT for DC 0, AC 0, DC 1, AC 1 (the first two alone for
  grey), DRI if the interval is not 0, SOS, the data, EOI.  tables: (luma, chroma) in row-major
  order."""
  if components not in (1, 3) or (components == 1 and (h0, v0) != (1, 1)):
    raise ValueError(f'jpeg_container: {components} component(s) at sampling {h0} x {v0}')
  out = [b'\xff\xd8', _marker_segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))]
  for tq in range(2 if components == 3 else 1):
    out.append(_marker_segment(0xDB, bytes([tq]) + bytes(int(v) for v in np.asarray(tables[tq])[ZIGZAG])))
  out.append(_marker_segment(0xC0, struct.pack('>BHHB', 8, height, width, components) + b''.join(
      bytes([i + 1, ((h0 << 4) | v0) if i == 0 else 0x11, min(i, 1)]) for i in range(components))))
  for tag, counts, values in HUFFMAN_TABLES[:2 * min(components, 2)]:
    out.append(_marker_segment(0xC4, bytes([tag]) + counts + values))
  if restart_interval:
    out.append(_marker_segment(0xDD, struct.pack('>H', restart_interval)))
  out.append(_marker_segment(0xDA, bytes([components]) + b''.join(
      bytes([i + 1, 0x11 * min(i, 1)]) for i in range(components)) + b'\x00\x3f\x00'))
  return b''.join(out) + bytes(entropy_coded) + b'\xff\xd9'


class EncodeSpec(NamedTuple):
  """What one image of encode_jpeg_batch becomes: geometry, sampling, tables, restart interval."""
  height: int
  width: int
  components: int
  h0: int
  v0: int
  tables: Tuple[np.ndarray, np.ndarray]
  restart_interval: int

  @property
  def blocks(self):
    mcus = -(-self.width // (8 * self.h0)) * -(-self.height // (8 * self.v0))
    return mcus * (1 if self.components == 1 else self.h0 * self.v0 + 2)


def encode_specs(shapes, dtypes, quality=75, subsampling='4:2:0', restart_interval=0) -> List[EncodeSpec]:
  """The argument checks of encode_jpeg_batch (no device needed): ValueError naming the argument."""
  n = len(shapes)
  if isinstance(quality, (list, tuple, np.ndarray)):
    if len(quality) != n:
      raise ValueError(f'quality: {len(quality)} entries for {n} images')
    qualities = [_quality(q) for q in quality]
  else:
    qualities = [_quality(quality)] * n
  if subsampling not in _SUBSAMPLING:
    raise ValueError(f"subsampling: '4:4:4', '4:2:2' or '4:2:0', got {subsampling!r}")
  row = restart_interval == 'row'
  if not row and (isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer)) or
                  not 0 <= int(restart_interval) <= 65535):
    raise ValueError(f"restart_interval: MCUs 0..65535 or 'row', got {restart_interval!r}")
  specs = []
  for shape, dtype, q in zip(shapes, dtypes, qualities):
    if len(shape) != 3 or shape[2] not in (1, 3) or shape[0] < 1 or shape[1] < 1 or dtype != torch.uint8:
      raise ValueError(f'images: uint8 (H,W,1) or (H,W,3) expected, got {dtype} {tuple(shape)}')
    if shape[0] > 65535 or shape[1] > 65535:
      raise ValueError(f'images: a JPEG file holds at most 65535 x 65535 pixels, got {tuple(shape)}')
    h0, v0 = (1, 1) if shape[2] == 1 else _SUBSAMPLING[subsampling]
    interval = -(-int(shape[1]) // (8 * h0)) if row else int(restart_interval)
    specs.append(EncodeSpec(int(shape[0]), int(shape[1]), int(shape[2]), h0, v0, quality_tables(q), interval))
  return specs


class JpegEncodeBatch:
  """The table, the workspace and the output buffer of one batch on the current stream of the
  images' device: `launch(phases)` queues `se3ds_jpeg_encode` (the timing tool launches the phases
  apart), `files()` reads the sizes and then the bytes in use back and adds the containers."""

  def __init__(self, images: Sequence[torch.Tensor], specs: Sequence[EncodeSpec]):
    L = _lib.lib()
    n = len(images)
    self.images, self.specs, self.device = images, specs, images[0].device
    table = np.zeros((n, L.se3ds_jpeg_encode_fields()), np.int64)
    blocks = tiles = 0
    tile_blocks = L.se3ds_jpeg_encode_tile_blocks()
    for i, (x, s) in enumerate(zip(images, specs)):
      table[i, :9] = (x.data_ptr(), s.width, s.height, s.components, s.h0, s.v0, s.restart_interval, blocks, tiles)
      table[i, 16:].view(np.uint16)[:] = np.concatenate(s.tables)
      blocks += s.blocks
      mcus_x, mcus_y = -(-s.width // (8 * s.h0)), -(-s.height // (8 * s.v0))
      tiles += mcus_y * -(-mcus_x // (tile_blocks // (s.blocks // (mcus_x * mcus_y))))
    self.table = table
    self.workspace_bytes = L.se3ds_jpeg_encode_workspace_bytes(table.ctypes.data, n)
    self.out_bytes = L.se3ds_jpeg_encode_out_bytes(table.ctypes.data, n)
    with torch.cuda.device(self.device):
      self.table_dev, _ = upload([table], self.device)
      self.workspace = torch.empty((max(self.workspace_bytes, 16),), dtype=torch.uint8, device=self.device)
      self.out = torch.empty((max(self.out_bytes, 16),), dtype=torch.uint8, device=self.device)
      self.sizes = torch.empty((n + 1,), dtype=torch.int64, device=self.device)

  def launch(self, phases: int = 15) -> None:
    with torch.cuda.device(self.device):
      rc = _lib.lib().se3ds_jpeg_encode(
          _lib.ptr(self.table_dev), self.table.ctypes.data, len(self.table), _lib.ptr(self.workspace),
          self.workspace_bytes, _lib.ptr(self.out), self.out_bytes, _lib.ptr(self.sizes), phases, _lib.stream())
    _lib.check(rc, 'se3ds_jpeg_encode')

  def entropy_coded(self) -> List[bytes]:
    """Every image's bytes between the SOS header and EOI.  The output buffer is a worst-case bound,
    so the n + 1 offsets come back first and then only the bytes in use."""
    starts = Readback(self.sizes).wait()
    data = Readback(self.out[:max(int(starts[-1]), 1)]).wait()
    return [data[int(a):int(b)].tobytes() for a, b in zip(starts[:-1], starts[1:])]

  def files(self) -> List[bytes]:
    return [jpeg_container(s.height, s.width, s.components, s.h0, s.v0, s.tables, s.restart_interval, data)
            for s, data in zip(self.specs, self.entropy_coded())]


def encode_jpeg_batch(images: Sequence[torch.Tensor], quality=75, subsampling='4:2:0', restart_interval=0,
                      device=None) -> List[bytes]:
  """uint8 device tensors (H,W,1|3), any mix of sizes -> their baseline JPEG files, the bytes Pillow's
  Image.save(f, 'JPEG', quality=q, subsampling=s) writes: one upload (the table), the launches of
  `se3ds_jpeg_encode` (csrc/jpeg_encode.hip: transform, measure + scan, pack), the offsets and the
  packed bytes back; the host adds the container (jpeg_container).
  quality: an int 1..100 or a sequence with one per image.  subsampling: '4:4:4', '4:2:2' or
  '4:2:0'; a one-channel image is a grey file and ignores it.  restart_interval: MCUs per restart
  interval, 0 = none, 'row' = one MCU row (a file whose segments decode_jpeg_batch spreads over
  workgroups).  device: where the tensors must be (None: where the first one is).  Bad arguments
  raise ValueError naming the argument; a non-CUDA tensor raises Se3dsHipError: there is no CPU
  encoder.
  Memory: the workspace (346 B a block) and the output buffer (416 B a block, every block at its
  longest and every byte stuffed) are sized for the worst case and allocated per call: 0.15 GB for
  one 2048 x 4096 image at 4:2:0, 1.35 GB for nine of them, to emit a few MB.  Only the bytes in
  use come back: the n + 1 offsets first, then out[:offsets[n]]."""
  images = list(images)
  if not images:
    return []
  specs = encode_specs([x.shape for x in images], [x.dtype for x in images], quality, subsampling,
                       restart_interval)
  dev = images[0].device if device is None else torch.device(device)
  for x in images:
    if x.device.type != dev.type or (dev.index is not None and x.device.index != dev.index):
      raise ValueError(f'images: a tensor on {x.device} in a batch on {dev}')
  _lib.require_cuda(*images)
  batch = JpegEncodeBatch([x.contiguous() for x in images], specs)
  batch.launch(15)
  return batch.files()
