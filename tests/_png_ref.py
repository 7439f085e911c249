"""Test-side PNG reference: a per-byte reconstruction written from the PNG specification's
definitions (section 9.2 filter types, 9.4 Paeth predictor), the matching per-row filter, and an
encoder that applies a chosen filter type to each row.  Plain loops: it only ever sees tiny images.
Pinned by hand-worked literals in tests/test_png_container.py."""
import struct
import zlib

import numpy as np


def paeth_predictor(a: int, b: int, c: int) -> int:
  p = a + b - c
  pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
  if pa <= pb and pa <= pc:
    return a
  if pb <= pc:
    return b
  return c


def _predict(ft: int, a: int, b: int, c: int) -> int:
  if ft == 0:
    return 0
  if ft == 1:
    return a
  if ft == 2:
    return b
  if ft == 3:
    return (a + b) >> 1
  if ft == 4:
    return paeth_predictor(a, b, c)
  raise ValueError(f'filter type {ft}')


def reconstruct(filtered: bytes, height: int, row_bytes: int, bpp: int) -> np.ndarray:
  """Filtered scan lines (type byte + row_bytes each) -> uint8 (height, row_bytes)."""
  assert len(filtered) == height * (1 + row_bytes)
  out = [[0] * row_bytes for _ in range(height)]
  for y in range(height):
    base = y * (1 + row_bytes)
    ft = filtered[base]
    for i in range(row_bytes):
      a = out[y][i - bpp] if i >= bpp else 0
      b = out[y - 1][i] if y > 0 else 0
      c = out[y - 1][i - bpp] if (y > 0 and i >= bpp) else 0
      out[y][i] = (filtered[base + 1 + i] + _predict(ft, a, b, c)) & 0xff
  return np.array(out, np.uint8).reshape(height, row_bytes)


def apply_filters(raw: np.ndarray, filter_types, bpp: int) -> bytes:
  """uint8 (height, row_bytes) -> filtered scan lines, row y filtered with filter_types[y]."""
  height, row_bytes = raw.shape
  rows = raw.tolist()
  out = bytearray()
  for y in range(height):
    ft = int(filter_types[y])
    out.append(ft)
    for i in range(row_bytes):
      a = rows[y][i - bpp] if i >= bpp else 0
      b = rows[y - 1][i] if y > 0 else 0
      c = rows[y - 1][i - bpp] if (y > 0 and i >= bpp) else 0
      out.append((rows[y][i] - _predict(ft, a, b, c)) & 0xff)
  return bytes(out)


def chunk(tag: bytes, data: bytes) -> bytes:
  return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data))


def container(width: int, height: int, bit_depth: int, colour_type: int, filtered: bytes,
              idat_split: int = 1, interlace: int = 0, extra=()) -> bytes:
  """A PNG file around an already filtered stream; idat_split: number of IDAT chunks; extra:
  (tag, data) chunks placed between IHDR and the first IDAT."""
  z = zlib.compress(filtered, 6)
  step = max(1, -(-len(z) // idat_split))
  parts = [z[i:i + step] for i in range(0, len(z), step)]
  return (b'\x89PNG\r\n\x1a\n' +
          chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, bit_depth, colour_type, 0, 0,
                                     interlace)) +
          b''.join(chunk(t, d) for t, d in extra) +
          b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b''))


def raw_bytes(pixels: np.ndarray) -> np.ndarray:
  """uint8 (H,W) / (H,W,3) or uint16 (H,W) pixels -> the PNG's big-endian byte rows (H, row_bytes)."""
  if pixels.dtype == np.uint16:
    return pixels.astype('>u2').view(np.uint8).reshape(pixels.shape[0], -1)
  assert pixels.dtype == np.uint8
  return pixels.reshape(pixels.shape[0], -1)


def encode_png(pixels: np.ndarray, filter_types, idat_split: int = 1) -> bytes:
  """uint8 (H,W) grey, uint8 (H,W,3) RGB or uint16 (H,W) grey -> PNG with the given row filters."""
  h, w = pixels.shape[:2]
  depth = 16 if pixels.dtype == np.uint16 else 8
  colour = 2 if pixels.ndim == 3 else 0
  bpp = (3 if colour == 2 else 1) * depth // 8
  return container(w, h, depth, colour, apply_filters(raw_bytes(pixels), filter_types, bpp),
                   idat_split)


def decode_png(filtered: bytes, height: int, width: int, bit_depth: int, channels: int) -> np.ndarray:
  """The reference decode of one plane: uint8 (H,W[,3]) or uint16 (H,W) values."""
  bpp = channels * bit_depth // 8
  rows = reconstruct(filtered, height, width * bpp, bpp)
  if bit_depth == 16:
    pairs = rows.reshape(height, width, 2).astype(np.uint16)
    return pairs[..., 0] * np.uint16(256) + pairs[..., 1]
  return rows.reshape((height, width, 3) if channels == 3 else (height, width))
