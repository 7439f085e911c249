"""The animated-GIF format of DESIGN.md 3.18 restated in plain Python and NumPy for the tests:
median cut, look-up table, ordered dither, strip-wise LZW, sub-blocks, container -- and an LZW
decoder and container walk to read files back.  Imports nothing from se3ds_amd."""
import struct

import numpy as np

STRIP_PIXELS = 16384


def bayer8():
  m = np.array([[0, 2], [3, 1]])
  while m.shape[0] < 8:
    m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
  return m


def strip_rows(width):
  return max(1, -(-STRIP_PIXELS // width))


def slot_bits_bound(pixels):
  """What the issue states: 12 bits a pixel, the clears, the framing codes."""
  return 12 * (pixels + pixels // 3838 + 2)


# ------------------------------------------------------------------------------------ palette
def grey_palette():
  return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def histogram(video):
  v = video.reshape(-1, 3).astype(np.int64) >> 3
  return np.bincount(v[:, 0] << 10 | v[:, 1] << 5 | v[:, 2], minlength=32768).astype(np.uint32)


def _coords(bins):
  return np.stack([bins >> 10, bins >> 5 & 31, bins & 31], axis=1)


def median_cut(hist):
  hist = np.asarray(hist).astype(np.int64)
  boxes = [np.flatnonzero(hist)]
  while len(boxes) < 256:
    pick, best = -1, -1
    for i, b in enumerate(boxes):
      if len(b) >= 2:
        total = sum(hist[b].tolist())   # Python integers
        if total > best:
          pick, best = i, total
    if pick < 0:
      break
    b = boxes[pick]
    co = _coords(b)
    extent = co.max(axis=0) - co.min(axis=0)
    axis = max((1, 0, 2), key=lambda a: extent[a])   # max keeps the first of equals: g, r, b
    order = sorted(range(len(b)), key=lambda j: (co[j, axis], b[j]))
    b = b[order]
    total, run, k = int(hist[b].sum()), 0, 0
    for j in range(len(b)):
      run += int(hist[b[j]])
      k = j + 1
      if run >= (total + 1) // 2:
        break
    k = min(max(k, 1), len(b) - 1)
    boxes[pick] = b[:k]
    boxes.append(b[k:])
  palette = np.zeros((256, 3), np.uint8)
  for i, b in enumerate(boxes):
    total = sum(int(hist[j]) for j in b)
    co = _coords(b)
    for ch in range(3):
      s = sum(int(hist[j]) * (8 * int(co[n, ch]) + 4) for n, j in enumerate(b))
      palette[i, ch] = (s + total // 2) // total
  return palette, len(boxes)


def nearest_lut(palette, n_used):
  bins = np.arange(32768)
  centres = 8 * _coords(bins) + 4
  pal = palette[:n_used].astype(np.int64)
  lut = np.empty(32768, np.uint8)
  for at in range(0, 32768, 4096):
    d = ((centres[at:at + 4096, None, :] - pal[None, :, :]) ** 2).sum(axis=2)
    lut[at:at + 4096] = d.argmin(axis=1)   # the first of equals
  return lut


def index_plane(video, lut, dither):
  t, h, w, _ = video.shape
  d = bayer8()[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7]
  off = ((d * dither) >> 6) - (dither >> 1)
  v = np.clip(video.astype(np.int64) + off[None, :, :, None], 0, 255) >> 3
  return lut[v[..., 0] << 10 | v[..., 1] << 5 | v[..., 2]]


def quantise(video, dither=32):
  """(T,H,W,1|3) uint8 -> (palette (256,3) uint8, index (T,H,W) uint8)."""
  if video.shape[3] == 1:
    return grey_palette(), video[..., 0].copy()
  palette, used = median_cut(histogram(video))
  return palette, index_plane(video, nearest_lut(palette, used), dither)


# ---------------------------------------------------------------------------------------- LZW
def strip_codes(px, first, last):
  """[(code, width)] of one strip, the issue's pseudocode line by line."""
  out = []
  width, nxt, table = 9, 258, {}
  if first:
    out.append((256, 9))
  prefix = int(px[0])
  for c in px[1:]:
    c = int(c)
    if (prefix, c) in table:
      prefix = table[(prefix, c)]
      continue
    out.append((prefix, width))
    if nxt < 4096:
      table[(prefix, c)] = nxt
      if nxt == (1 << width) and width < 12:
        width += 1
      nxt += 1
    else:
      out.append((256, width))
      table, width, nxt = {}, 9, 258
    prefix = c
  out.append((prefix, width))
  if nxt < 4096:
    if nxt == (1 << width) and width < 12:
      width += 1
    nxt += 1
  out.append((257 if last else 256, width))
  return out


def pack_codes(codes):
  """-> (bytes with the last one zero-padded, bits)."""
  out, total, acc, bits = bytearray(), 0, 0, 0
  for code, width in codes:
    acc |= code << bits
    bits += width
    total += width
    while bits >= 8:
      out.append(acc & 255)
      acc >>= 8
      bits -= 8
  if bits:
    out.append(acc)
  return bytes(out), total


def frame_data(index):
  """(H,W) uint8 -> the frame's LZW bytes: its strips' codes back to back."""
  h, w = index.shape
  rows = strip_rows(w)
  starts = list(range(0, h, rows))
  codes = []
  for i, r in enumerate(starts):
    codes += strip_codes(index[r:r + rows].reshape(-1), i == 0, i == len(starts) - 1)
  return pack_codes(codes)[0]


def sub_blocks(data):
  out = b''
  for at in range(0, len(data), 255):
    part = data[at:at + 255]
    out += bytes([len(part)]) + part
  return out + b'\x00'


def delay_cs(fps):
  return max(2, int(100 / fps + 0.5))


def container(width, height, palette, frames, fps=10, loop=0):
  out = b'GIF89a' + struct.pack('<HH', width, height) + b'\xf7\x00\x00' + palette.astype(np.uint8).tobytes()
  if loop is not None:
    out += b'\x21\xff\x0bNETSCAPE2.0\x03\x01' + struct.pack('<H', loop) + b'\x00'
  for blocks in frames:
    out += b'\x21\xf9\x04\x04' + struct.pack('<H', delay_cs(fps)) + b'\x00\x00'
    out += b'\x2c\x00\x00\x00\x00' + struct.pack('<HH', width, height) + b'\x00' + b'\x08' + blocks
  return out + b'\x3b'


def encode(video, fps=10, loop=0, dither=32):
  palette, index = quantise(video, dither)
  t, h, w = index.shape
  return container(w, h, palette, [sub_blocks(frame_data(index[i])) for i in range(t)], fps, loop)


# ------------------------------------------------------------------------------------- decode
def lzw_decode(data):
  """GIF LZW at minimum code size 8 -> uint8 indices, up to the end code."""
  acc = have = pos = 0
  out = []
  table, width, nxt, prev = {}, 9, 258, None
  while True:
    while have < width:
      assert pos < len(data), 'the stream ends without an end code'
      acc |= data[pos] << have
      pos += 1
      have += 8
    code = acc & ((1 << width) - 1)
    acc >>= width
    have -= width
    if code == 256:
      table, width, nxt, prev = {}, 9, 258, None
      continue
    if code == 257:
      break
    if prev is None:
      assert code < 256, code
      entry = [code]
    else:
      before = table[prev] if prev >= 258 else [prev]
      if code < 256:
        entry = [code]
      elif code < nxt:
        entry = table[code]
      else:
        assert code == nxt, (code, nxt)
        entry = before + [before[0]]
      if nxt < 4096:
        table[nxt] = before + [entry[0]]
        nxt += 1
        if nxt == (1 << width) and width < 12:
          width += 1
    out += entry
    prev = code
  assert pos == len(data) and acc == 0, 'bits behind the end code'
  return np.array(out, np.uint8)


def decode_file(buf):
  """-> dict(width, height, palette (256,3), loop (None or int), delays [cs], frames (T,H,W) indices,
  blocks [[sub-block lengths]])."""
  assert buf[:6] == b'GIF89a'
  w, h = struct.unpack('<HH', buf[6:10])
  assert buf[10:13] == b'\xf7\x00\x00'
  palette = np.frombuffer(buf[13:13 + 768], np.uint8).reshape(256, 3)
  p, loop, delays, frames, blocks = 13 + 768, None, [], [], []
  while buf[p] != 0x3b:
    if buf[p:p + 3] == b'\x21\xff\x0b':
      assert buf[p + 3:p + 16] == b'NETSCAPE2.0\x03\x01' and buf[p + 18] == 0
      loop, = struct.unpack('<H', buf[p + 16:p + 18])
      p += 19
    elif buf[p:p + 4] == b'\x21\xf9\x04\x04':
      delays.append(struct.unpack('<H', buf[p + 4:p + 6])[0])
      assert buf[p + 6:p + 8] == b'\x00\x00'
      p += 8
    else:
      assert buf[p:p + 5] == b'\x2c\x00\x00\x00\x00', buf[p:p + 5]
      assert struct.unpack('<HH', buf[p + 5:p + 9]) == (w, h) and buf[p + 9:p + 11] == b'\x00\x08'
      p += 11
      data, sizes = b'', []
      while buf[p]:
        sizes.append(buf[p])
        data += buf[p + 1:p + 1 + buf[p]]
        p += 1 + buf[p]
      p += 1
      px = lzw_decode(data)
      assert px.size == w * h, (px.size, w, h)
      frames.append(px.reshape(h, w))
      blocks.append(sizes)
  assert p == len(buf) - 1
  return dict(width=w, height=h, palette=palette, loop=loop, delays=delays, frames=np.stack(frames), blocks=blocks)


# ---------------------------------------------------------------------------------- test scenes
def noise(shape, seed):
  return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def synthetic_frame(h=96, w=128, seed=5):
  """Smooth gradients plus a noisy patch, (h,w,3) uint8."""
  y, x = np.mgrid[0:h, 0:w]
  px = np.stack([255 * x // (w - 1), 255 * y // (h - 1), 255 * (x + y) // (w + h - 2)], axis=2).astype(np.uint8)
  px[h // 4:h // 2, w // 4:w // 2] = noise((h // 2 - h // 4, w // 2 - w // 4, 3), seed)
  return px
