"""The JPEG encoder's oracle, NumPy only: libjpeg's default baseline encoder restated from its
specification -- what Pillow's Image.save(f, 'JPEG', quality=q, subsampling=s) runs -- vectorised
over blocks.  tests/test_jpeg_encode_cpu.py pins it against Pillow byte for byte; the device encoder
(utils/jpeg.py encode_jpeg_batch, csrc/jpeg_encode_core.h) is tested against it.  It shares nothing
with the package but the specification; the Annex K Huffman tables, the zig-zag order and the bit
packer come from tests/_jpeg_ref.py.

  quality_tables   jpeg_set_quality(q, force_baseline=TRUE) on the Annex K quantisation tables
  coefficients     pixels -> per component (block rows, block columns, 64) quantised coefficients in
                   row-major order, whole MCUs, dummy blocks as libjpeg fills them
  entropy          coefficients -> the bytes between SOS and EOI (stuffed, RSTn, 1-padded)
  encode           pixels -> the file
"""
import struct

import numpy as np

from _jpeg_ref import ANNEX_K, SAMPLINGS, ZZ, _pack, code_book

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113,
                 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
SUBSAMPLING = {'4:4:4': '444', '4:2:2': '422', '4:2:0': '420'}


def quality_tables(q: int):
  """(luma, chroma) int64 (64,) in row-major order."""
  scale = 5000 // q if q < 50 else 200 - 2 * q
  return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA, CHROMA))


def _fix(x):
  return int(x * 65536 + 0.5)


def ycc(rgb):
  r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
  y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
  cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
  cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
  return y, cb, cr


def _edge(a, rows, cols):
  return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode='edge')


def planes(pixels, sampling):
  """The component planes, whole MCUs: columns replicated at full resolution, rows at full resolution
  up to the vertical factor only, then the last downsampled row."""
  nc, h0, v0 = SAMPLINGS[sampling]
  h, w = pixels.shape[:2]
  mx, my = -(-w // (8 * h0)), -(-h // (8 * v0))
  if nc == 1:
    return [_edge(pixels.reshape(h, w).astype(np.int64), my * 8, mx * 8)]
  y, cb, cr = ycc(pixels)
  out = [_edge(y, my * 8 * v0, mx * 8 * h0)]
  for c in (cb, cr):
    c = _edge(c, -(-h // v0) * v0, mx * 8 * h0)
    if h0 == 2 and v0 == 1:
      c = (c[:, 0::2] + c[:, 1::2] + (np.arange(c.shape[1] // 2) & 1)) >> 1
    elif h0 == 2:
      c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 1 + (np.arange(c.shape[1] // 2) & 1)) >> 2
    out.append(_edge(c, my * 8, mx * 8))
  return out


def _pass(d, shift_same, shift_odd, rows):
  """jfdctint, one pass over the last axis of d (..., 8)."""
  d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
  t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
  t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
  ds = lambda x: (x + (1 << (shift_odd - 1))) >> shift_odd
  if rows:
    o0, o4 = (t10 + t11) << shift_same, (t10 - t11) << shift_same
  else:
    o0, o4 = (t10 + t11 + (1 << (shift_same - 1))) >> shift_same, (t10 - t11 + (1 << (shift_same - 1))) >> shift_same
  z1 = (t12 + t13) * 4433
  o2, o6 = ds(z1 + t13 * 6270), ds(z1 - t12 * 15137)
  z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
  z5 = (z3 + z4) * 9633
  a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
  z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
  return np.stack([o0, ds(a7 + z1 + z4), o2, ds(a6 + z2 + z3), o4, ds(a5 + z2 + z4), o6, ds(a4 + z1 + z3)], -1)


def fdct(blocks):
  """(..., 8, 8) samples -> (..., 8, 8) coefficients scaled by 8."""
  d = _pass(blocks.astype(np.int64) - 128, 2, 11, True)
  return np.swapaxes(_pass(np.swapaxes(d, -1, -2), 2, 15, False), -1, -2)


def quantise(c, q):
  d = 8 * q
  return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(pixels, quality, sampling):
  """pixels uint8 (H, W, 1|3) -> [per component (block rows, block columns, 64) int64], (luma, chroma)
  tables."""
  nc, h0, v0 = SAMPLINGS[sampling]
  assert pixels.shape[2] == nc
  h, w = pixels.shape[:2]
  tables = quality_tables(quality)
  out = []
  for ci, p in enumerate(planes(pixels, sampling)):
    rows, cols = p.shape[0] // 8, p.shape[1] // 8
    blocks = p.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
    q = quantise(fdct(blocks).reshape(rows, cols, 64), tables[min(ci, 1)])
    if ci == 0 and nc == 3:
      real_cols, real_rows = -(-w // 8), -(-h // 8)
      for col in range(real_cols, cols):   # at most one: its left neighbour's DC
        q[:, col, 1:] = 0
        q[:, col, 0] = q[:, col - 1, 0]
      for row in range(real_rows, rows):   # at most one: the DC of the MCU's upper-right block
        q[row, :, 1:] = 0
        q[row, :, 0] = np.repeat(q[row - 1, h0 - 1::h0, 0], h0)
    out.append(q)
  return out, tables


def scan_order(coefs, sampling):
  """-> (blocks (N, 64) in scan order, component of each, MCU of each)."""
  nc, h0, v0 = SAMPLINGS[sampling]
  my, mx = coefs[-1].shape[:2]
  if nc == 1:
    n = my * mx
    return coefs[0].reshape(n, 64), np.zeros(n, np.int64), np.arange(n)
  luma = coefs[0].reshape(my, v0, mx, h0, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, h0 * v0, 64)
  per = np.concatenate([luma, coefs[1].reshape(my * mx, 1, 64), coefs[2].reshape(my * mx, 1, 64)], 1)
  slots = h0 * v0 + 2
  comp = np.tile(np.array([0] * (h0 * v0) + [1, 2]), my * mx)
  return per.reshape(-1, 64), comp, np.repeat(np.arange(my * mx), slots)


_BOOKS = {key: code_book(*ANNEX_K[key]) for key in ANNEX_K}


def _table(tc, th, size):
  code, length = np.zeros(size, np.int64), np.zeros(size, np.int64)
  for sym, (c, l) in _BOOKS[(tc, th)].items():
    code[sym], length[sym] = c, l
  return code, length


_DC = [_table(0, 0, 12), _table(0, 1, 12)]
_AC = [_table(1, 0, 256), _table(1, 1, 256)]


def _category(v):
  a, n = np.abs(v), np.zeros(v.shape, np.int64)
  for k in range(12):
    n += a >= (1 << k)
  return n


def symbols(blocks, comp, mcu, restart):
  """Every block's (value, length) pairs, vectorised: -> (values, lengths, block of each), in
  stream order."""
  n = blocks.shape[0]
  z = blocks[:, ZZ]
  tab = np.minimum(comp, 1)
  seg = mcu // restart if restart else np.zeros(n, np.int64)
  # the DC predictor: the previous block of the component inside the segment
  diff = z[:, 0].copy()
  for c in np.unique(comp):
    idx = np.flatnonzero(comp == c)
    prev = np.concatenate([[0], z[idx[:-1], 0]])
    prev[np.concatenate([[True], seg[idx[1:]] != seg[idx[:-1]]])] = 0
    diff[idx] -= prev
  # slots: per block 65 positions (DC, 63 AC, EOB) x 4 (three ZRLs, the symbol)
  vals, lens = np.zeros((n, 65, 4), np.int64), np.zeros((n, 65, 4), np.int64)
  cat = _category(diff)
  extra = np.where(diff < 0, diff + (1 << cat) - 1, diff)
  for t in (0, 1):
    m = tab == t
    vals[m, 0, 3] = (_DC[t][0][cat[m]] << cat[m]) | extra[m]
    lens[m, 0, 3] = _DC[t][1][cat[m]] + cat[m]
  ac = z[:, 1:]
  nz = ac != 0
  pos = np.arange(1, 64)[None, :]
  last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)          # last non-zero at or before k
  before = np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], 1)
  run = pos - before - 1
  cat = _category(ac)
  extra = np.where(ac < 0, ac + (1 << cat) - 1, ac)
  for t in (0, 1):
    m = (tab == t)[:, None] & nz
    b, k = np.nonzero(m)
    sym = ((run[b, k] & 15) << 4) | cat[b, k]
    vals[b, k + 1, 3] = (_AC[t][0][sym] << cat[b, k]) | extra[b, k]
    lens[b, k + 1, 3] = _AC[t][1][sym] + cat[b, k]
    for j in range(3):
      zb, zk = b[run[b, k] >= 16 * (j + 1)], k[run[b, k] >= 16 * (j + 1)]
      vals[zb, zk + 1, j], lens[zb, zk + 1, j] = _AC[t][0][0xF0], _AC[t][1][0xF0]
    eob = (tab == t) & (last[:, -1] < 63)
    vals[eob, 64, 3], lens[eob, 64, 3] = _AC[t][0][0], _AC[t][1][0]
  keep = lens.reshape(-1) > 0
  owner = np.repeat(np.arange(n), 65 * 4)[keep]
  return vals.reshape(-1)[keep], lens.reshape(-1)[keep], owner


def entropy(coefs, sampling, restart=0):
  """The bytes between the SOS header and EOI."""
  blocks, comp, mcu = scan_order(coefs, sampling)
  vals, lens, owner = symbols(blocks, comp, mcu, restart)
  if not restart:
    return _pack(vals, lens)[0]
  seg = mcu[owner] // restart
  cuts = np.flatnonzero(np.diff(seg)) + 1
  out = bytearray()
  for i, (a, b) in enumerate(zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(vals)]]))):
    if i:
      out += bytes([0xFF, 0xD0 + (i - 1) % 8])
    out += _pack(vals[a:b], lens[a:b])[0]
  return bytes(out)


def container(height, width, sampling, tables, restart, data):
  nc, h0, v0 = SAMPLINGS[sampling]
  seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack('>H', 2 + len(body)) + body
  out = b'\xff\xd8' + seg(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
  for tq in range(2 if nc == 3 else 1):
    out += seg(0xDB, bytes([tq]) + bytes(int(v) for v in np.asarray(tables[tq])[ZZ]))
  out += seg(0xC0, struct.pack('>BHHB', 8, height, width, nc) + b''.join(
      bytes([i + 1, ((h0 << 4) | v0) if i == 0 else 0x11, min(i, 1)]) for i in range(nc)))
  for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1))[:2 * min(nc, 2)]:
    counts, values = ANNEX_K[(tc, th)]
    out += seg(0xC4, bytes([(tc << 4) | th]) + bytes(counts) + bytes(values))
  if restart:
    out += seg(0xDD, struct.pack('>H', restart))
  out += seg(0xDA, bytes([nc]) + b''.join(bytes([i + 1, 0x11 * min(i, 1)]) for i in range(nc)) + b'\x00\x3f\x00')
  return out + data + b'\xff\xd9'


def restart_mcus(restart, width, sampling):
  """'row' -> the MCUs of one MCU row."""
  return -(-width // (8 * SAMPLINGS[sampling][1])) if restart == 'row' else int(restart)


def encode(pixels, quality=75, subsampling='4:2:0', restart=0):
  """uint8 (H, W, 1|3) -> the file.  A one-channel image is a grey file."""
  pixels = np.asarray(pixels)
  sampling = 'grey' if pixels.shape[2] == 1 else SUBSAMPLING[subsampling]
  restart = restart_mcus(restart, pixels.shape[1], sampling)
  coefs, tables = coefficients(pixels, quality, sampling)
  return container(pixels.shape[0], pixels.shape[1], sampling, tables, restart, entropy(coefs, sampling, restart))


def scene(kind, h, w, c, seed=0):
  """The test pictures: smooth, noise, smooth + noise, constant, a 0/255 checkerboard."""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  smooth = np.stack([127.5 + 127.5 * np.sin(0.07 * (k + 1) * xx + 0.05 * (3 - k) * yy + k) for k in range(c)], -1)
  if kind == 'smooth':
    a = smooth
  elif kind == 'noise':
    a = rng.integers(0, 256, (h, w, c))
  elif kind == 'mixed':
    a = smooth + rng.normal(0, 12, (h, w, c))
  elif kind == 'constant':
    a = np.full((h, w, c), 93)
  elif kind == 'checker':
    a = np.repeat((((yy + xx) & 1) * 255)[..., None], c, -1)
  else:
    raise ValueError(kind)
  return np.clip(np.rint(a), 0, 255).astype(np.uint8)


# ------------------------------------------------------------- tools/jpeg_encode_host_check.cpp
def table_row(height, width, sampling, tables, restart):
  """One row of se3ds_jpeg_encode's table (csrc/jpeg_encode_core.h `struct Image`), without the
  pointer and the running sum: int64 (48,)."""
  nc, h0, v0 = SAMPLINGS[sampling]
  row = np.zeros(48, np.int64)
  row[1:7] = (width, height, nc, h0, v0, restart)
  row[16:].view(np.uint16)[:] = np.concatenate([np.asarray(t) for t in tables]).astype(np.uint16)
  return row


def corpus_cases():
  """(pixels, quality, subsampling, restart): every sampling, dummy blocks, restarts, long blocks."""
  cases = []
  for i, (h, w) in enumerate([(1, 1), (2, 3), (8, 17), (9, 20), (20, 9), (33, 47), (40, 40), (17, 250), (64, 96)]):
    for j, (sub, c) in enumerate([('4:2:0', 1), ('4:4:4', 3), ('4:2:2', 3), ('4:2:0', 3)]):
      kind = ('smooth', 'noise', 'mixed', 'constant', 'checker')[(i + j) % 5]
      cases.append((scene(kind, h, w, c, seed=10 * i + j), (1, 50, 75, 100)[(i + 2 * j) % 4], sub,
                    (0, 1, 2, 'row')[(i + j) % 4]))
  cases.append((scene('noise', 64, 96, 3, seed=3), 100, '4:4:4', 0))
  cases.append((scene('checker', 40, 72, 3), 100, '4:2:0', 1))
  cases.append((scene('constant', 136, 136, 1), 75, '4:2:0', 0))
  # more MCUs in a row than a transform tile holds (40 at 4:2:0, 60 at 4:2:2, 80 at 4:4:4, 240 grey)
  cases.append((scene('mixed', 20, 650, 3, seed=5), 75, '4:2:0', 0))
  cases.append((scene('mixed', 9, 970, 3, seed=6), 90, '4:2:2', 'row'))
  cases.append((scene('mixed', 9, 650, 3, seed=7), 50, '4:4:4', 0))
  cases.append((scene('mixed', 9, 1930, 1, seed=8), 75, '4:2:0', 3))
  return cases


def corpus_file(cases) -> bytes:
  out = bytearray(b'JPGE' + struct.pack('<I', len(cases)))
  for pixels, quality, subsampling, restart in cases:
    sampling = 'grey' if pixels.shape[2] == 1 else SUBSAMPLING[subsampling]
    restart = restart_mcus(restart, pixels.shape[1], sampling)
    coefs, tables = coefficients(pixels, quality, sampling)
    want = entropy(coefs, sampling, restart)
    out += table_row(pixels.shape[0], pixels.shape[1], sampling, tables, restart).tobytes()
    out += struct.pack('<II', pixels.size, len(want)) + pixels.tobytes() + want
  return bytes(out)
