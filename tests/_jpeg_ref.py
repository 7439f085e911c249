"""Reference material for the JPEG tests, NumPy only.

  write_jpeg     a baseline JPEG built from CHOSEN quantised coefficients: any of the four samplings,
                 the Annex K Huffman tables or given ones, 8- or 16-bit DQT, DRI; blocks may be
                 replaced by hand-made symbol lists (for malformed streams).  It reports where every
                 symbol and every stuffed FF lies in the raw bytes of its segment.
  decode         the oracle: container walk, bitwise Huffman decode, then `pixels`.
  pixels         expected pixels from coefficients: slow-integer IDCT (13-bit constants, descale 11
                 then 18), fancy upsampling, colour; int64 arithmetic that asserts every intermediate
                 fits int32, and SATURATES the sample to [0, 255].
  scan_status    the serial decode of one entropy segment with the status rules of
                 csrc/jpeg_core.h, for corrupted streams whose fate is not known by construction.
The arithmetic is pinned against Pillow (libjpeg-turbo) in tests/test_jpeg_cpu.py."""
import struct
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
               13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
               52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
STATUS = ['OK', 'TRUNCATED', 'BAD_CODE', 'BAD_RUN', 'BAD_DC', 'TOO_LONG']
SAMPLINGS = {'grey': (1, 1, 1), '444': (3, 1, 1), '422': (3, 2, 1), '420': (3, 2, 2)}   # comps, h0, v0

# ITU-T T.81 Annex K.3: the typical Huffman tables, (counts per length 1..16, values)
_AC_TAIL = ('43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 '
            '79 7a ')
ANNEX_K = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
        '01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 '
        '24 33 62 72 82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a ' + _AC_TAIL +
        '83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 '
        'b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 '
        'f2 f3 f4 f5 f6 f7 f8 f9 fa'))),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
        '00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 '
        '15 62 72 d1 0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a ' + _AC_TAIL +
        '82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 '
        'b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 '
        'f3 f4 f5 f6 f7 f8 f9 fa'))),
}
_AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
# every code word 16 bits long (an incomplete code, which T.81 allows)
LONG_CODES = {(0, 0): ([0] * 15 + [12], list(range(12))), (0, 1): ([0] * 15 + [12], list(range(12))),
              (1, 0): ([0] * 15 + [162], _AC_SYMBOLS), (1, 1): ([0] * 15 + [162], _AC_SYMBOLS)}
# DC tables with a code for the categories 12..15, which baseline does not have
WIDE_DC = dict(ANNEX_K)
WIDE_DC[(0, 0)] = WIDE_DC[(0, 1)] = ([0, 0, 0, 16] + [0] * 12, list(range(16)))
FLAT_QUANT = np.ones(64, np.int64)


def code_book(counts, values) -> Dict[int, Tuple[int, int]]:
  """value -> (code, length), T.81 Annex C."""
  book, code, k = {}, 0, 0
  for l in range(1, 17):
    for _ in range(counts[l - 1]):
      book[values[k]] = (code, l)
      code += 1
      k += 1
    code <<= 1
  return book


def category(v: int) -> int:
  return int(abs(int(v))).bit_length()


def extra_bits(v: int, t: int) -> int:
  return v if v >= 0 else v + (1 << t) - 1


def block_symbols(block, pred) -> List[tuple]:
  """The symbols of one block (64 coefficients in row-major order): ('dc', category, extra) and
  ('ac', run << 4 | size, extra).  A block that ends at coefficient 63 carries no EOB."""
  block = np.asarray(block).reshape(64)
  if not block[1:].any():
    d = int(block[0]) - pred
    return [('dc', category(d), extra_bits(d, category(d))), ('ac', 0x00, 0)]
  z = [int(v) for v in block[ZZ]]
  d = z[0] - pred
  out = [('dc', category(d), extra_bits(d, category(d)))]
  run = 0
  last = max([k for k in range(1, 64) if z[k]], default=0)
  for k in range(1, last + 1):
    if z[k] == 0:
      run += 1
      continue
    while run > 15:
      out.append(('ac', 0xF0, 0))
      run -= 16
    s = category(z[k])
    out.append(('ac', (run << 4) | s, extra_bits(z[k], s)))
    run = 0
  if last < 63:
    out.append(('ac', 0x00, 0))
  return out


class Written(NamedTuple):
  data: bytes
  segments: List[Tuple[int, int]]          # (offset in data, length) of every entropy segment
  symbols: List[np.ndarray]                # per segment (n, 2): raw bit position of each symbol's
                                           # first and last bit
  stuffed: List[np.ndarray]                # per segment: raw byte offsets of the FFs that got a 00
  filled: int = 0                          # `fill`: the count that satisfied the predicate


def _pack(vals, lens):
  """Symbols (value, bit length) -> (stuffed bytes, raw bit span of each symbol, raw offsets of the
  stuffed FFs).  The last byte is padded with 1 bits."""
  vals, lens = np.asarray(vals, np.int64), np.asarray(lens, np.int64)
  ends = np.cumsum(lens)
  starts = ends - lens
  total = int(ends[-1]) if len(ends) else 0
  rep = np.repeat(np.arange(len(vals)), lens)
  within = np.arange(total) - starts[rep]
  bits = ((vals[rep] >> (lens[rep] - 1 - within)) & 1).astype(np.uint8)
  bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
  plain = np.packbits(bits)
  is_ff = plain == 0xFF
  before = np.concatenate([[0], np.cumsum(is_ff)])   # stuffed zeros in front of plain byte i
  where = np.flatnonzero(is_ff)
  raw = np.insert(plain, where + 1, 0)
  to_raw = lambda bit: ((bit >> 3) + before[bit >> 3]) * 8 + (bit & 7)
  spans = np.stack([to_raw(starts), to_raw(ends - 1)], 1) if total else np.zeros((0, 2), np.int64)
  return raw.tobytes(), spans, where + before[where]


def write_jpeg(coefs: Sequence[np.ndarray], height: int, width: int, sampling: str,
               quant: Sequence[np.ndarray] = (FLAT_QUANT, FLAT_QUANT), huffman=None, dqt16: bool = False,
               dri: int = 0, tamper: Optional[Dict[int, List[tuple]]] = None, sof: str = 'C0',
               extra: bytes = b'', fill=None) -> Written:
  """coefs: per component (block rows, block columns, 64) quantised coefficients in row-major order,
  covering whole MCUs.  quant: (luma, chroma) tables in row-major order.  huffman: {(class, id): (counts,
  values)}, ids 0 = luma, 1 = chroma; default Annex K.  tamper: scan-order block index -> the symbols
  written instead of that block's: ('dc', category, extra), ('ac', run/size, extra) or ('raw', value,
  bits); the DC predictor runs on as if the block had been written.  extra: bytes in front of SOF
  (more marker segments).  fill = (block index, predicate[, candidate counts]): that block, a luma block without AC
  coefficients in a file without DRI, gets the smallest k in 0..63 of coefficients -1 at zig-zag
  indices 1..k (3 bits each, never an FF) for which predicate(raw bytes, symbol spans, stuffed
  offsets) holds; `filled` reports k, and the caller's expected pixels must put them in."""
  huffman = huffman or ANNEX_K
  nc, h0, v0 = SAMPLINGS[sampling]
  mx, my = -(-width // (8 * h0)), -(-height // (8 * v0))
  shapes = [(my * v0, mx * h0)] + [(my, mx)] * (nc - 1)
  coefs = [np.asarray(c) for c in coefs]
  assert [c.shape for c in coefs] == [s + (64,) for s in shapes], [c.shape for c in coefs]
  out = bytearray(b'\xff\xd8' + extra)
  for tq in range(2 if nc == 3 else 1):
    q = np.asarray(quant[tq]).reshape(64)[ZZ]
    body = bytes([(16 if dqt16 else 0) | tq]) + (b''.join(struct.pack('>H', int(v)) for v in q) if dqt16
                                                  else bytes(int(v) for v in q))
    out += b'\xff\xdb' + struct.pack('>H', 2 + len(body)) + body
  comp_bytes = b''.join(bytes([i + 1, ((h0 << 4) | v0) if i == 0 else 0x11, min(i, 1)]) for i in range(nc))
  out += bytes([0xFF, int(sof, 16)]) + struct.pack('>HBHHB', 8 + 3 * nc, 8, height, width, nc) + comp_bytes
  for (tc, th), (counts, values) in sorted(huffman.items()):
    if th == 1 and nc == 1:
      continue
    body = bytes([(tc << 4) | th]) + bytes(counts) + bytes(values)
    out += b'\xff\xc4' + struct.pack('>H', 2 + len(body)) + body
  if dri:
    out += b'\xff\xdd' + struct.pack('>HH', 4, dri)
  out += b'\xff\xda' + struct.pack('>HB', 6 + 2 * nc, nc) + b''.join(
      bytes([i + 1, 0x11 * min(i, 1)]) for i in range(nc)) + b'\x00\x3f\x00'
  books = {key: code_book(*huffman[key]) for key in huffman}
  tamper = tamper or {}
  segments, symbols, stuffed = [], [], []
  vals, lens, pred, block_index = [], [], [0] * nc, 0

  fill_at, filled = [None], [0]

  def close():
    raw, spans, ff = _pack(vals, lens)
    if fill is not None:
      assert not dri and fill_at[0] is not None and huffman is ANNEX_K
      for k in (fill[2] if len(fill) > 2 else range(64)):
        raw, spans, ff = _pack(np.insert(vals, fill_at[0], [0] * k), np.insert(lens, fill_at[0], [3] * k))
        if fill[1](raw, spans, ff):
          filled[0] = k
          break
      else:
        raise AssertionError('fill: no count of filler coefficients satisfies the predicate')
    segments.append((len(out), len(raw)))
    symbols.append(spans)
    stuffed.append(ff)
    out.extend(raw)
    vals.clear()
    lens.clear()

  for m in range(mx * my):
    if dri and m and m % dri == 0:
      close()
      out += bytes([0xFF, 0xD0 + (m // dri - 1) % 8])
      pred = [0] * nc
    r, c = divmod(m, mx)
    for ci in range(nc):
      ch, cv = (h0, v0) if ci == 0 else (1, 1)
      for by in range(cv):
        for bx in range(ch):
          block = coefs[ci][r * cv + by, c * ch + bx]
          syms = tamper.get(block_index, None) or block_symbols(block, pred[ci])
          pred[ci] = int(block[0])
          for kind, a, b in syms:
            if kind == 'raw':
              vals.append(a)
              lens.append(b)
              continue
            code, l = books[(0 if kind == 'dc' else 1, min(ci, 1))][a]
            size = a if kind == 'dc' else a & 15
            vals.append((code << size) | b)
            lens.append(l + size)
          if fill is not None and block_index == fill[0]:
            assert ci == 0 and not np.any(block[1:])
            fill_at[0] = len(vals) - 1   # in front of the EOB
          block_index += 1
  close()
  out += b'\xff\xd9'
  return Written(bytes(out), segments, symbols, stuffed, filled[0])


def random_coefs(rng, height, width, sampling, density=1.0, dc=200, ac=30):
  """In-range random coefficients for `write_jpeg` (with FLAT_QUANT the samples mostly stay in range)."""
  nc, h0, v0 = SAMPLINGS[sampling]
  mx, my = -(-width // (8 * h0)), -(-height // (8 * v0))
  out = []
  for ci in range(nc):
    shape = (my * (v0 if ci == 0 else 1), mx * (h0 if ci == 0 else 1), 64)
    c = rng.integers(-ac, ac + 1, shape)
    c *= rng.random(shape) < density
    c[..., 0] = rng.integers(-dc, dc + 1, shape[:2])
    out.append(c)
  return out


def flat_420(height: int, width: int, dc: int = 0) -> bytes:
  """A flat 4:2:0 file: every luma block has DC `dc`, so every block but the first is "DC difference
  0, EOB" -- 32 bits per MCU, a periodic stream."""
  my, mx = -(-height // 16), -(-width // 16)
  luma = np.zeros((2 * my, 2 * mx, 64), np.int64)
  luma[..., 0] = dc
  return write_jpeg([luma, np.zeros((my, mx, 64), np.int64), np.zeros((my, mx, 64), np.int64)], height, width,
                    '420').data


# ------------------------------------------------------------------------------------ the oracle
def parse(d: bytes):
  """-> (height, width, components [(id, h, v, tq)]), quant {id: row-major table}, huffman {(class <<
  4) | id: {(length, code): value}}, dri, scan [(id, td, ta)], the bytes behind SOS."""
  p, q, h, dri, frame = 2, {}, {}, 0, None
  while True:
    assert d[p] == 0xFF, p
    m = d[p + 1]
    p += 2
    if m == 0xD8 or 0xD0 <= m <= 0xD7:
      continue
    n = (d[p] << 8) | d[p + 1]
    s = d[p + 2:p + n]
    if m == 0xDB:
      i = 0
      while i < len(s):
        pq, tq = s[i] >> 4, s[i] & 15
        i += 1
        t = np.zeros(64, np.int64)
        for k in range(64):
          if pq:
            t[ZZ[k]] = (s[i] << 8) | s[i + 1]
            i += 2
          else:
            t[ZZ[k]] = s[i]
            i += 1
        q[tq] = t
    elif m == 0xC4:
      i = 0
      while i < len(s):
        tc = s[i]
        counts = list(s[i + 1:i + 17])
        values = list(s[i + 17:i + 17 + sum(counts)])
        i += 17 + sum(counts)
        h[tc] = {(l, code): v for v, (code, l) in code_book(counts, values).items()}
    elif m in (0xC0, 0xC1):
      nc = s[5]
      frame = ((s[1] << 8) | s[2], (s[3] << 8) | s[4],
               [(s[6 + 3 * i], s[7 + 3 * i] >> 4, s[7 + 3 * i] & 15, s[8 + 3 * i]) for i in range(nc)])
    elif m == 0xDD:
      dri = (s[0] << 8) | s[1]
    elif m == 0xDA:
      ns = s[0]
      return frame, q, h, dri, [(s[1 + 2 * i], s[2 + 2 * i] >> 4, s[2 + 2 * i] & 15) for i in range(ns)], d[p + n:]
    p += n


class _Bits:
  def __init__(self, d):
    self.d, self.p, self.acc, self.n = d, 0, 0, 0

  def bit(self):
    if self.n == 0:
      b = self.d[self.p]
      self.p += 1
      if b == 0xFF:
        assert self.d[self.p] == 0
        self.p += 1
      self.acc, self.n = b, 8
    self.n -= 1
    return (self.acc >> self.n) & 1

  def get(self, k):
    v = 0
    for _ in range(k):
      v = (v << 1) | self.bit()
    return v

  def restart(self):
    self.n = 0
    assert self.d[self.p] == 0xFF and 0xD0 <= self.d[self.p + 1] <= 0xD7, self.d[self.p:self.p + 2]
    self.p += 2


def _huff(b, tab):
  code = 0
  for l in range(1, 17):
    code = (code << 1) | b.bit()
    if (l, code) in tab:
      return tab[(l, code)]
  raise ValueError('no code word')


def _ext(v, t):
  return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def _geometry(frame):
  height, width, comps = frame
  if len(comps) == 1:
    comps = [(comps[0][0], 1, 1, comps[0][3])]
  hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
  return height, width, comps, hm, vm, -(-width // (8 * hm)), -(-height // (8 * vm))


def decode_coefficients(d: bytes):
  """The bitwise Huffman decode of a well-formed file -> (per component (rows, columns, 64) int64 in
  row-major order, per component quantisation table, frame)."""
  frame, q, h, dri, sc, ent = parse(d)
  height, width, comps, hm, vm, mw, mh = _geometry(frame)
  coef = [np.zeros((mh * c[2], mw * c[1], 64), np.int64) for c in comps]
  b, pred, sel = _Bits(ent), [0] * len(comps), {cid: (td, ta) for cid, td, ta in sc}
  for m in range(mw * mh):
    if dri and m and m % dri == 0:
      b.restart()
      pred = [0] * len(comps)
    my, mx = divmod(m, mw)
    for ci, (cid, ch, cv, tq) in enumerate(comps):
      td, ta = sel[cid]
      for by in range(cv):
        for bx in range(ch):
          blk = coef[ci][my * cv + by, mx * ch + bx]
          t = _huff(b, h[td])
          pred[ci] += _ext(b.get(t), t)
          blk[0] = pred[ci]
          k = 1
          while k < 64:
            rs = _huff(b, h[0x10 | ta])
            r, s = rs >> 4, rs & 15
            if s == 0:
              if r == 15:
                k += 16
                continue
              break
            k += r
            blk[ZZ[k]] = _ext(b.get(s), s)
            k += 1
  return coef, [q[c[3]] for c in comps], frame


def _fits(*xs):
  for x in xs:
    assert x.size == 0 or (x.min() >= -2 ** 31 and x.max() < 2 ** 31), 'an intermediate leaves int32'
  return xs[0] if len(xs) == 1 else xs


def idct1(x, sh):
  """One 1-D pass over the last axis (8 values), int64."""
  in0, in1, in2, in3, in4, in5, in6, in7 = [x[..., i] for i in range(8)]
  z1 = _fits((in2 + in6) * 4433)
  tmp2, tmp3 = _fits(z1 - in6 * 15137, z1 + in2 * 6270)
  tmp0, tmp1 = _fits((in0 + in4) << 13, (in0 - in4) << 13)
  t10, t13, t11, t12 = _fits(tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2)
  tmp0, tmp1, tmp2, tmp3 = in7, in5, in3, in1
  z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
  z5 = _fits((z3 + z4) * 9633)
  tmp0, tmp1, tmp2, tmp3 = _fits(tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299)
  z1, z2 = _fits(-z1 * 7373, -z2 * 20995)
  z3, z4 = _fits(-z3 * 16069 + z5, -z4 * 3196 + z5)
  tmp0, tmp1, tmp2, tmp3 = _fits(tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4)
  o = [t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3]
  return np.stack([_fits(v + (1 << (sh - 1))) >> sh for v in o], -1)


def idct(blocks):
  """(..., 8, 8) dequantised [row, column] -> (samples before + 128 and the clamp, the largest
  magnitudes after the first pass and of the samples)."""
  ws = np.swapaxes(idct1(np.swapaxes(blocks, -1, -2), 11), -1, -2)
  out = idct1(ws, 18)
  return out, (int(np.abs(ws).max()) if ws.size else 0, int(np.abs(out).max()) if out.size else 0)


def pixels(coefs, quants, height, width, sampling_hv, channels=0, stats=None) -> np.ndarray:
  """Expected pixels (H, W, C) uint8 from per-component coefficients (rows, columns, 64) and their
  quantisation tables.  sampling_hv: [(h, v)] per component.  channels as decode_jpeg_batch."""
  hm, vm = max(h for h, _ in sampling_hv), max(v for _, v in sampling_hv)
  full = []
  for c, q, (ch, cv) in zip(coefs, quants, sampling_hv):
    deq = _fits(np.asarray(c, np.int64) * np.asarray(q, np.int64)).reshape(c.shape[0], c.shape[1], 8, 8)
    o, st = idct(deq)
    if stats is not None:
      stats.append(st)
    o = np.clip(o + 128, 0, 255)
    plane = o.transpose(0, 2, 1, 3).reshape(o.shape[0] * 8, o.shape[1] * 8)
    dw, dh = -(-width * ch // hm), -(-height * cv // vm)
    p = plane[:dh, :dw]
    if ch == hm and cv == vm:
      full.append(p[:height, :width])
      continue
    assert hm == 2 * ch and vm in (cv, 2 * cv)
    if dw > 2:
      if vm == cv:
        o = np.zeros((dh, 2 * dw), np.int64)
        l, r = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
        o[:, 0::2], o[:, 1::2] = (3 * p + l + 1) >> 2, (3 * p + r + 2) >> 2
        o[:, 0], o[:, -1] = p[:, 0], p[:, -1]
      else:
        up, dn = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
        o = np.zeros((2 * dh, 2 * dw), np.int64)
        for v, nb in ((0, up), (1, dn)):
          cs = 3 * p + nb
          l, r = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
          e, od = (3 * cs + l + 8) >> 4, (3 * cs + r + 7) >> 4
          e[:, 0], od[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
          o[v::2, 0::2], o[v::2, 1::2] = e, od
    else:   # a component no wider than 2 samples is replicated, not filtered
      o = np.repeat(p, 2, 1)
      if vm != cv:
        o = np.repeat(o, 2, 0)
    full.append(o[:height, :width])
  if len(full) == 1 or channels == 1:
    grey = full[0].astype(np.uint8)[..., None]
    return np.repeat(grey, 3, -1) if (channels == 3 and len(full) == 1) else grey
  y, cb, cr = full[0], full[1] - 128, full[2] - 128
  r, b = y + ((91881 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)
  g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
  return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(d: bytes, channels=0, stats=None) -> np.ndarray:
  """The oracle on a file: (H, W, C) uint8."""
  coef, quants, frame = decode_coefficients(d)
  height, width, comps = _geometry(frame)[:3]
  return pixels(coef, quants, height, width, [(c[1], c[2]) for c in comps], channels, stats)


def expected(coefs, height, width, sampling, quant=(FLAT_QUANT, FLAT_QUANT), channels=0, stats=None):
  """Expected pixels of `write_jpeg(coefs, height, width, sampling, quant)` without decoding it."""
  nc, h0, v0 = SAMPLINGS[sampling]
  return pixels(coefs, [quant[min(i, 1)] for i in range(nc)], height, width,
                [(h0, v0)] + [(1, 1)] * (nc - 1), channels, stats)


# ------------------------------------------------------------------- status of a damaged segment
def scan_status(segment: bytes, tables, slots: Sequence[Tuple[int, int]], total_blocks: int) -> str:
  """The serial decode of one entropy segment by the rules of csrc/jpeg_core.h -> the status name.
  tables: parse()'s Huffman dicts; slots: (DC table, AC table) ids of every block of an MCU."""
  nbits = len(segment) * 8
  data = bytes(segment) + bytes(16)

  def step(byte):   # the raw index of the data byte behind `byte`
    return byte + (2 if data[byte] == 0xFF and data[byte + 1] == 0 else 1)

  def peek(pos, n):
    byte, acc = pos >> 3, 0
    for _ in range(6):
      acc = (acc << 8) | data[byte]
      byte = step(byte)
    return (acc >> (48 - (pos & 7) - n)) & ((1 << n) - 1)

  def advance(pos, n):
    byte, bit = pos >> 3, (pos & 7) + n
    while bit >= 8:
      byte, bit = step(byte), bit - 8
    return byte * 8 + bit

  def code(pos, tab):
    for l in range(1, 17):
      if (l, peek(pos, l)) in tab:
        return tab[(l, peek(pos, l))], l, None
    return 0, 16, 'BAD_CODE'

  pos, k, blocks, slot = 0, 0, 0, 0
  while pos < nbits:
    td, ta = slots[slot]
    if k == 0:
      t, l, err = code(pos, tables[td])
      if t > 11:
        err, t = err or 'BAD_DC', 11
      pos, k = advance(pos, l + t), 1
    else:
      rs, l, err = code(pos, tables[0x10 | ta])
      r, s = rs >> 4, rs & 15
      if s == 0:
        k = k + 16 if r == 15 else 64
        if k > 64:
          err, k = err or 'BAD_RUN', 64
      else:
        k += r
        if k > 63:
          err, k = err or 'BAD_RUN', 63
        k += 1
      pos = advance(pos, l + s)
    if not err and pos > nbits:
      err = 'TRUNCATED'
    if err:
      return err
    if k >= 64:
      k, slot, blocks = 0, (slot + 1) % len(slots), blocks + 1
      if blocks == total_blocks:
        nxt = advance(pos, 8 - (pos & 7)) if pos & 7 else pos
        return 'TOO_LONG' if nxt < nbits else 'OK'
  return 'TRUNCATED'


# ------------------------------------------------------------------------ the corpus of the tests
class Case(NamedTuple):
  name: str
  data: bytes
  status: str           # of the first segment that fails; 'OK' for a good file


def _flat_block(dc):
  b = np.zeros(64, np.int64)
  b[0] = dc
  return b


def bad_cases() -> List[Case]:
  """Malformed 4:2:0 files of 32 x 16 pixels (2 MCUs = 12 blocks), each with the status the decoder
  must give."""
  rng = np.random.default_rng(11)
  coefs = random_coefs(rng, 16, 32, '420')
  good = write_jpeg(coefs, 16, 32, '420')
  at, n = good.segments[0]
  cases = [Case('truncated', good.data[:at + n // 2] + b'\xff\xd9', 'TRUNCATED')]
  cases.append(Case('undefined_code', write_jpeg(coefs, 16, 32, '420', tamper={
      5: [('dc', 0, 0), ('raw', 0xFFFF, 16)]}).data, 'BAD_CODE'))
  cases.append(Case('run_past_63', write_jpeg(coefs, 16, 32, '420', tamper={
      7: [('dc', 1, 1)] + [('ac', 0x01, 1)] * 60 + [('ac', 0x51, 0)]}).data, 'BAD_RUN'))
  cases.append(Case('zrl_past_63', write_jpeg(coefs, 16, 32, '420', tamper={
      2: [('dc', 1, 1)] + [('ac', 0xF0, 0)] * 4}).data, 'BAD_RUN'))
  cases.append(Case('dc_category_12', write_jpeg(coefs, 16, 32, '420', huffman=WIDE_DC, tamper={
      3: [('dc', 12, 0xABC), ('ac', 0x00, 0)]}).data, 'BAD_DC'))
  # one MCU too many for the geometry: the frame header says 16 x 16
  more = bytearray(good.data)
  sof = more.index(b'\xff\xc0')
  more[sof + 5:sof + 9] = struct.pack('>HH', 16, 16)
  cases.append(Case('block_too_many', bytes(more), 'TOO_LONG'))
  # a damaged byte in mid-stream: whatever the serial decode by the same rules makes of it
  frame, _, tables, _, _, _ = parse(good.data)
  slots = [(0, 0)] * 4 + [(1, 1)] * 2
  for k in range(n // 3, n):
    hit = bytearray(good.data)
    hit[at + k] ^= 0x5A
    if hit[at + k] == 0xFF or hit[at + k - 1] == 0xFF:
      continue
    status = scan_status(bytes(hit[at:at + n]), tables, slots, 12)
    if status != 'OK':
      cases.append(Case('damaged_byte', bytes(hit), status))
      break
  assert len(cases) == 7
  return cases


def good_cases() -> List[Tuple[Case, np.ndarray]]:
  """Small well-formed files with their expected pixels: the four samplings, restart intervals, 16-bit
  codes and tables, a block that fills coefficient 63, ZRL chains, DC category 11, stuffed FFs."""
  rng = np.random.default_rng(12)
  out = []
  for name, (h, w, sampling, kw) in {
      'grey_9x17': (9, 17, 'grey', {}), '444_17x33': (17, 33, '444', {}), '422_5x4': (5, 4, '422', {}),
      '420_33x6': (33, 6, '420', {}), '420_dri1': (24, 40, '420', dict(dri=1)),
      '422_dri3': (16, 80, '422', dict(dri=3)), '444_long_codes': (16, 24, '444', dict(huffman=LONG_CODES)),
      '420_dqt16': (16, 16, '420', dict(dqt16=True)), '444_64x48': (64, 48, '444', {}),
  }.items():
    coefs = random_coefs(rng, h, w, sampling)
    quant = (FLAT_QUANT, FLAT_QUANT)
    if kw.get('dqt16'):
      quant = (FLAT_QUANT * 300, FLAT_QUANT * 257)
      coefs = [np.clip(c, -1, 1) for c in coefs]
    out.append((Case(name, write_jpeg(coefs, h, w, sampling, quant=quant, **kw).data, 'OK'),
                expected(coefs, h, w, sampling, quant)))
  coefs = extreme_coefs(rng, 16, 32, '420')
  out.append((Case('420_extremes', write_jpeg(coefs, 16, 32, '420').data, 'OK'), expected(coefs, 16, 32, '420')))
  written, coefs, h, w = chunk_tail_file(128, 32768)
  out.append((Case('grey_chunk_tail', written.data, 'OK'), expected(coefs, h, w, 'grey')))
  return out


def chunk_tail_file(chunk: int, window: int):
  """A grey file whose last symbol (the EOB of the last block) starts in one chunk and ends in the first
  byte of the next chunk of the same window, padding behind it: the entropy length is 1 modulo `chunk`
  and not 1 modulo `window`.  A lane that owns only that byte enters behind the last block with nothing
  but padding in front of it.  -> (Written, coefficients, height, width); the writer's symbol spans
  confirm the shape."""
  def shaped(raw, spans, ff):
    n = len(raw)
    return (n > chunk and n % chunk == 1 and n % window != 1 and
            spans[-1, 0] // (8 * chunk) != spans[-1, 1] // (8 * chunk) and spans[-1, 1] // 8 == n - 1)

  for seed in range(2000):
    rng = np.random.default_rng(1000 + seed)
    blocks = 5 + seed % 5      # the dense blocks take about 65 bytes each: some count comes near
    coefs = random_coefs(rng, 8, 8 * blocks, 'grey')
    coefs[0][0, -1, 1:] = 0
    try:
      written = write_jpeg(coefs, 8, 8 * blocks, 'grey', fill=(blocks - 1, shaped))
    except AssertionError:
      continue
    coefs[0][0, -1, ZZ[1:1 + written.filled]] = -1
    return written, coefs, 8, 8 * blocks
  raise AssertionError('no file with the last symbol across a chunk boundary')


def extreme_coefs(rng, height, width, sampling):
  """Coding extremes: DC differences of category 11, ZRL chains (one coefficient at index 63 or far
  out), blocks that fill coefficient 63 (no EOB), empty blocks."""
  coefs = random_coefs(rng, height, width, sampling, density=0.0, dc=0)
  for c in coefs:
    flat = c.reshape(-1, 64)
    flat[0::2, 0] = 1023
    flat[1::2, 0] = -1024          # differences of +-2047: category 11
    flat[0::3, 63] = 5             # three ZRLs, then the last coefficient: no EOB
    flat[1::3, ZZ[40]] = -3        # two ZRLs
    flat[2::5, 1:] = rng.integers(1, 4, (len(flat[2::5]), 63))   # dense to the end
  return coefs


def corpus_file(good: Sequence[Tuple[Case, np.ndarray]], bad: Sequence[Case]) -> bytes:
  """The corpus of tools/jpeg_host_check.cpp (its header has the format): the files go through
  `parse_jpeg`, and the program gets the tables `decode_jpeg_batch` would upload."""
  from se3ds_amd.utils import jpeg
  out = bytearray(b'JPGC' + struct.pack('<I', len(good) + len(bad)))
  for case, px in list(good) + [(c, None) for c in bad]:
    s = jpeg.parse_jpeg(case.data)
    image = np.zeros(200, np.int64)
    image[:5] = (s.width, s.height, s.components, s.h0, s.v0)
    image[6] = s.components
    image[9:14] = (0, len(s.segments), s.mcus_x, s.mcus_y, s.tables)
    raw = image.view(np.uint8)
    raw[128:128 + 128 * s.components] = s.quant.view(np.uint8).reshape(-1)
    raw[512:] = s.huffman.reshape(-1)
    first, last = s.segments[0][0], s.segments[-1][0] + s.segments[-1][1]
    mcus, step = s.mcus_x * s.mcus_y, s.restart_interval or s.mcus_x * s.mcus_y
    rows = [(0, at - first, n, k * step, min(step, mcus - k * step)) for k, (at, n) in enumerate(s.segments)]
    pixels_bytes = b'' if px is None else np.ascontiguousarray(px, np.uint8).tobytes()
    out += struct.pack('<iIII', STATUS.index(case.status), len(rows), last - first, len(pixels_bytes))
    out += raw.tobytes() + np.array(rows, np.int64).tobytes() + case.data[first:last] + pixels_bytes
  return bytes(out)
