"""Test-side deflate WRITER (RFC 1951) with zlib framing (RFC 1950), for streams no compressor
emits: stored, fixed-Huffman and dynamic-Huffman blocks from explicit symbols, explicit code lengths
and an explicit sequence of code-length symbols; and the corpus of good and malformed streams that
tests/test_inflate_cpu.py and tests/test_inflate_gpu.py share.  The tables below are the RFC's,
written out, not the arithmetic of csrc/inflate_core.h.  The oracle for what a stream inflates to
is CPython's zlib.decompress, never the code under test."""
import struct
import zlib
from typing import NamedTuple, Optional

import numpy as np

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
               131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
             2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12,
              13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# status names of csrc/inflate_core.h (enum class Status) in order
STATUS = ['OK', 'TRUNCATED', 'BAD_HEADER', 'BAD_BLOCK_TYPE', 'BAD_STORED_LENGTH', 'BAD_COUNTS',
          'OVER_SUBSCRIBED', 'INCOMPLETE', 'BAD_REPEAT', 'NO_END_OF_BLOCK', 'BAD_CODE', 'BAD_DISTANCE',
          'TOO_LONG', 'TOO_SHORT', 'BAD_ADLER', 'BAD_FILTER']
GRANULE = 16384   # csrc/inflate_core.h kGranule, the flush unit


class BitWriter:
  """Bits are packed from the least significant bit of each byte up (RFC 1951 3.1.1)."""

  def __init__(self):
    self.out = bytearray()
    self.acc = 0
    self.n = 0

  def bits(self, value: int, count: int):
    """A data element: least significant bit first."""
    assert 0 <= value < (1 << count) or count == 0
    self.acc |= value << self.n
    self.n += count
    while self.n >= 8:
      self.out.append(self.acc & 0xff)
      self.acc >>= 8
      self.n -= 8

  def code(self, code: int, length: int):
    """A Huffman code: most significant bit first."""
    for i in range(length - 1, -1, -1):
      self.bits((code >> i) & 1, 1)

  def align(self):
    if self.n:
      self.bits(0, 8 - self.n)

  def raw(self, data: bytes):
    assert self.n == 0
    self.out += data

  def done(self) -> bytes:
    self.align()
    return bytes(self.out)


def canonical(lengths):
  """{symbol: (code, length)} by the algorithm of RFC 1951 3.2.2 (no completeness check)."""
  count = [0] * 17
  for l in lengths:
    count[l] += 1
  count[0] = 0
  nxt, code = [0] * 17, 0
  for l in range(1, 17):
    code = (code + count[l - 1]) << 1
    nxt[l] = code
  out = {}
  for s, l in enumerate(lengths):
    if l:
      out[s] = (nxt[l], l)
      nxt[l] += 1
  return out


def complete_lengths(symbols, size):
  """Code lengths over an alphabet of `size` that give the (>= 2) `symbols` a complete code."""
  symbols = sorted(set(symbols))
  n = len(symbols)
  assert n >= 2
  top = (n - 1).bit_length()
  short = (1 << top) - n          # this many symbols can be one bit shorter
  lens = [0] * size
  for i, s in enumerate(symbols):
    lens[s] = top - 1 if i < short else top
  return lens


def _length_symbol(length):
  i = max(k for k in range(29) if LENGTH_BASE[k] <= length)
  return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]


def _dist_symbol(dist):
  i = max(k for k in range(30) if DIST_BASE[k] <= dist)
  return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def emit_items(w: BitWriter, items, lit_lens, dist_lens, end=True):
  """items: a literal byte value, a (length, distance) pair, ('lit', symbol) for a raw
  literal/length symbol (its extra bits are the writer's business) or ('dist', length, symbol) for a
  raw distance symbol after a length.  Then the end-of-block symbol."""
  lit, dist = canonical(lit_lens), canonical(dist_lens)
  for it in items:
    if isinstance(it, int):
      w.code(*lit[it])
    elif it[0] == 'lit':
      w.code(*lit[it[1]])
    else:
      raw = it[0] == 'dist'
      length = it[1] if raw else it[0]
      sym, eb, ev = _length_symbol(length)
      w.code(*lit[sym])
      w.bits(ev, eb)
      if raw:
        w.code(*dist[it[2]])
      else:
        dsym, eb, ev = _dist_symbol(it[1])
        w.code(*dist[dsym])
        w.bits(ev, eb)
  if end:
    w.code(*lit[256])


def stored_block(w: BitWriter, data: bytes, final: bool, nlen: Optional[int] = None):
  assert len(data) <= 0xffff
  w.bits(int(final), 1)
  w.bits(0, 2)
  w.align()
  w.raw(struct.pack('<HH', len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
  w.raw(data)


def fixed_block(w: BitWriter, items, final: bool, end=True):
  w.bits(int(final), 1)
  w.bits(1, 2)
  emit_items(w, items, FIXED_LIT, FIXED_DIST, end)


def dynamic_block(w: BitWriter, lit_lens, dist_lens, items, final: bool, clen_syms=None,
                  clen_lens=None, hclen=None, end=True):
  """lit_lens (257..288 entries) and dist_lens (1..32 entries) are sent as they are.  clen_syms: the
  code-length symbols that transmit lit_lens + dist_lens, each a length 0..15, (16, repeat 3..6),
  (17, repeat 3..10) or (18, repeat 11..138); None: one plain length per entry.  clen_lens: the 19
  lengths of the code-length code; None: a complete code over the symbols used.  hclen: how many of
  them are sent (4..19); None: up to the last non-zero one in CLEN_ORDER."""
  if clen_syms is None:
    clen_syms = list(lit_lens) + list(dist_lens)
  used = [s if isinstance(s, int) else s[0] for s in clen_syms]
  if clen_lens is None:
    pool = set(used)
    for extra in (0, 8, 7):          # a code needs two symbols to be complete
      if len(pool) < 2:
        pool.add(extra)
    clen_lens = complete_lengths(pool, 19)
  if hclen is None:
    hclen = max(4, max(i + 1 for i, s in enumerate(CLEN_ORDER) if clen_lens[s]))
  assert all(clen_lens[s] == 0 for s in CLEN_ORDER[hclen:])
  w.bits(int(final), 1)
  w.bits(2, 2)
  w.bits(len(lit_lens) - 257, 5)
  w.bits(len(dist_lens) - 1, 5)
  w.bits(hclen - 4, 4)
  for s in CLEN_ORDER[:hclen]:
    w.bits(clen_lens[s], 3)
  cl = canonical(clen_lens)
  for s in clen_syms:
    if isinstance(s, int):
      w.code(*cl[s])
    else:
      sym, rep = s
      w.code(*cl[sym])
      w.bits(rep - {16: 3, 17: 3, 18: 11}[sym], {16: 2, 17: 3, 18: 7}[sym])
  if items is not None:
    emit_items(w, items, lit_lens, dist_lens, end)


def expand_items(items) -> bytes:
  """What a list of literals and (length, distance) pairs inflates to."""
  out = bytearray()
  for it in items:
    if isinstance(it, int):
      out.append(it)
    else:
      length, dist = it
      assert 1 <= dist <= len(out)
      for _ in range(length):
        out.append(out[-dist])
  return bytes(out)


def zlib_frame(raw: bytes, data: bytes = b'', header: bytes = b'\x78\x9c', adler: Optional[int] = None):
  return header + raw + struct.pack('>I', zlib.adler32(data) if adler is None else adler)


def compress(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
  c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
  return c.compress(data) + c.flush()


# ------------------------------------------------------------------------------------ the corpus
class Case(NamedTuple):
  name: str
  stream: bytes            # zlib framing
  status: str              # a name of STATUS
  expected_len: int        # the "IHDR geometry": inflated bytes the caller expects
  pitch: int               # scan-line pitch handed to the decoder (>= 2, divides expected_len)
  data: Optional[bytes]    # status OK: what the stream inflates to
  zlib_raises: bool        # whether zlib.decompress rejects the stream itself
  detail: int = 0          # BAD_FILTER: (filter byte << 8) | (row << 16)

  @property
  def word(self) -> int:
    return STATUS.index(self.status) | self.detail


def _good(name, stream, data):
  """The whole output as one scan line: byte 0 is its filter type and must be <= 4."""
  assert len(data) == 0 or data[0] <= 4, name
  return Case(name, stream, 'OK', len(data), max(2, len(data)), data, False)


def _bad(name, stream, status, expected_len=100, pitch=None, zlib_raises=True, detail=0):
  return Case(name, stream, status, expected_len, pitch or max(2, expected_len), None, zlib_raises, detail)


def _line(rng, n, alphabet=None):
  """n bytes that start with filter type 0."""
  a = (rng.integers(0, 256, n, dtype=np.uint8) if alphabet is None
       else rng.choice(np.frombuffer(alphabet, np.uint8), n))
  if n:
    a[0] = 0
  return a.tobytes()


def _periodic(rng, n, period):
  unit = rng.integers(0, 256, period, dtype=np.uint8)
  unit[0] = 0
  return np.resize(unit, n).tobytes()


def good_cases(ring: int):
  """Every stream the decoder must inflate exactly.  ring: se3ds_png_inflate_ring_bytes()."""
  rng = np.random.default_rng(2024)
  text = _line(rng, 20000, b'etaoin sh')
  cases = []
  add = lambda name, stream, data: cases.append(_good(name, stream, data))

  # ---- stored
  d = _line(rng, 70000)
  add('stored_70000_level0', compress(d, 0), d)
  add('stored_empty_level0', compress(b'', 0), b'')
  w = BitWriter()
  fixed_block(w, [0, 1, 2], False)
  stored_block(w, b'', False)
  stored_block(w, b'tail', True)
  add('stored_zero_length_mid_stream', zlib_frame(w.done(), b'\0\1\2tail'), b'\0\1\2tail')
  # ---- fixed
  d = _line(rng, 3000, b'acgt')
  add('fixed_z_fixed_3000', compress(d, 6, zlib.Z_FIXED), d)
  add('fixed_empty_8_bytes', zlib.compress(b''), b'')
  # ---- dynamic
  for level in (1, 6, 9):
    add(f'dynamic_text_level{level}', compress(text, level), text)
  add('dynamic_huffman_only', compress(text, 6, zlib.Z_HUFFMAN_ONLY), text)
  d = b'\0' * 1000 + b'\7' * 5000
  add('dynamic_rle_runs', compress(d, 6, zlib.Z_RLE), d)
  # ---- overlapping and wave-width matches
  for p in (1, 2, 3, 4, 7, 63, 64, 65, 257, 258, 259):
    d = _periodic(rng, 4000, p)
    add(f'period_{p}', compress(d, 9), d)
  # ---- far matches
  d = _line(rng, 32506)
  d += d[:300]
  add('far_32506', compress(d, 9), d)
  items = list(_line(rng, 32768)) + [(258, 32768)]
  w = BitWriter()
  fixed_block(w, items, True)
  add('far_32768_hand_built', zlib_frame(w.done(), expand_items(items)), expand_items(items))
  # ---- hand-built dynamic headers
  cases += _dynamic_header_cases()
  # ---- block boundaries off the byte grid
  c = zlib.compressobj(6)
  parts = [_line(rng, 40, b'ab'), _line(rng, 3000, b'etaoin sh')[1:], _line(rng, 5000, b'xyz01')[1:]]
  s = (c.compress(parts[0]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(parts[1]) +
       c.flush(zlib.Z_FULL_FLUSH) + c.compress(parts[2]) + c.flush())
  add('sync_and_full_flush', s, b''.join(parts))
  # ---- the ring
  for n in (ring - 1, ring, ring + 1, 2 * ring + 5):
    d = _periodic(rng, n, 300)
    add(f'ring_{n}_bytes', compress(d, 6), d)
  for name, at in (('ring_wrap', ring - 100), ('granule_boundary', GRANULE - 100),
                   ('second_ring_wrap', 2 * ring - 100)):
    w = BitWriter()
    d = _line(rng, at)
    for i in range(0, at, 0xffff):
      stored_block(w, d[i:i + 0xffff], False)
    tail = [(258, 1000), 9, (258, 258), (258, 1)]
    fixed_block(w, tail, True)
    d = d + expand_items(list(d[-1000:]) + tail)[1000:]
    add(f'match_258_across_{name}', zlib_frame(w.done(), d), d)
  return cases


def _dynamic_header_cases():
  out = []

  def case(name, lit_lens, dist_lens, items, **kw):
    w = BitWriter()
    dynamic_block(w, lit_lens, dist_lens, items, True, **kw)
    data = expand_items(items)
    out.append(_good(name, zlib_frame(w.done(), data), data))

  # Eight literal/length codes of length 3 (literals 0..3, end of block, lengths 3, 10 and 11-12) and
  # eight distance codes of length 3: 266 + 8 lengths.  Entry 264 is a plain 3; a code 16 repeats it
  # over entry 265 and the first five distance lengths -- across the HLIT boundary.
  lit = [0] * 266
  for s in (0, 1, 2, 3, 256, 257, 264, 265):
    lit[s] = 3
  syms = [3] * 4 + [(18, 138), (18, 114)] + [3, 3] + [0, (17, 5)] + [3] + [(16, 6)] + [3, 3, 3]
  case('repeat_16_across_hlit', lit, [3] * 8, [0, 1, 2, 3, (3, 4), (10, 2), (12, 16)], clen_syms=syms)
  # Literals 0..5, end of block and length 3; zeros from entry 258 to the end of the 268
  # literal/length lengths and on over the first four distance lengths in ONE code 18.
  lit = [0] * 268
  for s in (0, 1, 2, 3, 4, 5, 256, 257):
    lit[s] = 3
  syms = [3] * 6 + [(18, 138), (18, 112)] + [3, 3] + [(18, 14), 1, 1]
  case('repeat_18_across_hlit', lit, [0, 0, 0, 0, 1, 1], [0, 1, 2, 3, 4, 5, (3, 5), (3, 7)],
       clen_syms=syms)
  # a single distance code of length 1: incomplete, and allowed (RFC 1951 3.2.7)
  lit = complete_lengths([0, 1, 2, 3, 256, 257, 258, 259], 260)
  case('single_distance_code', lit, [1], [0, 1, 2, 3, (3, 1), (5, 1)])
  # HDIST = 1 with length 0: literals only
  case('no_distance_code', lit, [0], [0, 1, 2, 3, 3, 2, 1])
  # The shortest header that can carry a non-zero length: HCLEN = 5 sends the code-length code's
  # lengths for 16, 17, 18, 0 and 8.  (HCLEN = 4 stops at symbol 0, and a header of zeros and
  # repeats of zero has no end-of-block code: hclen_4_stream() below, among the malformed ones.)
  clen = [0] * 19
  clen[17] = clen[18] = clen[0] = clen[8] = 2
  lit = [8] * 255 + [0, 8]                          # 0..254 and 256: 256 codes of length 8
  case('hclen_5', lit, [0], [0, 1, 2, 250, 254, 7], clen_syms=[8] * 255 + [0, 8, 0], clen_lens=clen,
       hclen=5)
  # HCLEN = 19 (symbol 15 is the last of CLEN_ORDER) and a 15-bit code: lengths 1..15 and a second 15
  lit = [0] * 257
  for k, s in enumerate([256, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]):
    lit[s] = min(k + 1, 15)
  case('fifteen_bit_code_hclen_19', lit, [0], [0, 14, 13, 5, 13, 14, 1], hclen=19,
       clen_lens=complete_lengths(range(16), 19))
  return out


def hclen_4_stream():
  """HCLEN = 4 sends lengths for the code-length symbols 16, 17, 18 and 0 only; with those, every
  literal/length length is zero.  A well-formed header that must end as NO_END_OF_BLOCK."""
  lens4 = [0] * 19
  lens4[17], lens4[18], lens4[0], lens4[16] = 2, 2, 2, 2
  w = BitWriter()
  dynamic_block(w, [0] * 257, [0], None, True, clen_syms=[(18, 138), (18, 109), (17, 10), 0],
                clen_lens=lens4, hclen=4)
  w.bits(0, 16)
  return zlib_frame(w.done() + bytes(4))


def bad_cases():
  """Malformed streams and streams that do not fit their geometry, with the status each must get."""
  rng = np.random.default_rng(77)
  text = _line(rng, 20000, b'etaoin sh')
  cases = []
  dyn = compress(text, 6)
  sto = compress(_line(rng, 5000), 0)
  # two scan lines of 10 000: a pitch the reconstruction kernel takes as well
  cases.append(_bad('truncated_at_1_byte', dyn[:1], 'TRUNCATED', len(text), 10000))
  cases.append(_bad('truncated_in_dynamic_header', dyn[:10], 'TRUNCATED', len(text), 10000))
  cases.append(_bad('truncated_in_stored_block', sto[:1000], 'TRUNCATED', 5000))
  cases.append(_bad('truncated_before_trailer_end', dyn[:-1], 'TRUNCATED', len(text), 10000))
  cases.append(_bad('truncated_to_nothing', b'', 'TRUNCATED', len(text), 10000))

  def framed(name, status, build, pad=8, **kw):
    w = BitWriter()
    build(w)
    cases.append(_bad(name, zlib_frame(w.done() + bytes(pad)), status, **kw))

  def type3(w):
    w.bits(1, 1)
    w.bits(3, 2)
  framed('block_type_3', 'BAD_BLOCK_TYPE', type3)
  framed('len_nlen_mismatch', 'BAD_STORED_LENGTH', lambda w: stored_block(w, b'abcd', True, nlen=0x1234))
  framed('distance_before_start', 'BAD_DISTANCE', lambda w: fixed_block(w, [0, 1, (3, 5)], True))
  framed('distance_before_start_at_0', 'BAD_DISTANCE', lambda w: fixed_block(w, [(3, 1)], True))
  over = [8] * 257 + [1]          # 257 codes of length 8 and one of length 1
  framed('over_subscribed_lengths', 'OVER_SUBSCRIBED', lambda w: dynamic_block(w, over, [0], None, True))
  inc = [0] * 257
  inc[0] = inc[256] = 2
  framed('incomplete_lengths', 'INCOMPLETE', lambda w: dynamic_block(w, inc, [0], None, True))
  two = [0] * 257
  two[0] = two[256] = 1
  framed('incomplete_distance_lengths', 'INCOMPLETE',
         lambda w: dynamic_block(w, two, [2, 2, 0, 0], None, True))
  framed('literal_symbol_286', 'BAD_CODE', lambda w: fixed_block(w, [0, ('lit', 286)], True))
  framed('distance_symbol_30', 'BAD_CODE', lambda w: fixed_block(w, [0, 1, 2, ('dist', 3, 30)], True))
  framed('distance_code_of_an_empty_set', 'BAD_CODE',
         lambda w: dynamic_block(w, complete_lengths([0, 1, 256, 257], 258), [0], [0, 1, ('lit', 257)],
                                 True, end=False))
  framed('repeat_without_previous', 'BAD_REPEAT',
         lambda w: dynamic_block(w, [0] * 257, [0], None, True, clen_syms=[(16, 3)] + [0] * 255))
  framed('repeat_past_the_end', 'BAD_REPEAT',
         lambda w: dynamic_block(w, [0] * 257, [0], None, True, clen_syms=[0] * 250 + [(18, 138)]))
  framed('too_many_length_symbols', 'BAD_COUNTS',
         lambda w: dynamic_block(w, [0] * 287, [0], None, True))
  cases.append(_bad('hclen_4_no_end_of_block', hclen_4_stream(), 'NO_END_OF_BLOCK'))
  # geometry
  good = _line(rng, 101, b'abc')
  cases.append(_bad('one_byte_longer_than_geometry', compress(good), 'TOO_LONG', 100, zlib_raises=False))
  cases.append(_bad('one_byte_shorter_than_geometry', compress(good), 'TOO_SHORT', 102, zlib_raises=False))
  cases.append(_bad('stored_longer_than_geometry', compress(good, 0), 'TOO_LONG', 100, zlib_raises=False))
  cases.append(_bad('wrong_adler', compress(good)[:-4] + struct.pack('>I', zlib.adler32(good) ^ 1),
                    'BAD_ADLER', 101))
  rows = np.zeros((4, 10), np.uint8)
  rows[:, 1:] = rng.integers(0, 256, (4, 9))
  rows[:, 0] = (1, 4, 5, 7)
  cases.append(_bad('filter_byte_5_in_row_2', compress(rows.tobytes()), 'BAD_FILTER', 40, pitch=10,
                    zlib_raises=False, detail=(5 << 8) | (2 << 16)))
  # zlib header
  raw = compress(good)[2:]

  def header(cmf, flags=0):      # FCHECK made valid
    v = (cmf << 8) | flags
    return struct.pack('>H', v + (31 - v % 31) % 31)
  cases.append(_bad('header_cm_7', header(0x77) + raw, 'BAD_HEADER', 101))
  cases.append(_bad('header_cinfo_8', header(0x88) + raw, 'BAD_HEADER', 101))
  cases.append(_bad('header_fdict', header(0x78, 0x20) + raw, 'BAD_HEADER', 101))
  cases.append(_bad('header_fcheck', b'\x78\x9d' + raw, 'BAD_HEADER', 101))
  return cases


def png_container(height, width, bit_depth, colour_type, idat: bytes) -> bytes:
  """A PNG file around an IDAT stream given as it is (tests/_png_ref.container compresses its own)."""
  def chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data))
  return (b'\x89PNG\r\n\x1a\n' +
          chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, bit_depth, colour_type, 0, 0, 0)) +
          chunk(b'IDAT', idat) + chunk(b'IEND', b''))


def corpus_file(cases) -> bytes:
  """The corpus in the format tools/inflate_host_check.cpp reads."""
  out = [b'INFC', struct.pack('<I', len(cases))]
  for c in cases:
    out.append(struct.pack('<IIIi', len(c.stream), c.expected_len, c.pitch, c.word))
    out.append(c.stream)
    if c.status == 'OK':
      out.append(c.data)
  return b''.join(out)
