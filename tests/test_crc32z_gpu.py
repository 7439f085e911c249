"""The device zip / zlib CRC-32 (se3ds_crc32z_multi, utils/crc32c.crc32z_device) on an MI355X.  Every
comparison is exact equality; the yardstick is `zlib.crc32(data, seed)`."""
import zlib

import numpy as np
import pytest
import torch

from se3ds_amd import _lib
from se3ds_amd.utils import crc32c as C

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SEEDS = (0, 0xffffffff, 0x1badb002)


def _block():
  return _lib.lib().se3ds_crc32z_block_bytes()


def _lengths():
  b = _block()
  return (list(range(10)) + [15, 16, 17, 63, 64, 65, 255, 256, 257] +
          [b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1, 3 * b + 5])


def _layout(aligns):
  """Disjoint ranges: every length of the sweep at every start alignment (mod 16) of `aligns`, a gap
  of at least one byte between neighbours.  -> (offsets, lengths, buffer size)"""
  offs, lens, pos = [], [], 0
  for n in _lengths():
    for a in aligns:
      pos = (pos + 1 + 15) // 16 * 16 + a
      offs.append(pos)
      lens.append(n)
      pos += n
  return offs, lens, pos + 3


def _device(data, offs, lens, seeds=None):
  buf = torch.from_numpy(np.array(data, dtype=np.uint8)).to(DEV)
  return C.crc32z_device(buf, offs, lens, seeds).tolist()


def _host(raw, offs, lens, seeds):
  return [zlib.crc32(raw[o:o + n], s) for o, n, s in zip(offs, lens, seeds)]


@pytest.fixture(scope='module')
def sweep():
  """Random bytes, the full length x alignment layout, each range once per seed, in one table."""
  offs, lens, size = _layout(range(16))
  data = np.random.default_rng(7).integers(0, 256, size, dtype=np.uint8)
  offs, lens, seeds = offs * len(SEEDS), lens * len(SEEDS), [s for s in SEEDS for _ in offs]
  return data, offs, lens, seeds, _host(data.tobytes(), offs, lens, seeds)


def test_known_answers_on_the_device():
  assert _lib.lib().se3ds_crc32z_fields() == 3 and 0 < _block() <= 1 << 20
  digits = np.frombuffer(b'123456789', np.uint8)
  assert _device(digits, [0], [9]) == [0xCBF43926]
  first = _device(digits, [0], [5])[0]
  assert _device(digits, [5, 0, 9], [4, 0, 0], [first, 77, 0]) == [0xCBF43926, 77, 0]   # continued; empty
  assert _device(digits, [0], [9], np.array([0], np.uint32)) == [0xCBF43926]


def test_length_alignment_and_seed_sweep(sweep):
  data, offs, lens, seeds, want = sweep
  got = _device(data, offs, lens, seeds)
  bad = [(o % 16, n, hex(s), hex(g), hex(w)) for o, n, s, g, w in zip(offs, lens, seeds, got, want) if g != w]
  assert not bad, bad[:8]
  assert sorted({o % 16 for o in offs}) == list(range(16))
  assert [g for g, n in zip(got, lens) if n == 0] == [s for s, n in zip(seeds, lens) if n == 0]


def test_constant_data_isolates_the_length_term():
  """All-zero and all-0xff data: the CRC depends on the length and the seed alone, so a wrong
  x^(8 L) of this polynomial shows."""
  offs, lens, size = _layout((0, 5, 11))
  seeds = [SEEDS[i % 3] for i in range(len(offs))]
  for fill in (0, 255):
    data = np.full(size, fill, np.uint8)
    assert _device(data, offs, lens, seeds) == _host(data.tobytes(), offs, lens, seeds), fill


def test_isolation(sweep):
  data, offs, lens, seeds, want = sweep
  inside = np.zeros(data.size, bool)
  for o, n in zip(offs, lens):
    inside[o:o + n] = True
  other = data.copy()
  other[~inside] ^= 0xff                     # differs in every byte outside the ranges
  assert (~inside).sum() >= len(offs) // len(SEEDS)
  assert _device(other, offs, lens, seeds) == want
  for k in (lens.index(1), lens.index(257) + 3, len(lens) - 1, lens.index(_block()) + 9):
    flipped = data.copy()
    flipped[offs[k] + lens[k] // 2] ^= 0x04
    got = _device(flipped, offs, lens, seeds)
    same = [i for i in range(len(offs)) if offs[i] == offs[k]]   # the range under every seed
    assert all(got[i] != want[i] for i in same)
    assert all(got[i] == want[i] for i in range(len(offs)) if i not in same)


def test_mixed_launch_and_overlap():
  """One launch: a multi-block range, a thousand tiny ones, overlaps, empty ranges and ranges that
  end at the buffer's last byte."""
  b = _block()
  rng = np.random.default_rng(9)
  size = 5 * b + 77 + 40001
  data = rng.integers(0, 256, size, dtype=np.uint8)
  raw = data.tobytes()
  offs, lens, seeds = [], [], []

  def add(o, n, s=None):
    offs.append(o), lens.append(n), seeds.append(int(rng.integers(0, 2 ** 32)) if s is None else s)

  for i in range(1000):
    n = int(rng.integers(0, 41))
    add(int(rng.integers(0, size - n + 1)), n)
    if i == 500:
      add(17, 5 * b + 77)                    # the multi-block range in the middle of the table
    if i % 100 == 0:
      add(i, 0), add(size, 0)                # empty, also at the very end
  add(size - 1, 1), add(size - (2 * b + 3), 2 * b + 3), add(0, size, 0)   # end at the last byte
  o, n, h = 1001, 2 * b + 77, b + 13         # a range and its two halves: the second continues the first
  add(o, n, 0), add(o, h, 0)
  first = zlib.crc32(raw[o:o + h])
  add(o + h, n - h, first)
  got = _device(data, offs, lens, seeds)
  assert got == _host(raw, offs, lens, seeds)
  assert got[-1] == got[-3] and got[-2] == first


@pytest.mark.parametrize('size', [4 * 300 + 1, 4 * 300 + 2, 4 * 300 + 3, 13, 16 * 70 + 13, 16 * 2048 + 13])
def test_buffer_end(size):
  """Buffers of 1, 2, 3 mod 4 and of 13 mod 16 bytes, the last beyond two blocks: ranges that end on
  the last byte and ranges that start at byte 0 -- a 4- or 16-byte load past the range would leave
  the buffer."""
  data = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
  offs = [0, 0, size - 1, size // 2, 3, 0, size - 7]
  lens = [size, size - 1, 1, size - size // 2, size - 3, 5, 7]
  seeds = [0, 1, 2, 0xffffffff, 4, 5, 0x80000000]
  assert _device(data, offs, lens, seeds) == _host(data.tobytes(), offs, lens, seeds)


def test_the_entry_refuses_a_range_that_leaves_the_buffer():
  L = _lib.lib()
  buf = torch.arange(100, dtype=torch.uint8, device=DEV)
  crc = torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
  ws_bytes = int(L.se3ds_crc32z_workspace_bytes(200, 2))
  ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=DEV)
  stream = torch.cuda.current_stream().cuda_stream

  def call(table):
    t = np.asarray(table, np.int64).reshape(-1, 3)
    td = torch.from_numpy(t).to(DEV)
    rc = L.se3ds_crc32z_multi(buf.data_ptr(), 100, td.data_ptr(), t.ctypes.data, 2, crc.data_ptr(),
                              ws.data_ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    return rc

  cases = [call([[0, 101, 0], [0, 0, 0]]), call([[0, 0, 0], [100, 1, 0]]), call([[-1, 4, 0], [0, 0, 0]]),
           call([[96, 8, 0], [0, 0, 0]]), call([[0, 4, 2 ** 32], [0, 0, 0]])]
  assert cases == [-1] * len(cases)
  assert crc.tolist() == [0x5a5a5a5a] * 2 and not ws.any()   # nothing was launched
  assert call([[0, 100, 0], [99, 1, 7]]) == 0
  raw = bytes(range(100))
  assert crc.cpu().numpy().view(np.uint32).tolist() == [zlib.crc32(raw), zlib.crc32(raw[99:], 7)]
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    C.crc32z_device(buf, [50], [51])
  assert C.crc32z_device(buf, [], []).shape == (0,)
  assert C.crc32z_device(buf[:0], [0, 0], [0, 0], [5, 6]).tolist() == [5, 6]
