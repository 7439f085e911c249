"""The device inflate's decoder without a GPU: the hand-built corpus of tests/_deflate_ref.py against
CPython's zlib, `parse_png_container` against `parse_png`, and csrc/inflate_core.h itself as a
stand-alone host program (tools/inflate_host_check.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer over the whole corpus -- the malformed streams included, which is where
an out-of-bounds access would show.  The same corpus runs on the device in tests/test_inflate_gpu.py."""
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import _deflate_ref as D
import _png_ref
from se3ds_amd import _lib
from se3ds_amd.utils import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, 'se3ds_amd', 'csrc', 'inflate_core.h')


def _core_constant(name):
  return int(re.search(rf'constexpr uint32_t {name} = (\d+);', open(CORE).read()).group(1))


@pytest.fixture(scope='module')
def cases():
  return D.good_cases(_core_constant('kRingBytes')), D.bad_cases()


def test_helper_constants_match_the_core():
  assert D.GRANULE == _core_constant('kGranule')
  text = open(CORE).read()
  names = re.findall(r'^\s+([A-Z_]+) = (\d+),', text[text.index('enum class Status'):], flags=re.M)
  assert [n for n, _ in names] == D.STATUS and [int(v) for _, v in names] == list(range(len(D.STATUS)))
  assert [s.name for s in png.InflateStatus] == D.STATUS
  assert [int(s) for s in png.InflateStatus] == list(range(len(D.STATUS)))


def test_good_corpus_inflates_under_zlib_to_the_intended_bytes(cases):
  good, _ = cases
  assert len({c.name for c in good}) == len(good) >= 35
  for c in good:
    assert zlib.decompress(c.stream) == c.data, c.name
    assert c.expected_len == len(c.data) and c.expected_len % c.pitch == 0 and c.pitch >= 2, c.name


def test_malformed_corpus_is_rejected_by_zlib(cases):
  _, bad = cases
  for c in bad:
    assert c.status != 'OK' and c.expected_len % c.pitch == 0 and c.pitch >= 2, c.name
    if c.zlib_raises:
      with pytest.raises(zlib.error):
        zlib.decompress(c.stream)
    else:   # a sound stream that does not fit the geometry, or carries a bad filter type
      data = zlib.decompress(c.stream)
      assert len(data) != c.expected_len or c.status == 'BAD_FILTER', c.name


def test_hand_built_blocks_are_what_they_claim():
  """The writer against zlib on blocks whose content is known by construction."""
  items = [0, 7, 7, (5, 1), (3, 7), 200, (258, 2)]
  w = D.BitWriter()
  D.fixed_block(w, items, True)
  assert zlib.decompress(D.zlib_frame(w.done(), D.expand_items(items))) == D.expand_items(items)
  assert D.expand_items([1, 2, (4, 2)]) == bytes([1, 2, 1, 2, 1, 2])
  assert D.canonical([2, 1, 3, 3]) == {0: (0b10, 2), 1: (0b0, 1), 2: (0b110, 3), 3: (0b111, 3)}   # RFC 3.2.2
  assert D.complete_lengths([5, 9, 11], 12) == [0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 2]


def test_container_walk_agrees_with_parse_png():
  rng = np.random.default_rng(3)
  for pixels in (rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (4, 9), dtype=np.uint8),
                 rng.integers(0, 65536, (3, 2)).astype(np.uint16)):
    buf = _png_ref.encode_png(pixels, rng.integers(0, 5, pixels.shape[0]), idat_split=3)
    plane, stream = png.parse_png(buf), png.parse_png_container(buf)
    assert isinstance(stream, png.PngStream) and stream[:4] == plane[:4]
    assert (stream.row_bytes, stream.bytes_per_pixel) == (plane.row_bytes, plane.bytes_per_pixel)
    assert zlib.decompress(stream.compressed) == plane.filtered
  good = _png_ref.container(2, 2, 8, 0, bytes(6))
  sig = good[:8]
  ihdr_end = 8 + 25
  broken = [
      b'\x88' + good[1:],                                           # signature
      good[:40],                                                    # truncated chunk
      good[:20] + bytes([good[20] ^ 1]) + good[21:],                # CRC
      sig + good[ihdr_end:],                                        # first chunk is not IHDR
      good[:-12],                                                   # no IEND
      sig + good[8:ihdr_end] + good[-12:],                          # no IDAT
      good[:ihdr_end] + _png_ref.chunk(b'XYZW', b'') + good[ihdr_end:],   # unknown critical chunk
      _png_ref.container(0, 2, 8, 0, bytes(6)),                     # zero width
      _png_ref.container(2, 2, 3, 0, bytes(6)),                     # not a PNG kind
  ]
  unsupported = [_png_ref.container(2, 2, 8, 6, bytes(18)), _png_ref.container(2, 2, 8, 0, bytes(6), interlace=1),
                 _png_ref.container(2, 2, 4, 0, bytes(4))]
  for buf, kind in [(b, ValueError) for b in broken] + [(b, NotImplementedError) for b in unsupported]:
    with pytest.raises(kind) as a:
      png.parse_png(buf)
    with pytest.raises(kind) as b:
      png.parse_png_container(buf)
    assert str(a.value) == str(b.value)
  # what only the inflate can see is not the container walk's to report
  short = D.png_container(2, 2, 8, 0, zlib.compress(bytes(5)))
  with pytest.raises(ValueError, match='5 inflated bytes'):
    png.parse_png(short)
  assert png.parse_png_container(short).compressed == zlib.compress(bytes(5))


def test_inflate_argument_is_checked_before_the_device():
  with pytest.raises(ValueError, match='inflate'):
    png.decode_png_batch({'x': [b'']}, torch.device('cpu'), inflate='gpu')
  with pytest.raises(_lib.Se3dsHipError):
    png.decode_png_batch({'x': [_png_ref.container(1, 1, 8, 0, bytes(2))]}, torch.device('cpu'),
                         inflate='device')
  with pytest.raises(_lib.Se3dsHipError):
    png.decode_png_batch_async({'x': [_png_ref.container(1, 1, 8, 0, bytes(2))]}, 'cpu')
  L = _lib.lib()
  assert L.se3ds_png_inflate_fields() == 5
  ring = L.se3ds_png_inflate_ring_bytes()
  assert ring == _core_constant('kRingBytes') and ring & (ring - 1) == 0 and ring >= 32768 + D.GRANULE + 258


def test_failure_messages():
  s = png.PngStream(4, 9, 8, 1, b'')
  word = D.STATUS.index('BAD_FILTER') | (5 << 8) | (2 << 16)
  assert png.inflate_failure(word, s) == 'filter type 5 in row 2'
  assert png.inflate_failure(D.STATUS.index('BAD_DISTANCE'), s) == \
      'the IDAT stream does not inflate: distance beyond the start of the output'
  assert png.inflate_failure(D.STATUS.index('TOO_LONG'), s) == 'more inflated bytes than 4 x (1 + 9)'
  for i in range(1, len(D.STATUS)):
    assert png.inflate_failure(i, s)


def test_decoder_core_as_a_sanitised_host_program(cases, tmp_path):
  """tools/inflate_host_check.cpp includes csrc/inflate_core.h with the one-lane host policy.  Built
  with AddressSanitizer + UndefinedBehaviorSanitizer (reports are fatal) it must reproduce every
  good stream byte for byte, give every malformed one its status, and exit clean."""
  good, bad = cases
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the decoder core cannot be checked on the host'
  exe = str(tmp_path / 'inflate_host_check')
  # the sanitizer runtimes linked statically (clang's default): the program stands alone
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'inflate_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  corpus = tmp_path / 'corpus.bin'
  corpus.write_bytes(D.corpus_file(good + bad))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert f'{len(good) + len(bad)} cases x 2 alignments OK' in r.stdout
  # the checker does fail when it should: one flipped expectation
  wrong = good[:1] + [bad[0]._replace(status='BAD_ADLER')]
  corpus.write_bytes(D.corpus_file(wrong))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected 14' in r.stderr
