"""The JPEG decoder without a GPU: the NumPy oracle of tests/_jpeg_ref.py against Pillow and against
the golden fixture Pillow wrote, the test writer against the oracle, `parse_jpeg` on what it must
refuse, the constants of the binding, and csrc/jpeg_core.h itself as a stand-alone host program
(tools/jpeg_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer: simulated lanes
run the speculation, the decoding from wrong states included, over the good and the malformed
corpus.  The same corpus runs on the device in tests/test_jpeg_gpu.py."""
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import _jpeg_ref as J
from se3ds_amd import _lib
from se3ds_amd.utils import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, 'se3ds_amd', 'csrc', 'jpeg_core.h')
SIZES = [(1, 1), (2, 3), (8, 8), (9, 17), (17, 33), (5, 4), (3, 5), (40, 2), (33, 6), (64, 48)]


def _core_constant(name):
  return int(re.search(rf'constexpr int {name} = (\d+);', open(CORE).read()).group(1))


def test_oracle_equals_pillow_bit_for_bit():
  """252 files: the sizes x (three samplings + optimize + two restart layouts + grey) x three
  qualities.  At quality 30 the source is posterised so that the coefficients stay moderate: Pillow
  comparisons use only files whose first-pass values fit int16 (beyond, its table look-up wraps)."""
  Image = pytest.importorskip('PIL.Image')
  rng = np.random.default_rng(0)
  n = 0
  for h, w in SIZES + [(16, 16), (37, 45)]:
    for kw in (dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, optimize=True),
               dict(subsampling=2, restart_marker_blocks=1), dict(subsampling=1, restart_marker_rows=1),
               dict(grey=True)):
      for quality in (30, 95, 100):
        kw2 = dict(kw)
        grey = kw2.pop('grey', False)
        a = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
        if quality == 30:
          a = (a // 64 * 64).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, 'JPEG', quality=quality, **kw2)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue()))).reshape(h, w, -1)
        stats = []
        got = J.decode(buf.getvalue(), stats=stats)
        assert max(s[0] for s in stats) < 2 ** 15
        assert got.shape == want.shape and np.array_equal(got, want), (h, w, kw, quality)
        n += 1
  assert n == 252


@pytest.fixture(scope='module')
def golden():
  z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  names = sorted(k[5:] for k in z.files if k.startswith('file_'))
  return {k: (z['file_' + k].tobytes(), z['pixels_' + k]) for k in names}


def test_oracle_equals_the_golden_fixture(golden):
  assert len(golden) >= 12
  seen = set()
  for name, (data, pixels) in golden.items():
    got = J.decode(data)
    assert got.shape == pixels.shape and np.array_equal(got, pixels), name
    scan = jpeg.parse_jpeg(data)
    assert (scan.height, scan.width, scan.components) == pixels.shape
    seen.add((scan.components, scan.h0, scan.v0, bool(scan.restart_interval)))
  assert {s[:3] for s in seen} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)} and any(s[3] for s in seen)


def test_writer_then_oracle_returns_the_coefficients():
  rng = np.random.default_rng(1)
  for sampling in J.SAMPLINGS:
    for h, w in ((1, 1), (9, 17), (33, 6), (40, 2)):
      for kw in ({}, dict(dri=1), dict(dri=3), dict(dqt16=True), dict(huffman=J.LONG_CODES), dict(sof='C1')):
        coefs = J.random_coefs(rng, h, w, sampling)
        written = J.write_jpeg(coefs, h, w, sampling, **kw)
        got, quants, frame = J.decode_coefficients(written.data)
        assert all(np.array_equal(g, c) for g, c in zip(got, coefs)), (sampling, h, w, kw)
        assert np.array_equal(J.decode(written.data), J.expected(coefs, h, w, sampling))
        scan = jpeg.parse_jpeg(written.data)
        assert tuple(scan.segments) == tuple(written.segments)
        assert (scan.height, scan.width, scan.components) == (h, w, J.SAMPLINGS[sampling][0])
        # the writer's report: every stuffed FF is an FF 00 in the segment, symbols are in order
        for (at, n), spans, ff in zip(written.segments, written.symbols, written.stuffed):
          seg = written.data[at:at + n]
          assert all(seg[o] == 0xFF and seg[o + 1] == 0 for o in ff) and seg.count(b'\xff') == len(ff)
          assert np.all(spans[:, 0] <= spans[:, 1]) and np.all(spans[1:, 0] > spans[:-1, 1])
  coefs = J.extreme_coefs(rng, 16, 32, '420')
  written = J.write_jpeg(coefs, 16, 32, '420')
  got, _, _ = J.decode_coefficients(written.data)
  assert all(np.array_equal(g, c) for g, c in zip(got, coefs))
  # the flat file is what the general writer makes of flat coefficients: 32 bits per MCU
  scan = jpeg.parse_jpeg(J.flat_420(32, 48, 5))
  assert scan.segments[0][1] == (36 + 32 * 5 + 7) // 8


def test_annex_k_tables_are_those_pillow_writes():
  Image = pytest.importorskip('PIL.Image')
  buf = io.BytesIO()
  Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, 'JPEG')
  tables = J.parse(buf.getvalue())[2]
  for (tc, th), (counts, values) in J.ANNEX_K.items():
    assert {(l, c): v for v, (c, l) in J.code_book(counts, values).items()} == tables[(tc << 4) | th]


def test_malformed_corpus_has_the_status_the_serial_decode_gives():
  bad = J.bad_cases()
  assert [c.name for c in bad] == ['truncated', 'undefined_code', 'run_past_63', 'zrl_past_63', 'dc_category_12',
                                   'block_too_many', 'damaged_byte']
  for c in bad:
    scan = jpeg.parse_jpeg(c.data)
    tables = J.parse(c.data)[2]
    at, n = scan.segments[0]
    blocks = scan.mcus_x * scan.mcus_y * scan.blocks_per_mcu
    assert J.scan_status(c.data[at:at + n], tables, [(0, 0)] * 4 + [(1, 1)] * 2, blocks) == c.status, c.name


def _small(sampling='420', w=16, **kw):
  rng = np.random.default_rng(5)
  return J.write_jpeg(J.random_coefs(rng, 16, w, sampling), 16, w, sampling, **kw).data


def _retag(data, old, new):
  i = data.index(old)
  return data[:i] + new + data[i + len(old):]


def test_parser_refuses_by_name():
  good = _small()
  scan = jpeg.parse_jpeg(good)
  assert (scan.h0, scan.v0, scan.restart_interval, len(scan.segments)) == (2, 2, 0, 1)
  sof = good.index(b'\xff\xc0')
  sos = good.index(b'\xff\xda')
  app14 = lambda transform: b'\xff\xee' + struct.pack('>H', 14) + b'Adobe' + bytes([0, 100, 0, 0, 0, 0, transform])
  com = b'\xff\xfe' + struct.pack('>H', 7) + b'hello'
  assert jpeg.parse_jpeg(good[:2] + com + app14(1) + good[2:]).segments[0][1] == scan.segments[0][1]
  four = good[:sof] + b'\xff\xc0' + struct.pack('>HBHHB', 8 + 12, 8, 16, 16, 4) + bytes(
      [1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0, 4, 0x11, 0]) + good[sos:]
  one_of_three = good[:sos] + b'\xff\xda' + struct.pack('>HB', 8, 1) + bytes([1, 0, 0, 63, 0]) + good[sos + 14:]
  end = len(good) - 2
  unsupported = [
      (_retag(good, b'\xff\xc0', b'\xff\xc2'), 'progressive'),
      (_retag(good, b'\xff\xc0', b'\xff\xc3'), 'lossless'),
      (_retag(good, b'\xff\xc0', b'\xff\xc9'), 'arithmetic'),
      (good[:sof + 4] + b'\x0c' + good[sof + 5:], '12-bit'),
      (four, 'four components'),
      (one_of_three, 'more than one scan'),
      (good[:end] + good[sos:], 'more than one scan'),
      (good[:2] + app14(0) + good[2:], 'Adobe APP14 transform 0'),
      (good[:sof + 11] + b'\x12' + good[sof + 12:], 'sampling 1x2'),
      (good[:sof + 11] + b'\x41' + good[sof + 12:], 'sampling 4x1'),
      (good[:sof + 14] + b'\x21' + good[sof + 15:], 'sampling 2x2, 2x1'),
  ]
  for data, kind in unsupported:
    with pytest.raises(NotImplementedError, match=kind):
      jpeg.parse_jpeg(data)
  dqt = good.index(b'\xff\xdb')
  dht = good.index(b'\xff\xc4')
  malformed = [
      (b'\x00' + good[1:], 'no SOI'),
      (good[:sof] + good[sos:], 'no SOF'),
      (good[:sos], 'no SOS'),
      (good[:sos] + b'\xff\xd9', 'no SOS'),
      (good[:-2], 'no EOI'),
      (good[:sof + 2] + b'\xff\xff' + good[sof + 4:], 'leaves the file'),
      (good[:dqt] + good[sof:], 'quantisation table 0 is missing'),
      (good[:dht] + good[sos:], 'Huffman table 0 is missing'),
      (good[:sof + 5] + b'\x00\x00' + good[sof + 7:], 'zero size'),
      (good[:sof + 7] + b'\x00\x00' + good[sof + 9:], 'zero size'),
      (_small(w=32, dri=1).replace(b'\xff\xd0', b'\xff\xd3'), 'RST3 where RST0 is due'),
      (_retag(_small(w=32, dri=1), b'\xff\xdd\x00\x04\x00\x01', b'\xff\xdd\x00\x04\x00\x02'), 'entropy segments'),
      (good[:dht + 5] + b'\x03' + good[dht + 6:], 'no prefix code'),
  ]
  for data, kind in malformed:
    with pytest.raises(ValueError, match=kind):
      jpeg.parse_jpeg(data)


def test_a_progressive_file_from_pillow_is_refused_by_name():
  Image = pytest.importorskip('PIL.Image')
  buf = io.BytesIO()
  Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, 'JPEG', progressive=True)
  with pytest.raises(NotImplementedError, match='progressive'):
    jpeg.parse_jpeg(buf.getvalue())
  buf = io.BytesIO()
  Image.fromarray(np.zeros((16, 16, 4), np.uint8), 'CMYK').save(buf, 'JPEG')
  with pytest.raises(NotImplementedError, match='four components'):
    jpeg.parse_jpeg(buf.getvalue())


def test_binding_constants_and_no_cpu_fallback():
  L = _lib.lib()
  assert L.se3ds_jpeg_decode_lanes() == _core_constant('kLanes') == 256
  assert L.se3ds_jpeg_decode_chunk_bytes() == _core_constant('kChunkBytes') == 128
  assert L.se3ds_jpeg_decode_fields() == _core_constant('kImageFields')
  assert L.se3ds_jpeg_decode_segment_fields() == _core_constant('kSegmentFields')
  text = open(CORE).read()
  names = re.findall(r'^\s+([A-Z_]+) = (\d+),', text[text.index('enum class Status'):text.index('constexpr int kLanes')],
                     flags=re.M)
  assert [n for n, _ in names] == J.STATUS and [int(v) for _, v in names] == list(range(len(J.STATUS)))
  assert [s.name for s in jpeg.JpegStatus] == J.STATUS
  for i in range(1, len(J.STATUS)):
    assert jpeg.jpeg_failure(i | (77 << 8)).startswith('the scan does not decode: ')
  assert list(jpeg.status_rounds([5 | (77 << 8), 3 << 8])) == [77, 3]
  with pytest.raises(_lib.Se3dsHipError):
    jpeg.decode_jpeg_batch([_small()], torch.device('cpu'))
  with pytest.raises(_lib.Se3dsHipError):
    jpeg.decode_jpeg_batch([_small()], 'cpu', check=False)
  # the workspace query is host arithmetic: 6 blocks of 128 bytes and 16 x 16 + 2 x 8 x 8 samples
  scan = jpeg.parse_jpeg(_small())
  row = np.zeros(200, np.int64)
  row[:5] = (16, 16, 3, 2, 2)
  row[6], row[11], row[12] = 3, 1, 1
  assert L.se3ds_jpeg_decode_workspace_bytes(row.ctypes.data, 1) == 6 * 128 + 256 + 128
  assert scan.blocks_per_mcu == 6


def test_decoder_core_as_a_sanitised_host_program(tmp_path):
  """tools/jpeg_host_check.cpp includes csrc/jpeg_core.h and simulates 1, 4, 64 (16-byte chunks), 8
  and 256 (128-byte chunks) lanes.  Built with AddressSanitizer + UndefinedBehaviorSanitizer
  (reports are fatal) it must reproduce the pixels of every good file, give every malformed one its
  status, keep the bound on the rounds, and exit clean.  A program with its own main, run directly:
  nothing is preloaded."""
  good, bad = J.good_cases(), J.bad_cases()
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the decoder core cannot be checked on the host'
  exe = str(tmp_path / 'jpeg_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'jpeg_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  corpus = tmp_path / 'corpus.bin'
  corpus.write_bytes(J.corpus_file(good, bad))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert f'{len(good) + len(bad)} cases x 5 configurations x 2 alignments OK' in r.stdout
  # the checker does fail when it should: one flipped expectation, one flipped pixel
  corpus.write_bytes(J.corpus_file(good[:1], [bad[0]._replace(status='BAD_RUN')]))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 1 and 'status 1, expected 3' in r.stderr
  case, px = good[0]
  px = px.copy()
  px[0, 0, 0] ^= 1
  corpus.write_bytes(J.corpus_file([(case, px)], []))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 1 and 'pixels differ' in r.stderr
