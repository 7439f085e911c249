"""The JPEG encoder without a GPU: the NumPy oracle of tests/_jpeg_encode_ref.py against Pillow byte
for byte, the package's tables and container against Pillow's files, the golden fixture against its
generator, the argument checks of encode_jpeg_batch, and csrc/jpeg_encode_core.h itself as a
stand-alone host program (tools/jpeg_encode_host_check.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The device runs the same cases in tests/test_jpeg_encode_gpu.py."""
import importlib.util
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import _jpeg_encode_ref as E
import _jpeg_ref as J
from se3ds_amd import _lib
from se3ds_amd.utils import jpeg, logger as logger_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 3), (8, 8), (8, 17), (9, 20), (20, 9), (33, 47), (40, 40), (17, 250), (64, 96)]
QUALITIES = [1, 10, 25, 50, 75, 90, 100]
SAMPLINGS = ['grey', '4:4:4', '4:2:2', '4:2:0']
SCENES = ['smooth', 'noise', 'mixed', 'constant', 'checker']
RESTARTS = [0, 1, 2, 'row']


def _pillow(px, quality, sampling, restart=0):
  Image = pytest.importorskip('PIL.Image')
  kw = {} if sampling == 'grey' else {'subsampling': sampling}
  if restart == 'row':
    kw['restart_marker_rows'] = 1
  elif restart:
    kw['restart_marker_blocks'] = restart
  buf = io.BytesIO()
  Image.fromarray(px[..., 0] if px.shape[2] == 1 else px).save(buf, 'JPEG', quality=quality, **kw)
  return buf.getvalue()


def test_oracle_equals_pillow_byte_for_byte():
  """10 sizes x 7 qualities x 4 samplings x 5 scenes x 4 restart layouts = 5600 files, none excluded."""
  pytest.importorskip('PIL.Image')
  n = 0
  for h, w in SIZES:
    for sampling in SAMPLINGS:
      for kind in SCENES:
        px = E.scene(kind, h, w, 1 if sampling == 'grey' else 3, seed=h + w)
        for quality in QUALITIES:
          for restart in RESTARTS:
            got = E.encode(px, quality, '4:2:0' if sampling == 'grey' else sampling, restart)
            assert got == _pillow(px, quality, sampling, restart), (h, w, sampling, kind, quality, restart)
            n += 1
  assert n == 5600


def test_quality_tables_are_the_dqt_pillow_writes():
  pytest.importorskip('PIL.Image')
  px = np.zeros((8, 8, 3), np.uint8)
  for q in range(1, 101):
    quant = J.parse(_pillow(px, q, '4:2:0'))[1]
    for mine in (jpeg.quality_tables(q), E.quality_tables(q)):
      assert np.array_equal(mine[0], quant[0]) and np.array_equal(mine[1], quant[1]), q
  for bad in (0, 101, 75.0, True, None):
    with pytest.raises(ValueError, match='quality'):
      jpeg.quality_tables(bad)


def _generator():
  spec = importlib.util.spec_from_file_location('make_jpeg_encode_golden',
                                                os.path.join(ROOT, 'tools', 'make_jpeg_encode_golden.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


def test_golden_fixture_is_what_the_generator_writes_today():
  pytest.importorskip('PIL.Image')
  gen = _generator()
  assert os.path.getsize(gen.PATH) < 300 * 1024
  z = np.load(gen.PATH)
  want = gen.build()
  assert sorted(z.files) == sorted(want)
  for k, v in want.items():
    assert z[k].dtype == v.dtype and np.array_equal(z[k], v), k
  params = z['params'].tolist()
  assert len(params) == 178 and {tuple(p[:2]) for p in params} == set(SIZES) | {(40, 72)}
  assert {p[5] for p in params} == {0, 1, 2, -1, 65535}


def test_the_decoder_oracle_reads_the_encoder_oracle():
  Image = pytest.importorskip('PIL.Image')
  for (h, w), sampling, restart in zip(SIZES, SAMPLINGS * 3, RESTARTS * 3):
    px = E.scene('mixed', h, w, 1 if sampling == 'grey' else 3, seed=3)
    data = E.encode(px, 85, '4:2:0' if sampling == 'grey' else sampling, restart)
    want = np.asarray(Image.open(io.BytesIO(data))).reshape(h, w, -1)
    assert np.array_equal(J.decode(data), want), (h, w, sampling, restart)
    scan = jpeg.parse_jpeg(data)
    assert (scan.height, scan.width, scan.components) == px.shape


def test_container_layout():
  """SOI, APP0 JFIF 1.01, a DQT per table, SOF0, DHT in the order DC0 AC0 DC1 AC1, DRI only with an
  interval, SOS, data, EOI -- and the package's container equals the oracle's and Pillow's."""
  px = E.scene('mixed', 20, 9, 3)
  coefs, tables = E.coefficients(px, 75, '420')
  for restart in (0, 2):
    data = E.entropy(coefs, '420', restart)
    f = jpeg.jpeg_container(20, 9, 3, 2, 2, jpeg.quality_tables(75), restart, data)
    assert f == E.container(20, 9, '420', tables, restart, data) == _pillow(px, 75, '4:2:0', restart)
    markers, p = [], 2
    while f[p + 1] != 0xDA:
      markers.append((f[p + 1], f[p + 4] if f[p + 1] in (0xDB, 0xC4) else None))
      p += 2 + struct.unpack('>H', f[p + 2:p + 4])[0]
    want = [(0xE0, None), (0xDB, 0), (0xDB, 1), (0xC0, None), (0xC4, 0x00), (0xC4, 0x10), (0xC4, 0x01), (0xC4, 0x11)]
    assert markers == want + ([(0xDD, None)] if restart else [])
    assert f[:2] == b'\xff\xd8' and f[2:20] == b'\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
    sof = f.index(b'\xff\xc0')
    assert f[sof + 4:sof + 19] == bytes([8, 0, 20, 0, 9, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]) and f[-2:] == b'\xff\xd9'
  grey = E.scene('smooth', 9, 20, 1)
  g = jpeg.jpeg_container(9, 20, 1, 1, 1, jpeg.quality_tables(50), 0, E.entropy(E.coefficients(grey, 50, 'grey')[0], 'grey'))
  assert g == _pillow(grey, 50, 'grey') and g.count(b'\xff\xc4') == 2 and g.count(b'\xff\xdb') == 1
  with pytest.raises(ValueError, match='jpeg_container'):
    jpeg.jpeg_container(8, 8, 1, 2, 2, jpeg.quality_tables(50), 0, b'')
  assert [t[0] for t in jpeg.HUFFMAN_TABLES] == [0x00, 0x10, 0x01, 0x11]
  for (tag, counts, values), key in zip(jpeg.HUFFMAN_TABLES, ((0, 0), (1, 0), (0, 1), (1, 1))):
    assert (list(counts), list(values)) == (J.ANNEX_K[key][0], J.ANNEX_K[key][1])


def test_argument_errors_need_no_device():
  x = torch.zeros((16, 24, 3), dtype=torch.uint8)
  assert jpeg.encode_jpeg_batch([]) == []
  bad = [
      (dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(quality=75.5), 'quality'),
      (dict(quality=[75, 80]), 'quality'), (dict(quality=[True]), 'quality'),
      (dict(subsampling='4:1:1'), 'subsampling'), (dict(subsampling=2), 'subsampling'),
      (dict(restart_interval=-1), 'restart_interval'), (dict(restart_interval=65536), 'restart_interval'),
      (dict(restart_interval='rows'), 'restart_interval'), (dict(restart_interval=1.5), 'restart_interval'),
  ]
  for kw, name in bad:
    with pytest.raises(ValueError, match=name):
      jpeg.encode_jpeg_batch([x], **kw)
  for t in (torch.zeros((16, 24), dtype=torch.uint8), torch.zeros((16, 24, 2), dtype=torch.uint8),
            torch.zeros((16, 24, 3)), torch.zeros((0, 24, 3), dtype=torch.uint8),
            torch.zeros((1, 65536, 1), dtype=torch.uint8), torch.zeros((65536, 1, 1), dtype=torch.uint8)):
    with pytest.raises(ValueError, match='images'):
      jpeg.encode_jpeg_batch([t])
  with pytest.raises(ValueError, match='images'):
    jpeg.encode_jpeg_batch([x], device='cuda')
  with pytest.raises(_lib.Se3dsHipError):   # valid arguments, no device: there is no CPU encoder
    jpeg.encode_jpeg_batch([x], quality=[90], restart_interval='row')
  specs = jpeg.encode_specs([(16, 24, 3), (9, 20, 1)], [torch.uint8] * 2, [75, 90], '4:2:2', 'row')
  assert [(s.h0, s.v0, s.restart_interval, s.blocks) for s in specs] == [(2, 1, 2, 16), (1, 1, 3, 6)]
  with pytest.raises(ValueError, match='image_format'):
    logger_lib.UniversalLogger('unused', 0, image_format='gif')
  with pytest.raises(ValueError, match="encoder='device'"):
    logger_lib.UniversalLogger('unused', 0, encoder='host', image_format='jpeg')
  with pytest.raises(ValueError, match='quality'):
    logger_lib.UniversalLogger('unused', 0, image_format='jpeg', jpeg_quality=0)


def test_binding_constants_and_host_side_sizes():
  L = _lib.lib()
  text = open(os.path.join(ROOT, 'se3ds_amd', 'csrc', 'jpeg_encode_core.h')).read()
  const = lambda name: int(__import__('re').search(rf'constexpr int {name} = (\d+);', text).group(1))
  assert L.se3ds_jpeg_encode_fields() == const('kFields') == 48
  assert L.se3ds_jpeg_encode_scan_group_blocks() == const('kScanGroup')
  assert L.se3ds_jpeg_encode_pack_unit_blocks() == const('kPackBlocks')
  assert L.se3ds_jpeg_encode_block_words() == 52
  assert L.se3ds_jpeg_encode_tile_blocks() == const('kTileBlocks') == 240
  row = E.table_row(16, 24, '420', E.quality_tables(75), 0).reshape(1, 48)
  row[0, 0] = 4096   # any non-null address: the size queries are host arithmetic
  # 2 x 1 MCUs of 6 blocks: out <= 2 * (12 * 208 + 1) + 2, rounded up to 16
  assert L.se3ds_jpeg_encode_out_bytes(row.ctypes.data, 1) == (12 * 416 + 4 + 15) & ~15
  assert L.se3ds_jpeg_encode_workspace_bytes(row.ctypes.data, 1) >= 12 * (128 + 208 + 2 + 8)
  row[0, 4] = 4
  assert L.se3ds_jpeg_encode_out_bytes(row.ctypes.data, 1) == 0
  assert L.se3ds_jpeg_encode_workspace_bytes(row.ctypes.data, 1) == 0


def test_encoder_core_as_a_sanitised_host_program(tmp_path):
  """tools/jpeg_encode_host_check.cpp includes csrc/jpeg_encode_core.h and drives transform, measure
  (the group scan as the kernel does it) and pack lane by lane with 4, 64 and 256 lanes, every case
  alone and all as one batch.  Built with AddressSanitizer + UndefinedBehaviorSanitizer (reports
  are fatal), it must reproduce the oracle's entropy-coded bytes and exit clean.  A program with
  its own main, run directly: nothing is preloaded."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the encoder core cannot be checked on the host'
  exe = str(tmp_path / 'jpeg_encode_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'jpeg_encode_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  cases = E.corpus_cases()
  corpus = tmp_path / 'corpus.bin'
  corpus.write_bytes(E.corpus_file(cases))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert f'{len(cases)} cases x 3 lane counts, alone and as one batch OK' in r.stdout
  # the checker does fail when it should: one flipped pixel
  px = cases[5][0].copy()
  px[0, 0, 0] ^= 0x80
  data = bytearray(E.corpus_file([cases[5]]))
  at = data.index(cases[5][0].tobytes())
  data[at:at + px.size] = px.tobytes()
  corpus.write_bytes(bytes(data))
  r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
  assert r.returncode == 1 and ('bytes differ' in r.stderr or 'expected' in r.stderr), r.stderr
