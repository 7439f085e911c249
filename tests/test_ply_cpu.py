"""se3ds_amd.utils.ply without a GPU: csrc/ply_format_core.h as a stand-alone host program
(tools/ply_format_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, its text
against Python's own for the adversarial values, the reader, the host encoder, and the argument checks
of the wrapper and of the entry points (all of which run before any HIP call).  The device runs are
tests/test_ply_gpu.py."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _ply_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADSHAPE, BADDTYPE, WORKSPACE = -1, -2, -3


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
  """The sanitised program, built once.  No sanitizer touches code loaded into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the formatting core cannot be checked on the host'
  exe = str(tmp_path_factory.mktemp('ply') / 'ply_format_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'ply_format_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  return exe


def test_core_as_a_sanitised_host_program(host_check):
  """Digits and exponent against std::to_chars, the text back through strtod, every text in a heap
  block of exactly its length; reports are fatal."""
  r = subprocess.run([host_check], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  m = re.search(r'ply_format_host_check: (\d+) cases OK', r.stdout)
  # 277 powers of two x 3 x 2 signs, 2047 strided subnormals x 2, the multiples of 4099, 84 decades x 3
  # x 2, 15 + 9 x 4 integers, the longest line, 204 exponents of the logarithms
  assert m and int(m.group(1)) == 277 * 6 + 2047 * 2 + (2 ** 32 - 1) // 4099 + 1 + 84 * 6 + 15 + 36 + 1 + 204
  # the checker does fail when it should: one entry of the powers-of-5 table flipped
  r = subprocess.run([host_check, 'corrupt'], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected' in r.stderr


def test_text_equals_pythons(host_check, tmp_path):
  """Python is the oracle of the layout: the program's text of the adversarial set and of 2^16
  random bit patterns equals '{}'.format(np.float32(...)) string for string."""
  rng = np.random.default_rng(7)
  bits = np.concatenate([R.adversarial_bits(), rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])
  out = str(tmp_path / 'dump.txt')
  r = subprocess.run([host_check, 'dump', out], input=''.join('%08x\n' % b for b in bits), capture_output=True,
                     text=True)
  assert r.returncode == 0, r.stderr
  lines = open(out).read().splitlines()
  assert len(lines) == len(bits)
  values = bits.view(np.float32)
  for line, b, v in zip(lines, bits, values):
    assert line == '%08x %s' % (b, '{}'.format(v)), (hex(b), line)
  # spot checks of the rules, literally
  text = dict(line.split() for line in lines)
  assert text['3dcccccd'] == '0.10000000149011612' and text['80000000'] == '-0.0' and text['00000000'] == '0.0'
  assert text['4b800000'] == '16777216.0' and text['4ceb79a3'] == '123456792.0'
  assert text['5a0e1bca'] == '1.0000000272564224e+16' and text['5a0e1bc9'] == '9999999198822400.0'
  assert text['38d1b717'] == '9.999999747378752e-05' and text['38d1b718'] == '0.00010000000474974513'
  assert text['00000001'] == '1.401298464324817e-45' and text['7f7fffff'] == '3.4028234663852886e+38'
  assert text['ffc00000'] == 'nan' and text['7f800001'] == 'nan' and text['ff800000'] == '-inf'


def test_constants_of_the_core_and_the_library_agree():
  text = open(os.path.join(ROOT, 'se3ds_amd', 'csrc', 'ply_format_core.h')).read()
  L = _lib.lib()
  assert L.se3ds_ply_chunk_points() == int(re.search(r'constexpr int kChunkPoints = (\d+);', text).group(1))
  assert L.se3ds_ply_max_line_bytes() == 3 * (23 + 1) + 3 * (11 + 1) + 1
  assert L.se3ds_ply_max_points() == ply.MAX_SLAB_POINTS == 1 << 24
  assert ply.BINARY_RECORD.itemsize == 15 == R.RECORD.itemsize


def test_line_bound_covers_the_adversarial_set():
  bound = _lib.lib().se3ds_ply_max_line_bytes()
  values = R.adversarial_bits().view(np.float32)
  longest = max(len('{}'.format(v)) for v in values)
  line = 3 * (longest + 1) + 3 * (len(str(-2 ** 31)) + 1) + 1
  assert longest >= 22 and line <= bound
  xyz = np.repeat(values[:, None], 3, axis=1)
  rgb = np.full((len(values), 3), -2 ** 31, np.int32)
  assert max(len(l) + 1 for l in R.ascii_body(xyz, rgb).split(b'\n')[:-1]) <= bound


def test_headers_are_pinned():
  assert ply.header(5) == ('ply\nformat ascii 1.0 \nelement vertex 5\nproperty float x\nproperty float y\n'
                           'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n'
                           'end_header\n')
  assert ply.header(0, 'binary_little_endian') == (
      'ply\nformat binary_little_endian 1.0 \nelement vertex 0\nproperty float x\nproperty float y\n'
      'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
  assert ply.header(7) == R.HEADER_ASCII % 7 and ply.header(7, 'binary_little_endian') == R.HEADER_BINARY % 7
  with pytest.raises(ValueError):
    ply.header(1, 'binary_big_endian')


def _same(xyz, rgb, coords, colours):
  """bit for bit, except that a NaN comes back as some NaN"""
  want = np.asarray(coords)[0:3].T
  nan = np.isnan(want)
  assert xyz.dtype == np.float32 and rgb.dtype == np.int32 and xyz.shape == want.shape
  assert np.array_equal(np.isnan(xyz), nan)
  assert np.array_equal(xyz.view(np.uint32)[~nan], np.ascontiguousarray(want).view(np.uint32)[~nan])
  assert np.array_equal(rgb, np.asarray(colours).astype(np.int32))


@pytest.mark.parametrize('m', [0, 1, 700])
@pytest.mark.parametrize('dtype', [np.int32, np.uint8])
def test_host_encoder_and_reader_round_trip(tmp_path, m, dtype):
  coords, rgb = R.inputs(m, seed=m, colour_dtype=dtype)
  path = tmp_path / 'cloud.ply'
  ply.write_ply(path, torch.from_numpy(coords), torch.from_numpy(rgb))
  assert path.read_bytes() == R.ascii_file(coords, rgb)
  _same(*ply.read_ply(path), coords, rgb)
  # a (4, M) memory: the fourth row is ignored
  four = np.concatenate([coords, np.ones((1, m), np.float32)])
  ply.write_ply(str(path), torch.from_numpy(four), torch.from_numpy(rgb), encoder='host', format='ascii')
  assert path.read_bytes() == R.ascii_file(coords, rgb)


def test_reader_reads_the_binary_format_and_refuses_everything_else(tmp_path):
  coords, rgb = R.inputs(300, seed=3, colour_dtype=np.uint8)
  path = tmp_path / 'b.ply'
  path.write_bytes(R.binary_file(coords, rgb))
  xyz, colours = ply.read_ply(path)
  assert np.array_equal(xyz.view(np.uint32), np.ascontiguousarray(coords.T).view(np.uint32))   # NaN payloads too
  assert np.array_equal(colours, rgb.astype(np.int32)) and colours.dtype == np.int32
  good = R.ascii_file(coords[:, :2], rgb[:2])
  for bad in (b'', b'ply\n', good.replace(b'ascii 1.0 \n', b'ascii 1.0\n'), good.replace(b'uchar red', b'uchar r'),
              good.replace(b'vertex 2', b'vertex 3'), good.replace(b'vertex 2', b'vertex x'), good[:-2],
              good + b'1 2 3 4 5 6 \n', good.replace(b'format ascii', b'format binary_big_endian'),
              R.binary_file(coords, rgb)[:-1], R.binary_file(coords, rgb) + b'\0',
              good.replace(b'end_header\n', b'comment x\nend_header\n'), good[:-8] + b'a b c \n'):
    path.write_bytes(bad)
    with pytest.raises(ValueError):
      ply.read_ply(path)


def test_wrapper_checks_arguments_first(tmp_path):
  p = str(tmp_path / 'x.ply')
  c, rgb = torch.zeros((3, 5)), torch.zeros((5, 3), dtype=torch.int32)
  for kw in (dict(format='binary'), dict(format='binary_big_endian'), dict(encoder='gpu'), dict(encoder=None),
             dict(format='binary_little_endian'), dict(format='binary_little_endian', encoder='host'),
             dict(slab_points=0), dict(slab_points=(1 << 24) + 1), dict(slab_points=2.5), dict(slab_points=True)):
    with pytest.raises(ValueError):
      ply.write_ply(p, c, rgb, **kw)
  for coords, colours in ((torch.zeros((2, 5)), rgb), (torch.zeros((5, 5)), rgb), (torch.zeros((1, 3, 5)), rgb),
                          (torch.zeros((5,)), rgb), (c, torch.zeros((5, 4), dtype=torch.int32)),
                          (c, torch.zeros((4, 3), dtype=torch.int32)), (c, torch.zeros((15,), dtype=torch.int32)),
                          (c.double(), rgb), (c.half(), rgb), (c.to(torch.int32), rgb), (c, rgb.long()),
                          (c, rgb.float()), (c, rgb.to(torch.int8)), (c.numpy(), rgb), (c, rgb.numpy())):
    for encoder in ('host', 'device'):
      with pytest.raises(ValueError):
        ply.write_ply(p, coords, colours, encoder=encoder)
  # the kernels have no CPU fallback
  for format in ply.FORMATS:
    with pytest.raises(_lib.Se3dsHipError):
      ply.write_ply(p, c, rgb, format=format, encoder='device')
  assert os.listdir(tmp_path) == []


def test_model_method_signature():
  from se3ds_amd.models import models
  sig = inspect.signature(models.SE3DSModel.write_memory_as_pointcloud)
  assert list(sig.parameters) == ['self', 'filename', 'encoder', 'format']
  assert sig.parameters['encoder'].default == 'host' and sig.parameters['format'].default == 'ascii'
  sig = inspect.signature(ply.write_ply)
  assert list(sig.parameters) == ['filename', 'coords', 'rgb', 'format', 'encoder', 'slab_points']
  assert [sig.parameters[k].default for k in ('format', 'encoder', 'slab_points')] == ['ascii', 'host', 1 << 20]


def test_workspace_query():
  q = _lib.lib().se3ds_ply_ascii_workspace_bytes
  for bad in (-1, -2 ** 40, (1 << 24) + 1, 2 ** 40):
    assert q(bad) == 0, bad
  chunk = _lib.lib().se3ds_ply_chunk_points()
  last = 0
  for m in (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 1, 4097, 1 << 19, 1 << 20, (1 << 24) - 1, 1 << 24):
    b = q(m)
    assert b > 0 and b % 16 == 0 and b >= last and b >= 48 * m + 12 * ((m + chunk - 1) // chunk), m
    last = b


def test_entry_points_check_their_arguments_before_the_device():
  """Every refusal returns before the first HIP call, so it shows without a GPU: the pointers only
  have to be non-null and aligned, nothing follows them.  m = 0 is legal and launches nothing."""
  L = _lib.lib()
  mem = (ctypes.c_uint8 * 1024)()
  p = (ctypes.addressof(mem) + 15) & ~15
  big = 1 << 40

  def ascii(coords=p, stride=8, rgb=p, dtype=_lib.I32, m=8, out=p + 1, cap=big, count=p + 8, ws=p + 16, ws_bytes=big,
            phases=7):
    return L.se3ds_ply_ascii(coords, stride, rgb, dtype, m, out, cap, count, ws, ws_bytes, phases, None)

  assert ascii(dtype=_lib.F32) == BADDTYPE and ascii(dtype=_lib.BF16) == BADDTYPE and ascii(dtype=9) == BADDTYPE
  for kw in (dict(m=-1), dict(m=(1 << 24) + 1, stride=1 << 25), dict(stride=7), dict(coords=None), dict(rgb=None),
             dict(out=None), dict(count=None), dict(ws=None), dict(coords=p + 2), dict(rgb=p + 2), dict(count=p + 4),
             dict(ws=p + 8), dict(phases=0), dict(phases=8), dict(cap=8 * 109 - 1)):
    assert ascii(**kw) == BADSHAPE, kw
  assert ascii(dtype=_lib.U8, rgb=p + 1, m=0, ws_bytes=16) == 0       # uint8 colours need no alignment
  assert ascii(ws_bytes=L.se3ds_ply_ascii_workspace_bytes(8) - 1) == WORKSPACE and ascii(ws_bytes=0) == WORKSPACE
  assert ascii(m=0, stride=0, cap=0, ws_bytes=16) == 0

  def binary(coords=p, stride=8, rgb=p, dtype=_lib.I32, m=8, out=p, cap=big, flag=p + 4):
    return L.se3ds_ply_binary(coords, stride, rgb, dtype, m, out, cap, flag, None)

  assert binary(dtype=_lib.F32) == BADDTYPE
  for kw in (dict(m=-1), dict(m=(1 << 24) + 1, stride=1 << 25), dict(stride=7), dict(coords=None), dict(rgb=None),
             dict(out=None), dict(flag=None), dict(out=p + 8), dict(flag=p + 2), dict(coords=p + 1), dict(cap=8 * 15 - 1)):
    assert binary(**kw) == BADSHAPE, kw
  assert binary(m=0, stride=0, cap=0) == 0
