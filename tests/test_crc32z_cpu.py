"""The device zip / zlib CRC-32 without a GPU: the seeded kPolyZip instantiation of csrc/crc32c_core.h
as a stand-alone host program (tools/crc32z_host_check.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer over the length x alignment x seed sweep, the wrapper's table builder and
the argument checks of se3ds_crc32z_multi, which run before any HIP call.  The device runs are
tests/test_crc32z_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from se3ds_amd import _lib
from se3ds_amd.utils import crc32c as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_core_as_a_sanitised_host_program(tmp_path):
  """The same slice routine, block walk and combine order as the kernel, serially, against a bitwise
  loop written in the program (pinned there to crc32("123456789") = 0xCBF43926); every case ends at
  the end of an exact-size heap allocation.  Reports are fatal.  No sanitizer touches code loaded
  into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the CRC-32 core cannot be checked on the host'
  exe = str(tmp_path / 'crc32z_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'crc32z_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  m = re.search(r'crc32z_host_check: (\d+) cases OK', r.stdout)
  # fills x lengths x alignments x seeds x run lengths
  assert m and int(m.group(1)) >= 4 * 26 * 16 * 3 * 4
  # the checker does fail when it should: one data bit flipped behind the yardstick's back
  r = subprocess.run([exe, 'corrupt'], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected' in r.stderr


def test_constants_of_the_library():
  L = _lib.lib()
  assert L.se3ds_crc32z_fields() == 3
  assert L.se3ds_crc32z_block_bytes() == L.se3ds_crc32c_block_bytes() == 1 << 14
  assert L.se3ds_crc32z_workspace_bytes(0, 0) == 0
  for n in (1, 2, 31, 32, 1000):
    assert L.se3ds_crc32z_workspace_bytes(123, n) >= 8 * (n + 1)


def test_seeded_table_builder():
  t = C.build_table([5, 0, 7], [1, 0, 2 ** 40], [0, 0xffffffff, 9])
  assert t.dtype == np.int64 and t.shape == (3, 3) and t.flags.c_contiguous
  assert t.tolist() == [[5, 1, 0], [0, 0, 0xffffffff], [7, 2 ** 40, 9]]
  assert C.build_table([], [], []).shape == (0, 3)
  assert C.build_table([3], [4], np.array([0xfffffffe], np.uint32)).tolist() == [[3, 4, 0xfffffffe]]
  for seeds in ([1], [1, 2, 3], [0, -1], [0, 2 ** 32]):
    with pytest.raises(ValueError):
      C.build_table([1, 2], [3, 4], seeds)


def test_arguments_are_checked_before_the_device():
  """Every BADSHAPE condition returns before the first HIP call, so it shows without a GPU: the
  pointers only have to be non-null and aligned, nothing follows them."""
  L = _lib.lib()
  mem = (ctypes.c_int64 * 64)()
  p = ctypes.addressof(mem)
  ws = int(L.se3ds_crc32z_workspace_bytes(0, 2))

  def call(table, n=None, buf=p, buf_bytes=100, table_dev=p, host=True, crc=p, workspace=p, ws_bytes=ws):
    t = np.asarray(table, np.int64).reshape(-1, 3)
    return L.se3ds_crc32z_multi(buf, buf_bytes, table_dev, t.ctypes.data if host else None,
                                t.shape[0] if n is None else n, crc, workspace, ws_bytes, None)

  good = [[0, 100, 0], [99, 1, 0xffffffff]]
  assert call(good, n=0) == -1 and call(good, n=-3) == -1
  for null in ('buf', 'table_dev', 'crc', 'workspace'):
    assert call(good, **{null: None}) == -1, null
  assert call(good, host=False) == -1
  assert call([[-1, 4, 0], [0, 0, 0]]) == -1                  # negative offset
  assert call([[0, 0, 0], [4, -1, 0]]) == -1                  # negative length
  assert call([[0, 101, 0], [0, 0, 0]]) == -1                 # leaves the buffer
  assert call([[0, 0, 0], [100, 1, 0]]) == -1
  assert call([[2 ** 62, 2 ** 62, 0], [0, 0, 0]]) == -1       # no wrap-around
  assert call([[0, 2 ** 63 - 1, 0], [0, 0, 0]]) == -1
  assert call([[0, 4, 2 ** 32], [0, 0, 0]]) == -1             # a seed is 32 bits
  assert call([[0, 4, 0], [0, 0, -1]]) == -1
  assert call(good, ws_bytes=ws - 1) == -1 and call(good, ws_bytes=0) == -1
  assert call(good, buf_bytes=-1) == -1
  assert call(good, workspace=p + 4) == -1 and call(good, table_dev=p + 4) == -1   # misaligned


def test_no_host_fallback():
  import torch
  with pytest.raises(_lib.Se3dsHipError):
    C.crc32z_device(torch.zeros((4,), dtype=torch.uint8), [0], [4])
