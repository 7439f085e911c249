"""The device CRC-32C without a GPU: csrc/crc32c_core.h as a stand-alone host program
(tools/crc32c_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer over the length x
alignment sweep, the wrapper's pure host parts (table builder, slab packer) and the argument checks
of se3ds_crc32c_multi, which run before any HIP call.  The device runs are tests/test_crc32c_gpu.py."""
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
CORE = os.path.join(ROOT, 'se3ds_amd', 'csrc', 'crc32c_core.h')


def test_core_as_a_sanitised_host_program(tmp_path):
  """The same slice routine, block walk and combine order as the kernel, serially, against a bitwise
  loop written in the program; every case ends at the end of an exact-size heap allocation.  Reports
  are fatal.  No sanitizer touches code loaded into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the CRC-32C core cannot be checked on the host'
  exe = str(tmp_path / 'crc32c_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'crc32c_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  m = re.search(r'crc32c_host_check: (\d+) cases OK', r.stdout)
  assert m and int(m.group(1)) >= 4 * 26 * 16 * 4   # fills x lengths x alignments x run lengths
  # the checker does fail when it should: one data bit flipped behind the yardstick's back
  r = subprocess.run([exe, 'corrupt'], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected' in r.stderr


def test_constants_of_the_core_and_the_library_agree():
  text = open(CORE).read()
  shift = int(re.search(r'constexpr int kBlockShift = (\d+);', text).group(1))
  L = _lib.lib()
  assert L.se3ds_crc32c_block_bytes() == 1 << shift <= 1 << 20
  assert L.se3ds_crc32c_fields() == 2
  assert L.se3ds_crc32c_workspace_bytes(0, 0) == 0
  for n in (1, 2, 31, 32, 1000):
    assert L.se3ds_crc32c_workspace_bytes(123, n) >= 8 * (n + 1)


def test_table_builder():
  t = C.build_table([5, 0, 7], [1, 0, 2 ** 40])
  assert t.dtype == np.int64 and t.shape == (3, 2) and t.flags.c_contiguous
  assert t.tolist() == [[5, 1], [0, 0], [7, 2 ** 40]]
  assert C.build_table([], []).shape == (0, 2)
  assert C.build_table(np.array([3], np.uint8), np.array([4], np.int32)).tolist() == [[3, 4]]
  with pytest.raises(ValueError):
    C.build_table([1, 2], [3])


def _check_plan(sizes, slab_bytes):
  plan = C.pack_slabs(sizes, slab_bytes)
  order = [i for idx, _, _ in plan for i in idx]
  assert order == list(range(len(sizes)))                       # input order, every item once
  for idx, offs, used in plan:
    assert len(idx) == len(offs) >= 1
    end = 0
    for i, o in zip(idx, offs):
      assert o % C.SLAB_ALIGN == 0 and o >= end and o + sizes[i] <= used   # inside, no overlap
      end = o + sizes[i]
    assert end == used
    assert used <= slab_bytes or len(idx) == 1                  # only an oversized item exceeds it
  return plan


def test_slab_packer():
  assert C.pack_slabs([], 100) == []
  plan = _check_plan([10, 20, 30], 1000)
  assert plan == [([0, 1, 2], [0, 16, 48], 78)]
  plan = _check_plan([10, 500, 7, 3, 90, 90], 100)
  assert [idx for idx, _, _ in plan] == [[0], [1], [2, 3], [4], [5]]   # 500 > 100: a slab of its own
  assert plan[1] == ([1], [0], 500)
  plan = _check_plan([0, 0, 5, 0], 16)
  assert plan == [([0, 1, 2, 3], [0, 0, 0, 16], 16)]
  assert _check_plan([100], 100) == [([0], [0], 100)]
  assert [idx for idx, _, _ in _check_plan([100, 1], 100)] == [[0], [1]]   # padding counts
  rng = np.random.default_rng(0)
  for _ in range(50):
    sizes = rng.integers(0, 300, rng.integers(1, 40)).tolist()
    _check_plan(sizes, int(rng.integers(1, 400)))
  with pytest.raises(ValueError):
    C.pack_slabs([1], 0)


def test_items_are_taken_as_their_bytes():
  assert C._as_bytes(b'abc').tolist() == [97, 98, 99]
  assert C._as_bytes(np.array([True, False])).tolist() == [1, 0]
  assert C._as_bytes(np.array(1, '<u2')).tolist() == [1, 0]
  assert C._as_bytes(np.arange(6, dtype='<i4').reshape(2, 3)[:, 1]).size == 8   # made contiguous


def test_arguments_are_checked_before_the_device():
  """Every BADSHAPE condition returns before the first HIP call, so it shows without a GPU: the
  pointers only have to be non-null and aligned, nothing follows them."""
  L = _lib.lib()
  mem = (ctypes.c_int64 * 64)()
  p = ctypes.addressof(mem)
  ws = int(L.se3ds_crc32c_workspace_bytes(0, 2))

  def call(table, n=None, buf=p, buf_bytes=100, table_dev=p, host=True, crc=p, workspace=p, ws_bytes=ws):
    t = np.asarray(table, np.int64).reshape(-1, 2)
    return L.se3ds_crc32c_multi(buf, buf_bytes, table_dev, t.ctypes.data if host else None,
                                t.shape[0] if n is None else n, crc, workspace, ws_bytes, None)

  good = [[0, 100], [99, 1]]
  assert call(good, n=0) == -1 and call(good, n=-3) == -1
  for null in ('buf', 'table_dev', 'crc', 'workspace'):
    assert call(good, **{null: None}) == -1, null
  assert call(good, host=False) == -1
  assert call([[-1, 4], [0, 0]]) == -1                     # negative offset
  assert call([[0, 0], [4, -1]]) == -1                     # negative length
  assert call([[0, 101], [0, 0]]) == -1                    # leaves the buffer
  assert call([[0, 0], [100, 1]]) == -1
  assert call([[2 ** 62, 2 ** 62], [0, 0]]) == -1          # no wrap-around
  assert call([[0, 2 ** 63 - 1], [0, 0]]) == -1
  assert call(good, ws_bytes=ws - 1) == -1 and call(good, ws_bytes=0) == -1
  assert call(good, buf_bytes=-1) == -1
  assert call(good, workspace=p + 4) == -1 and call(good, table_dev=p + 4) == -1   # misaligned


def test_no_host_fallback():
  import torch
  with pytest.raises(_lib.Se3dsHipError):
    C.crc32c_device(torch.zeros((4,), dtype=torch.uint8), [0], [4])
  with pytest.raises(_lib.Se3dsHipError):
    C.crc32c_host_slabs([b'abc'], device='cpu')
  from se3ds_amd.utils import tf_bundle, tf_records
  with pytest.raises(ValueError, match='verify'):
    list(tf_records.read_records('nowhere', verify='gpu'))
  with pytest.raises(ValueError, match='verify'):
    tf_bundle.read_bundle('nowhere', verify='gpu')
  with pytest.raises(ValueError, match='checksums'):
    tf_bundle.write_bundle('nowhere', {}, checksums='gpu')
