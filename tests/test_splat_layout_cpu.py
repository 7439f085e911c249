"""The host arithmetic of the warp's splat without a GPU: csrc/splat_layout.h as a stand-alone host
program (tools/splat_layout_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, and
the sizes the built library reports against values recorded before the layouts moved into that header
(tests/golden/splat_workspace_sizes.json).  The device runs are tests/test_warp_gpu.py."""
import json
import os
import re
import shutil
import subprocess

from se3ds_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (1, 2, 8)
M = (0, 1, 3, 50, 4099, 8192, 70001, 4194304, 33554432)
HEIGHT_WIDTH = ((8, 16), (48, 96), (256, 512), (512, 1024), (1024, 2048))
CHANNELS = (1, 2, 3, 5, 7, 9, 60)


def test_layout_as_a_sanitised_host_program(tmp_path):
  """Every workspace carved from a heap block of exactly the reported size, sizes and offsets against
  the sums and chains geom.hip held before, the chunk geometry against the two functions it
  replaced, the route against the pinned table; reports are fatal.  No sanitizer touches code loaded
  into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the splat layout cannot be checked on the host'
  exe = str(tmp_path / 'splat_layout_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'splat_layout_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  m = re.search(r'splat_layout_host_check: (\d+) cases OK', r.stdout)
  assert m and int(m.group(1)) == len(N) * len(M) * len(HEIGHT_WIDTH) * len(CHANNELS) == 945
  # the checker does fail when it should: walks that count fewer resolve items than the yardstick
  r = subprocess.run([exe, 'corrupt'], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected' in r.stderr


def test_reported_workspace_sizes_did_not_move():
  """se3ds_splat_workspace_bytes of the built library (a host-only query) on 56 cases of the sweep,
  against the integers tests/golden/make_splat_workspace_sizes.py recorded."""
  rows = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'splat_workspace_sizes.json')))
  sweep = [(n, m, h, w, c) for n in N for m in M for h, w in HEIGHT_WIDTH for c in CHANNELS]
  assert [tuple(r[:5]) for r in rows] == sweep[::17] and len(rows) == 56
  query = _lib.lib().se3ds_splat_workspace_bytes
  for n, m, h, w, c, want in rows:
    assert query(n, m, h, w, c) == want, (n, m, h, w, c)
