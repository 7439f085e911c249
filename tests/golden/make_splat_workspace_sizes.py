"""Writes tests/golden/splat_workspace_sizes.json: what se3ds_splat_workspace_bytes of the built library
returns for every 17th case of the sweep of tools/splat_layout_host_check.cpp (56 of 945), so that
tests/test_splat_layout_cpu.py can pin the sizes a later build reports.  The query is host-only (no
GPU).  Recorded from the build that still summed the sizes by hand, before csrc/splat_layout.h.  Run
from the repository root after building the library:

  python tests/golden/make_splat_workspace_sizes.py
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = (1, 2, 8)
M = (0, 1, 3, 50, 4099, 8192, 70001, 4194304, 33554432)
HEIGHT = (8, 48, 256, 512, 1024)   # width = 2 * height
CHANNELS = (1, 2, 3, 5, 7, 9, 60)
STRIDE = 17


def sweep():
  """(n, m, height, width, channels) in the order of the host check's loops."""
  return [(n, m, h, 2 * h, c) for n, m, h, c in itertools.product(N, M, HEIGHT, CHANNELS)]


def main():
  from se3ds_amd import _lib
  query = _lib.lib().se3ds_splat_workspace_bytes
  rows = [list(case) + [query(*case)] for case in sweep()[::STRIDE]]
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'splat_workspace_sizes.json')
  with open(path, 'w') as f:
    f.write('[\n' + ',\n'.join('  ' + json.dumps(r) for r in rows) + '\n]\n')
  print(path, len(rows), 'cases')


if __name__ == '__main__':
  main()
