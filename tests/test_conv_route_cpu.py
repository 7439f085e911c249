"""The routing of the convolution family without a GPU: csrc/conv_route.h as a stand-alone host
program (tools/conv_route_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, and
what the four host-only queries of the built library answer against the integers recorded before the
routing moved into that header (tests/golden/conv_route_queries.json).  The device runs are
tests/test_conv_lattice_gpu.py (every route by name, bit for bit) and tests/test_nets_gpu.py (the
switches)."""
import itertools
import json
import os
import re
import shutil
import subprocess

from se3ds_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE = (0, 3)
K = (1, 2, 3, 4, 7)
STRIDES = (1, 2)
CIN = (3, 4, 8, 16, 32, 64, 96, 128, 192, 256, 512, 1024, 2048)
COUT = (1, 3, 4, 8, 64, 128, 192, 256, 512, 1024, 2048)
HW = ((8, 16), (32, 64), (33, 65), (129, 257), (512, 1024))
N = (1, 8, 16)
SWITCHES = ('SE3DS_NO_THIN', 'SE3DS_HALO_TILE', 'SE3DS_BIG_TILE', 'SE3DS_FUSED_BN_STATS', 'SE3DS_HALO_M16')


def test_routing_as_a_sanitised_host_program(tmp_path):
  """conv_route, the two statistics-row queries, wgrad_route, wgrad_swapped_route and the two workspace
  sizes against a transcription of the dispatchers conv.hip held before, over the whole sweep; every
  route a dispatcher can choose is met; the production shapes keep their routes; reports are fatal.
  No sanitizer touches code loaded into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the routing cannot be checked on the host'
  exe = str(tmp_path / 'conv_route_host_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                      '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 'conv_route_host_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  m = re.search(r'conv_route_host_check: (\d+) cases OK', r.stdout)
  assert m and int(m.group(1)) == 10772190
  # the checker does fail when it should: a yardstick that asks the macro tile before the halo kernel
  r = subprocess.run([exe, 'corrupt'], capture_output=True, text=True)
  assert r.returncode == 1 and 'expected' in r.stderr


def test_the_four_host_queries_did_not_move(monkeypatch):
  """se3ds_conv2d_fwd_stats_rows, se3ds_conv2d_dgrad_bnstats_rows, se3ds_conv2d_wgrad_workspace_bytes
  and se3ds_conv2d_wgrad_swapped_workspace_bytes of the built library on 95 shapes of the sweep, under
  the default environment and under seven settings of the switches (read per call), against the
  integers tests/golden/make_conv_route_queries.py recorded."""
  data = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_route_queries.json')))
  full = [(d, k, s, ci, co, h, w, n)
          for d, k, s, ci, co, (h, w), n in itertools.product(DTYPE, K, STRIDES, CIN, COUT, HW, N)]
  cases = full[::701] + [c for c in full if c[:3] == (3, 3, 1)][::67]
  assert [tuple(c) for c in data['cases']] == cases and len(cases) == 95
  assert len(data['recorded']) == 8 and data['recorded'][0]['env'] == {}
  L = _lib.lib()
  for rec in data['recorded']:
    for name in SWITCHES:
      monkeypatch.delenv(name, raising=False)
    for name, value in rec['env'].items():
      monkeypatch.setenv(name, value)
    assert len(rec['answers']) == len(cases)
    for i, ((d, k, s, ci, co, h, w, n), want) in enumerate(zip(cases, rec['answers'])):
      got = [L.se3ds_conv2d_fwd_stats_rows(d, n, ci, h, w, co, k, k, s, int(i % 3 != 0), int(i % 3 == 1)),
             L.se3ds_conv2d_dgrad_bnstats_rows(d, n, h, w, ci, co, k, k, s, int(i % 5 == 4)),
             L.se3ds_conv2d_wgrad_workspace_bytes(n, h, w, ci, co, k, k),
             L.se3ds_conv2d_wgrad_swapped_workspace_bytes(n, h, w, ci, co, k)]
      assert got == want, (rec['env'], cases[i])
