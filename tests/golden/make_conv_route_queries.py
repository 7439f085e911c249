"""Writes tests/golden/conv_route_queries.json: what the four host-only queries of the convolution
family -- se3ds_conv2d_fwd_stats_rows, se3ds_conv2d_dgrad_bnstats_rows,
se3ds_conv2d_wgrad_workspace_bytes, se3ds_conv2d_wgrad_swapped_workspace_bytes -- return for every
701st shape of the sweep of tools/conv_route_host_check.cpp (62 of 42 900) and, because few of those
meet the halo and macro-tile kernels, for every 67th of its bf16 3x3 stride-1 shapes (33 of 2 145),
under the default environment and under each routing switch, so that
tests/test_conv_route_cpu.py can pin what a later build answers.  No GPU.  Recorded from the build that still decided the route in conv.hip's
dispatchers, before csrc/conv_route.h.  The switches are read per call, but every environment gets a
process of its own all the same: nothing one of them leaves behind reaches the next.  Run from the
repository root after building the library:

  python tests/golden/make_conv_route_queries.py
"""
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DTYPE = (0, 3)   # SE3DS_F32, SE3DS_BF16
K = (1, 2, 3, 4, 7)
STRIDES = (1, 2)
CIN = (3, 4, 8, 16, 32, 64, 96, 128, 192, 256, 512, 1024, 2048)
COUT = (1, 3, 4, 8, 64, 128, 192, 256, 512, 1024, 2048)
HW = ((8, 16), (32, 64), (33, 65), (129, 257), (512, 1024))
N = (1, 8, 16)
STRIDE, STRIDE_3X3 = 701, 67
ENVS = ({}, {'SE3DS_NO_THIN': '1'}, {'SE3DS_HALO_TILE': '0'}, {'SE3DS_HALO_TILE': '128'},
        {'SE3DS_BIG_TILE': '0'}, {'SE3DS_BIG_TILE': '1'}, {'SE3DS_FUSED_BN_STATS': '0'},
        {'SE3DS_FUSED_BN_STATS': '1'})
SWITCHES = sorted({k for e in ENVS for k in e} | {'SE3DS_HALO_M16'})


def sweep():
  """(dtype, k, stride, cin, cout, h, w, n): every 701st of the product, then every 67th of its bf16
  3x3 stride-1 part."""
  full = [(d, k, s, ci, co, h, w, n)
          for d, k, s, ci, co, (h, w), n in itertools.product(DTYPE, K, STRIDES, CIN, COUT, HW, N)]
  return full[::STRIDE] + [c for c in full if c[:3] == (3, 3, 1)][::STRIDE_3X3]


def answers(lib, cases):
  """Per case [fwd_stats_rows, dgrad_bnstats_rows, wgrad_workspace_bytes, wgrad_swapped_workspace_bytes];
  the mask and the row scale of the two statistics queries go by the case's position."""
  rows = []
  for i, (d, k, s, ci, co, h, w, n) in enumerate(cases):
    has_mask, binary = i % 3 != 0, i % 3 == 1
    rows.append([lib.se3ds_conv2d_fwd_stats_rows(d, n, ci, h, w, co, k, k, s, int(has_mask), int(binary)),
                 lib.se3ds_conv2d_dgrad_bnstats_rows(d, n, h, w, ci, co, k, k, s, int(i % 5 == 4)),
                 lib.se3ds_conv2d_wgrad_workspace_bytes(n, h, w, ci, co, k, k),
                 lib.se3ds_conv2d_wgrad_swapped_workspace_bytes(n, h, w, ci, co, k)])
  return rows


def main():
  if '--child' in sys.argv:
    from se3ds_amd import _lib
    print(json.dumps(answers(_lib.lib(), sweep())))
    return
  recorded = []
  for env in ENVS:
    child = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    child.update(env)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=child, check=True,
                         capture_output=True, text=True).stdout
    recorded.append({'env': env, 'answers': json.loads(out.strip().splitlines()[-1])})
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_route_queries.json')
  with open(path, 'w') as f:
    f.write('{"cases": ' + json.dumps([list(c) for c in sweep()]) + ',\n "recorded": [\n' +
            ',\n'.join('  ' + json.dumps(r) for r in recorded) + '\n]}\n')
  print(path, len(sweep()), 'cases x', len(ENVS), 'environments')


if __name__ == '__main__':
  main()
