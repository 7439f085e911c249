"""The Frechet distance of two FeatureMoments at dim 2048: the host path (download + NumPy + SciPy
sqrtm, FeatureMoments.fid(method='host')) against the device path (csrc/frechet.hip,
fid(method='device')) with and without the cached root of the first set, at 500, 5000 and 10000
rows per set.  Also one se3ds_f64_gemm at the same size as TFLOP/s (2 n^3 per product) and the
share of the device path that is not GEMM time.  Inputs: the seeded generator of the tests.

Timing: a warm-up call, then device events around whole calls (a device call ends with its one host
read, so the events cover it), median of --repeats; the host path on the wall clock.

  python tools/frechet_bench.py [--dim 2048] [--rows 500 5000 10000] [--repeats 5] [--host-repeats 1]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import _frechet_ref as ref  # noqa: E402
from se3ds_amd.utils import inception_utils as iu  # noqa: E402

DEV = torch.device('cuda:0')


def event_ms(fn, repeats):
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
  return statistics.median(times)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--dim', type=int, default=iu.POOL_DIM)
  ap.add_argument('--rows', type=int, nargs='+', default=[500, 5000, 10000])
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--host-repeats', type=int, default=1)
  a = ap.parse_args()
  n = a.dim
  print(f'dim {n}, host CPUs {len(os.sched_getaffinity(0))}, torch threads {torch.get_num_threads()}')

  x = torch.randn((n, n), dtype=torch.float64, device=DEV)
  y = torch.randn((n, n), dtype=torch.float64, device=DEV)
  out = torch.empty_like(x)

  def gemms():
    for _ in range(10):
      iu.f64_gemm(x, y, out=out)

  gemm_ms = event_ms(gemms, a.repeats) / 10
  print(f'se3ds_f64_gemm n = {n}: {gemm_ms:.3f} ms  {2 * n ** 3 / gemm_ms / 1e9:.2f} TFLOP/s')

  for rows in a.rows:
    fa = iu.FeatureMoments(dim=n, device=DEV).update(torch.from_numpy(ref.features(rows, n, 31)).to(DEV))
    fb = iu.FeatureMoments(dim=n, device=DEV).update(torch.from_numpy(ref.features(rows, n, 32)).to(DEV))
    host_s = []
    for _ in range(a.host_repeats):
      t0 = time.perf_counter()
      want = fa.fid(fb)
      host_s.append(time.perf_counter() - t0)
    host_ms = statistics.median(host_s) * 1e3

    def uncached():
      fa._root = None
      return fa.fid(fb, method='device')

    cold_ms = event_ms(uncached, a.repeats)
    got = fa.fid(fb, method='device')
    k1 = fa._root[3]
    mu2, s2 = fb.mean_cov_device()
    r = iu.frechet_distance_device(fa._root[0], fa._root[1], mu2, s2, root1=fa._root[2])
    k2 = r.iterations[1]
    warm_ms = event_ms(lambda: fa.fid(fb, method='device'), a.repeats)
    mu1, s1 = fa.mean_cov()
    mu2h, s2h = fb.mean_cov()
    s = ref.scale(mu1, s1, mu2h, s2h)
    cold_gemm, warm_gemm = (3 * (k1 + k2) + 2) * gemm_ms, (3 * k2 + 2) * gemm_ms
    print(f'rows {rows}: host {host_ms:.0f} ms | device, root computed {cold_ms:.1f} ms '
          f'({host_ms / cold_ms:.0f}x), root cached {warm_ms:.1f} ms ({host_ms / warm_ms:.0f}x) | '
          f'iterations {k1} + {k2} | not GEMM: {100 * (1 - cold_gemm / cold_ms):.0f} % / '
          f'{100 * (1 - warm_gemm / warm_ms):.0f} % | converged {r.converged} | '
          f'|device - host| / s = {abs(got - want) / s:.2g}')


if __name__ == '__main__':
  main()
