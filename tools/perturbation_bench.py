"""The collision screen of the VLN perturbation augmentation on the device: (a) one
se3ds_collision_count launch for all candidates against (b) the same counts made op by op with
torch, one candidate at a time as the reference does it on the host (slice, multiply, compare,
sum), at K = 64 candidates on one 512x1024 depth panorama and at N = 8 panoramas x 64 candidates.

Both legs start from what a caller has: the depth on the device, and the window table and the
thresholds on the device (their one host-to-device copy is outside the timed window of both).
(a) == (b) is checked on the counts before anything is timed.  Timing: device events after
warm-up, (b), (a), (b) alternating in one process; the two (b) legs of a round against each other
give the run-to-run spread the (a) / (b) ratio has to be read against.  Bytes are the window
pixels x 4, each counted once per candidate that reads it (the panoramas themselves are 2 MiB
each and stay in the L2 / Infinity Cache: this is not an HBM figure).

  python tools/perturbation_bench.py [--rounds 5] [--iters 20] [--kernel-iters 2000] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from se3ds_amd import _lib  # noqa: E402
from se3ds_amd import constants  # noqa: E402
from se3ds_amd.inference import perturbation_utils as pu  # noqa: E402

DEV = torch.device('cuda:0')
F32 = np.float32


def time_ms(fn, iters):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=20, help='op-by-op passes per timed window')
  ap.add_argument('--kernel-iters', type=int, default=2000,
                  help='kernel launches per timed window (tens of microseconds each)')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('perturbation_bench needs an MI355X: a CPU run cannot give a time')
  h, w, per_image = 512, 1024, 64
  results = []
  for n in (1, 8):
    k = n * per_image
    g = torch.Generator(device=DEV).manual_seed(n)
    depth = torch.rand((n, h, w), device=DEV, generator=g) * 0.15   # 0 ... 3 m
    offsets = pu.draw_candidates(np.random.default_rng(n), k)
    index = np.repeat(np.arange(n, dtype=np.int32), per_image)
    windows, distance = pu.collision_windows(offsets, h, w)
    threshold = distance + F32(0.1)
    d_win = torch.from_numpy(windows).to(DEV)
    d_idx = torch.from_numpy(index).to(DEV)
    d_thr = torch.from_numpy(threshold).to(DEV)
    count = torch.empty((k,), dtype=torch.int32, device=DEV)
    L = _lib.lib()
    scale = float(constants.DEPTH_SCALE)
    rows = [tuple(int(v) for v in r) for r in windows]
    thr_rows = [d_thr[c] for c in range(k)]   # 0-d device tensors: no host value enters (b)'s compare

    def fa():
      _lib.check(L.se3ds_collision_count(depth.data_ptr(), n, h, w, d_win.data_ptr(), d_idx.data_ptr(),
                                         d_thr.data_ptr(), scale, k, count.data_ptr(), _lib.stream()),
                 'se3ds_collision_count')
      return count

    def fb():
      out = []
      for c, (r0, r1, c0, c1) in enumerate(rows):
        region = depth[int(index[c]), r0:r1, c0:c1]
        out.append(((region * scale) < thr_rows[c]).sum())
      return torch.stack(out)

    got, want = fa().cpu().numpy(), fb().cpu().numpy()
    assert np.array_equal(got, want.astype(np.int32)), (n, got[:8], want[:8])
    # ... and the public function (one table copy + launch + division) gives the same counts
    pub = pu.get_proportion_invalid_batch(offsets, depth, index).count.cpu().numpy()
    assert np.array_equal(pub, got)
    for _ in range(3):   # warm-up of both legs
      fa()
      fb()
    torch.cuda.synchronize()
    ta, tb1, tb2 = [], [], []
    for _ in range(a.rounds):
      tb1.append(time_ms(fb, a.iters))
      ta.append(time_ms(fa, a.kernel_iters))
      tb2.append(time_ms(fb, a.iters))
    ms_a = float(np.median(ta))
    ms_b = float(np.median(tb1 + tb2))
    # (b) against itself: the largest relative gap between the two (b) legs of one round
    spread = float(max(abs(x - y) / min(x, y) for x, y in zip(tb1, tb2)))
    window_bytes = int(((windows[:, 1] - windows[:, 0]).astype(np.int64) *
                        (windows[:, 3] - windows[:, 2])).sum()) * 4
    r = dict(panoramas=n, candidates=k, size=[h, w], kernel_ms=ms_a, op_by_op_ms=ms_b,
             kernel_over_op_by_op=ms_a / ms_b, op_by_op_self_spread=spread,
             window_bytes=window_bytes, kernel_window_bytes_per_s=window_bytes / (ms_a * 1e-3),
             launches_kernel=2, launches_op_by_op=3 * k + 1,
             kernel_ms_rounds=ta, op_by_op_ms_rounds=tb1 + tb2)
    results.append(r)
    print(f'{n} x {per_image} candidates on {h}x{w}: kernel {ms_a * 1e3:8.1f} us '
          f'({window_bytes / 1e6:6.1f} MB of window pixels, {r["kernel_window_bytes_per_s"] / 1e12:5.2f} TB/s '
          f'from cache)  op by op {ms_b * 1e3:9.1f} us  kernel / op-by-op {ms_a / ms_b:6.4f}  '
          f'op-by-op against itself +-{100 * spread:4.1f} %', flush=True)
  doc = dict(tool='tools/perturbation_bench.py', rounds=a.rounds, iters=a.iters, kernel_iters=a.kernel_iters,
             device=torch.cuda.get_device_name(0), results=results)
  print(json.dumps(doc))
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(doc, f, indent=1)


if __name__ == '__main__':
  main()
