"""SSIM on the device: (a) utils/image_metrics.ssim, one fused launch plus a small reduce, against
(b) the same value made op by op in torch: the inputs widened to float64, the four window sums as
depthwise conv2d passes (1 x 11, then 11 x 1), the index arithmetic and the means as elementwise ops
and reductions, each writing its plane to HBM.  8 x 512 x 1024 x 3 fp32, the default window.

(a) and (b) are compared before anything is timed: they round in different orders, so the check is
|a - b| <= 1e-10 on the per-image values.  Timing: device events after warm-up, (b), (a), (b)
alternating in one process; the two (b) legs of a round against each other give the run-to-run
spread the ratio has to be read against.  The library's two launches are also timed alone, on
preallocated outputs, to show what the wrapper adds.  Bytes are computed from the shapes: what each form has to
read and write if every operator touched its operands exactly once.

  python tools/image_metrics_bench.py [--rounds 5] [--iters 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.utils import image_metrics  # noqa: E402

DEV = torch.device('cuda:0')
HBM_ACHIEVABLE = 6.3e12   # bytes / s
N, H, W, C, FS = 8, 512, 1024, 3, 11


def op_by_op(a, b, taps64, max_val=1.0, k1=0.01, k2=0.03):
  """(N,) float64 SSIM from float64 torch operators; a, b (N, H, W, C) fp32."""
  c = a.shape[3]
  x = a.permute(0, 3, 1, 2).to(torch.float64)
  y = b.permute(0, 3, 1, 2).to(torch.float64)
  row = taps64.reshape(1, 1, 1, -1).repeat(c, 1, 1, 1)
  col = taps64.reshape(1, 1, -1, 1).repeat(c, 1, 1, 1)
  window = lambda z: F.conv2d(F.conv2d(z, row, groups=c), col, groups=c)
  c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
  m0, m1 = window(x), window(y)
  n0 = 2.0 * m0 * m1
  d0 = m0 * m0 + m1 * m1
  lum = (n0 + c1) / (d0 + c1)
  n1 = 2.0 * window(x * y)
  d1 = window(x * x + y * y)
  cs = (n1 - n0 + c2) / (d1 - d0 + c2)
  return (lum * cs).mean(dim=(2, 3)).mean(dim=1)


def bytes_moved(n, h, w, c, fs):
  """(fused, op by op).  fused: a and b once as fp32, the workgroups' records written and read once, the
  means.  op by op: 8 bytes per element and operand of every operator of the chain above."""
  full, rows, out = n * h * w * c, n * h * (w - fs + 1) * c, n * (h - fs + 1) * (w - fs + 1) * c
  L = _lib.lib()
  fused = 2 * full * 4 + 2 * L.se3ds_ssim_workspace_bytes(n, h, w, c, fs) + 2 * n * c * 8
  chain = 2 * (full * 4 + full * 8)                 # widen a and b
  chain += 3 * full * 8                             # x * y
  chain += 3 * 3 * full * 8                         # x * x, y * y, their sum
  chain += 4 * ((full + rows) * 8 + (rows + out) * 8)   # four windows: row pass, column pass
  # 2 m0 m1 (2 ops), m0 m0, m1 m1, +, n0 + c1, d0 + c1, /, 2 w, n1 - n0, + c2, d1 - d0, + c2, /, lum cs
  binary, unary = 9, 6
  chain += (3 * binary + 2 * unary) * out * 8
  chain += out * 8                                  # the mean reads the map
  return int(fused), int(chain)


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
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  g = torch.Generator(device=DEV).manual_seed(1)
  a = torch.rand((N, H, W, C), device=DEV, generator=g)
  b = (a + 0.1 * (torch.rand((N, H, W, C), device=DEV, generator=g) - 0.5)).clamp_(0.0, 1.0)
  taps64 = torch.from_numpy(image_metrics.gaussian_taps(FS, 1.5).astype(np.float64)).to(DEV)
  fa = lambda: image_metrics.ssim(a, b, 1.0)
  fb = lambda: op_by_op(a, b, taps64)
  got, want = fa(), fb()
  gap = float((got - want).abs().max())
  assert gap <= 1e-10, gap
  del got, want
  for _ in range(3):   # warm-up of both legs
    fa()
    fb()
  torch.cuda.synchronize()
  ta, tb1, tb2 = [], [], []
  for _ in range(args.rounds):
    tb1.append(time_ms(fb, args.iters))
    ta.append(time_ms(fa, args.iters))
    tb2.append(time_ms(fb, args.iters))
  # the two launches alone, on preallocated outputs: what the wrapper's allocations and the channel
  # mean add to them shows as fused_ms - launches_ms
  L = _lib.lib()
  taps = image_metrics.gaussian_taps(FS, 1.5)
  means = torch.empty((2, N, C), dtype=torch.float64, device=DEV)
  ws = torch.empty((L.se3ds_ssim_workspace_bytes(N, H, W, C, FS),), dtype=torch.uint8, device=DEV)
  def launches():
    _lib.check(L.se3ds_ssim(a.data_ptr(), b.data_ptr(), _lib.F32, N, H, W, C, taps.ctypes.data, FS, 1.0, 0.01,
                            0.03, means[0].data_ptr(), means[1].data_ptr(), None, ws.data_ptr(), ws.numel(),
                            _lib.stream()), 'ssim')
  launches()
  assert float((means[0].mean(dim=1) - fa()).abs().max()) == 0.0
  ms_launches = float(np.median([time_ms(launches, args.iters) for _ in range(args.rounds)]))
  ms_a, ms_b = float(np.median(ta)), float(np.median(tb1 + tb2))
  spread = float(max(abs(x - y) / min(x, y) for x, y in zip(tb1, tb2)))
  fused_bytes, chain_bytes = bytes_moved(N, H, W, C, FS)
  doc = dict(tool='tools/image_metrics_bench.py', rounds=args.rounds, iters=args.iters,
             device=torch.cuda.get_device_name(0), shape=[N, H, W, C], filter_size=FS, dtype='float32',
             tile=[L.se3ds_ssim_tile_rows(), L.se3ds_ssim_tile_cols()], max_abs_gap=gap,
             fused_ms=ms_a, fused_launches_ms=ms_launches, op_by_op_ms=ms_b, fused_over_op_by_op=ms_a / ms_b, op_by_op_self_spread=spread,
             fused_bytes=fused_bytes, op_by_op_bytes=chain_bytes, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE,
             fused_share_of_hbm=fused_bytes / (ms_a * 1e-3) / HBM_ACHIEVABLE,
             op_by_op_share_of_hbm=chain_bytes / (ms_b * 1e-3) / HBM_ACHIEVABLE,
             fused_ms_rounds=ta, op_by_op_ms_rounds=tb1 + tb2)
  print(f'ssim {N}x{H}x{W}x{C} fp32: fused {ms_a:7.3f} ms (its two launches alone {ms_launches:7.3f} ms; '
        f'{fused_bytes / 1e6:7.1f} MB, '
        f'{100 * doc["fused_share_of_hbm"]:4.1f} % of 6.3 TB/s)  op by op {ms_b:7.3f} ms ({chain_bytes / 1e6:7.1f} MB)  '
        f'fused / op-by-op {ms_a / ms_b:5.3f}  op-by-op against itself +-{100 * spread:4.1f} %  '
        f'|fused - op-by-op| {gap:.2e}', flush=True)
  print(json.dumps(doc))
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(doc, f, indent=1)


if __name__ == '__main__':
  main()
