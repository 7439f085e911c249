"""The evaluation input transform on the device: (a) R2RVideoDataset.device_transform, one
se3ds_video_transform launch, against (b) the same outputs made op by op from the operators that
were there before it (pano_utils.resize per field, a torch multiply for the band mask), at
1024x2048 -> 512x1024 and -> 128x256, T = 8, batch 1 and 4, mask ratio 0 and 0.25.

(a) == (b) is checked bit for bit before anything is timed.  Timing: device events after warm-up,
(b), (a), (b) alternating in one process; the two (b) legs of a round against each other give the
run-to-run spread the (a) / (b) ratio has to be read against.  Bytes are computed from the shapes
(distinct source taps + outputs), and bytes / ms is set against the achievable HBM rate.

  python tools/video_input_bench.py [--rounds 5] [--iters 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from se3ds_amd.datasets import indoor_datasets  # noqa: E402
from se3ds_amd.utils import pano_utils  # noqa: E402

DEV = torch.device('cuda:0')
HBM_ACHIEVABLE = 6.3e12   # bytes / s
PLANES = dict(segmentation=1, pathdreamer_segmentation=1, depth=4, pathdreamer_depth=4)


def op_by_op(raw, params, size):
  n, t, h0, w0, _ = raw['image'].shape
  h, w = size, 2 * size
  out = {}
  out['original_image'] = pano_utils.resize(raw['image'].reshape(n * t, h0, w0, 3), h, w,
                                            'bilinear').reshape(n, t, h, w, 3)
  out['image'] = out['original_image']
  if any(p['hmask'] is not None for p in params):
    x = torch.arange(w, dtype=torch.float32, device=DEV)
    rows = []
    for p in params:
      mode, start, end = p['hmask']
      rows.append(((x > start) | (x < end)) if mode == 2 else ((x > start) & (x < end)))
    mask = torch.stack(rows).to(torch.float32)
    out['image'] = out['original_image'] * mask[:, None, None, :, None]
  for k in PLANES:
    out[k] = pano_utils.resize(raw[k][..., None].contiguous().reshape(n * t, h0, w0, 1), h, w,
                               'nearest').reshape(n, t, h, w, 1)
  return out


def taps(out, src):
  """Distinct source indices the bilinear taps of `out` outputs touch along an axis of `src`."""
  scale = np.float32(src) / np.float32(out)
  pos = (np.arange(out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
  lo = np.floor(pos).astype(np.int64)
  return len(set(np.clip(lo, 0, src - 1)) | set(np.clip(lo + 1, 0, src - 1)))


def bytes_moved(n, t, h0, w0, size, masked):
  """(fused, op by op): source bytes the taps need (each once) + bytes written; the op-by-op chain
  also re-reads the resized image for the mask multiply.  These are the bytes the algorithm needs,
  a lower bound on the traffic: the nearest planes count one element per output pixel, while the
  hardware fetches whole cache lines of every source row it touches (at 2x about twice that for
  the depth planes), so the share of the HBM rate printed from them is a lower bound too."""
  h, w = size, 2 * size
  frames, px = n * t, n * t * h * w
  read = frames * taps(h, h0) * taps(w, w0) * 12 + px * sum(PLANES.values())
  write = px * (12 + sum(PLANES.values()))
  fused = read + write + (px * 12 if masked else 0)
  chain = read + write + (px * 24 if masked else 0)
  return fused, chain


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
  a = ap.parse_args()
  t, h0 = 8, 1024
  w0 = 2 * h0
  results = []
  for n in (1, 4):
    g = torch.Generator(device=DEV).manual_seed(n)
    raw = dict(
        image=torch.rand((n, t, h0, w0, 3), device=DEV, generator=g),
        position=torch.rand((n, t, 4), device=DEV, generator=g))
    for k, b in PLANES.items():
      raw[k] = (torch.rand((n, t, h0, w0), device=DEV, generator=g) if b == 4 else
                torch.randint(0, 42, (n, t, h0, w0), device=DEV, generator=g, dtype=torch.uint8))
    for size in (512, 128):
      for ratio in (0.0, 0.25):
        ds = indoor_datasets.R2RVideoDataset(image_size=size, horizontal_mask_ratio=ratio)
        rng = np.random.default_rng(7)
        params = [ds.draw_params(rng) for _ in range(n)]
        fa = lambda: ds.device_transform(raw, params)
        fb = lambda: op_by_op(raw, params, size)
        got, want = fa(), fb()
        for k in want:
          assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (n, size, ratio, k)
        del got, want
        for _ in range(3):   # warm-up of both legs
          fa()
          fb()
        torch.cuda.synchronize()
        ta, tb1, tb2 = [], [], []
        for _ in range(a.rounds):
          tb1.append(time_ms(fb, a.iters))
          ta.append(time_ms(fa, a.iters))
          tb2.append(time_ms(fb, a.iters))
        ms_a = float(np.median(ta))
        ms_b = float(np.median(tb1 + tb2))
        # (b) against itself: the largest relative gap between the two (b) legs of one round
        spread = float(max(abs(x - y) / min(x, y) for x, y in zip(tb1, tb2)))
        fused_bytes, chain_bytes = bytes_moved(n, t, h0, w0, size, ratio > 0)
        r = dict(batch=n, frames=t, src=[h0, w0], dst=[size, 2 * size], mask_ratio=ratio,
                 fused_ms=ms_a, op_by_op_ms=ms_b, fused_over_op_by_op=ms_a / ms_b,
                 op_by_op_self_spread=spread, fused_bytes=fused_bytes, op_by_op_bytes=chain_bytes,
                 fused_bytes_per_ms=fused_bytes / ms_a,
                 fused_share_of_hbm=fused_bytes / (ms_a * 1e-3) / HBM_ACHIEVABLE,
                 op_by_op_share_of_hbm=chain_bytes / (ms_b * 1e-3) / HBM_ACHIEVABLE,
                 fused_ms_rounds=ta, op_by_op_ms_rounds=tb1 + tb2)
        results.append(r)
        print(f'batch {n} {h0}x{w0} -> {size}x{2 * size} mask {ratio:4.2f}: fused {ms_a:7.3f} ms '
              f'({fused_bytes / 1e6:7.1f} MB, {r["fused_bytes_per_ms"] / 1e9:5.2f} GB/ms, '
              f'{100 * r["fused_share_of_hbm"]:4.1f} % of 6.3 TB/s)  op by op {ms_b:7.3f} ms '
              f'({chain_bytes / 1e6:7.1f} MB)  fused / op-by-op {ms_a / ms_b:5.3f}  '
              f'op-by-op against itself +-{100 * spread:4.1f} %', flush=True)
    del raw
    torch.cuda.empty_cache()
  doc = dict(tool='tools/video_input_bench.py', rounds=a.rounds, iters=a.iters,
             hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, device=torch.cuda.get_device_name(0),
             results=results)
  print(json.dumps(doc))
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(doc, f, indent=1)


if __name__ == '__main__':
  main()
