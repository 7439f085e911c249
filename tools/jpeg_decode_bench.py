"""The device JPEG decode on panorama-sized files: 1024 x 2048 and 2048 x 4096, 4:2:0 and 4:4:4.

Input: a smooth-plus-texture synthetic scene, written by Pillow at quality 75 and 90 where Pillow is
importable, otherwise by the tests' writer with sparse random coefficients.  Per file: the decoded
pixels equal Pillow's first (where Pillow wrote the file); then device-event times of
`se3ds_jpeg_decode` with phases 1, 2, 4 (each alone, on the workspace the one before left) and 7
after a warm-up (median of --repeats), the whole `decode_jpeg_batch` call by the host clock, the rounds per
window from the status words, and Pillow's host decode of the same bytes on one thread -- the
comparison, never the code under test.  A table and one JSON line (--json FILE).

  python tools/jpeg_decode_bench.py [--repeats 20] [--sizes 1024x2048,2048x4096] [--json FILE]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.utils import jpeg  # noqa: E402

try:
  from PIL import Image
except ImportError:   # the tests' writer stands in
  Image = None


def scene(h, w, rng):
  """Smooth gradients and blobs plus band-limited texture, uint8 (h, w, 3)."""
  y, x = np.mgrid[0:h, 0:w].astype(np.float32)
  base = np.stack([128 + 90 * np.sin(x / w * 6.28 * f + p) * np.cos(y / h * 3.14 * g)
                   for f, g, p in ((1, 1, 0.0), (2, 1, 1.0), (1, 3, 2.0))], -1)
  noise = rng.normal(0, 1, (h // 4, w // 4, 3)).astype(np.float32)
  texture = np.repeat(np.repeat(noise, 4, 0), 4, 1) * 12 + rng.normal(0, 4, (h, w, 3))
  return np.clip(base + texture, 0, 255).astype(np.uint8)


def make_file(h, w, sampling, quality, rng):
  if Image is not None:
    buf = io.BytesIO()
    Image.fromarray(scene(h, w, rng)).save(buf, 'JPEG', quality=quality, subsampling={'444': 0, '420': 2}[sampling])
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)))
  import _jpeg_ref as J
  coefs = J.random_coefs(rng, h, w, sampling, density=0.08 if quality < 80 else 0.15, dc=100, ac=12)
  return J.write_jpeg(coefs, h, w, sampling).data, J.expected(coefs, h, w, sampling)


def device_ms(fn, repeats):
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return statistics.median(times), min(times), max(times)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--sizes', default='1024x2048,2048x4096')
  ap.add_argument('--json')
  args = ap.parse_args()
  dev = torch.device('cuda', torch.cuda.current_device())
  L = _lib.lib()
  W = L.se3ds_jpeg_decode_lanes() * L.se3ds_jpeg_decode_chunk_bytes()
  rng = np.random.default_rng(7)
  rows = []
  for size in args.sizes.split(','):
    h, w = (int(v) for v in size.split('x'))
    for sampling in ('420', '444'):
      for quality in (75, 90):
        data, want = make_file(h, w, sampling, quality, rng)
        scan = jpeg.parse_jpeg(data)
        (got,), pending = jpeg.decode_jpeg_batch([scan], dev, check=False)
        pending.check()
        equal = bool(np.array_equal(got.cpu().numpy(), want))
        words = pending.words
        windows = sum(-(-n // W) for _, n in scan.segments)
        rounds = int(jpeg.status_rounds(words).sum())
        # the library call alone: tables and bytes uploaded once, outside the timed region
        batch = jpeg.JpegBatch([scan], dev)
        # each phase on its own (2 and 4 read what the phases before them left in the workspace), then all
        t = {p: device_ms(lambda p=p: batch.launch(p), args.repeats) for p in (1, 2, 4, 7)}
        assert np.array_equal(batch.out[0].cpu().numpy(), want) == equal
        t0 = time.perf_counter()
        for _ in range(5):
          jpeg.decode_jpeg_batch([data], dev)
        whole = (time.perf_counter() - t0) / 5 * 1e3
        pillow = None
        if Image is not None:
          torch.set_num_threads(1)
          host = []
          for _ in range(5):
            t0 = time.perf_counter()
            Image.open(io.BytesIO(data)).load()
            host.append((time.perf_counter() - t0) * 1e3)
          pillow = statistics.median(host)
        row = dict(size=size, sampling=sampling, quality=quality, file_bytes=len(data),
                   entropy_bytes=sum(n for _, n in scan.segments), segments=len(scan.segments), equal=equal,
                   entropy_ms=t[1][0], idct_ms=t[2][0], pixel_ms=t[4][0], total_ms=t[7][0],
                   total_min_ms=t[7][1], total_max_ms=t[7][2], rounds_per_window=rounds / max(windows, 1),
                   windows=windows, call_ms=whole, pillow_ms=pillow,
                   writer='pillow' if Image is not None else 'tests/_jpeg_ref.py')
        rows.append(row)
        print('{size} {sampling} q{quality}: {entropy_bytes} entropy bytes, equal {equal}; entropy {entropy_ms:.3f} '
              'idct {idct_ms:.3f} pixel {pixel_ms:.3f} total {total_ms:.3f} ms [{total_min_ms:.3f}, '
              '{total_max_ms:.3f}]; {rounds_per_window:.1f} rounds/window over {windows} windows; whole call '
              '{call_ms:.2f} ms; Pillow {pillow_ms} ms'.format(**row), flush=True)
  line = json.dumps(dict(tool='jpeg_decode_bench', device=torch.cuda.get_device_name(dev), repeats=args.repeats,
                         rows=rows))
  print(line)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
