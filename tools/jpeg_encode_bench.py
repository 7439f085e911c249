"""The device JPEG encode on the shapes the project writes: a batch of 64 roll-out panoramas
(512 x 1024, 4:2:0), one 1024 x 2048 panorama at 4:4:4, one 2048 x 4096 sheet at 4:2:0, and the nine
2048 x 4096 sheets of a TensorBoard event -- at quality 75 and 90.

Per case: the device's files equal Pillow's first (where Pillow is importable); then device-event
times of `se3ds_jpeg_encode` with phases 1, 2, 4, 8 (each alone, on the workspace the one before
left) and 15, on a table uploaded once, after a warm-up (median, min, max of --repeats); the whole
`encode_jpeg_batch` call (upload, launches, both read-backs, containers) by the host clock; and
Pillow's encode of the same pixels on one host thread -- the comparison, never the code under test;
for the single images also what reading the whole worst-case output buffer back would cost.
For the nine sheets also `encode_png_batch` of the same pixels and its size; for the 2048 x 4096
picture `decode_jpeg_batch` of the file written with restart_interval='row' against the file
without restarts.  A table and one JSON line (--json FILE).

  python tools/jpeg_encode_bench.py [--repeats 20] [--json FILE]
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

from se3ds_amd.utils import jpeg, png  # noqa: E402
from se3ds_amd.utils._staging import Readback  # noqa: E402

try:
  from PIL import Image
except ImportError:
  Image = None

CASES = [   # name, height, width, batch, subsampling, qualities
    ('rollouts', 512, 1024, 64, '4:2:0', (75, 90)),
    ('panorama', 1024, 2048, 1, '4:4:4', (75, 90)),
    ('sheet', 2048, 4096, 1, '4:2:0', (75, 90)),
    ('nine_sheets', 2048, 4096, 9, '4:2:0', (90,)),
]


def scene(h, w, rng):
  """Smooth gradients plus band-limited texture, uint8 (h, w, 3)."""
  y, x = np.mgrid[0:h, 0:w].astype(np.float32)
  base = np.stack([128 + 90 * np.sin(x / w * 6.28 * f + p) * np.cos(y / h * 3.14 * g)
                   for f, g, p in ((1, 1, 0.0), (2, 1, 1.0), (1, 2, 2.0))], -1)
  noise = rng.normal(0, 1, (h // 4 + 1, w // 4 + 1, 3)).astype(np.float32)
  texture = np.kron(noise, np.ones((4, 4, 1), np.float32))[:h, :w] * 10
  return np.clip(base + texture, 0, 255).astype(np.uint8)


def stats(xs):
  return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs)}


def device_ms(fn, repeats):
  out = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b))
  return stats(out)


def host_ms(fn, repeats):
  out = []
  for _ in range(repeats):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t) * 1e3)
  return stats(out)


def pillow_encode(px, quality, subsampling):
  buf = io.BytesIO()
  Image.fromarray(px).save(buf, 'JPEG', quality=quality, subsampling=subsampling)
  return buf.getvalue()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--json', default=None)
  ap.add_argument('--cases', default=','.join(c[0] for c in CASES))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('jpeg_encode_bench: no GPU; a time measured anywhere else says nothing')
  torch.set_num_threads(1)
  dev = torch.device('cuda', torch.cuda.current_device())
  rng = np.random.default_rng(0)
  results = []
  for name, h, w, batch, sub, qualities in CASES:
    if name not in args.cases.split(','):
      continue
    distinct = [scene(h, w, rng) for _ in range(min(batch, 3))]
    pixels = [distinct[i % len(distinct)] for i in range(batch)]
    images = [torch.from_numpy(p).to(dev) for p in pixels]
    for q in qualities:
      row = {'case': name, 'height': h, 'width': w, 'batch': batch, 'subsampling': sub, 'quality': q}
      files = jpeg.encode_jpeg_batch(images, quality=q, subsampling=sub)
      row['bytes'] = sum(len(f) for f in files)
      if Image is not None:
        want = [pillow_encode(p, q, sub) for p in distinct]
        row['equals_pillow'] = all(f == want[i % len(distinct)] for i, f in enumerate(files))
        if not row['equals_pillow']:
          sys.exit(f'jpeg_encode_bench: {name} q{q} {sub}: the device files differ from Pillow\'s; nothing is timed')
        per = host_ms(lambda: pillow_encode(distinct[0], q, sub), max(3, args.repeats // 4))
        row['pillow_one_thread'] = {k: v * batch for k, v in per.items()}
      specs = jpeg.encode_specs([x.shape for x in images], [x.dtype for x in images], q, sub, 0)
      b = jpeg.JpegEncodeBatch(images, specs)
      row['workspace_bytes'], row['out_bytes'] = int(b.workspace_bytes), int(b.out_bytes)
      for _ in range(3):
        b.launch(15)
      torch.cuda.synchronize()
      for phases, key in ((1, 'transform'), (2, 'measure'), (4, 'pack_count'), (8, 'pack_write'), (15, 'all_phases')):
        row[key] = device_ms(lambda: b.launch(phases), args.repeats)
      if batch == 1:   # what one read-back of the whole worst-case output buffer would cost
        row['whole_out_readback'] = host_ms(lambda: Readback(b.out).wait(), max(3, args.repeats // 4))
      del b
      row['end_to_end'] = host_ms(lambda: jpeg.encode_jpeg_batch(images, quality=q, subsampling=sub),
                                  max(3, args.repeats // 2))
      if name == 'nine_sheets':
        pngs = png.encode_png_batch(images)
        row['png_bytes'] = sum(len(f) for f in pngs)
        row['png_end_to_end'] = host_ms(lambda: png.encode_png_batch(images), max(3, args.repeats // 4))
      if name == 'sheet':
        plain = files[0]
        rows = jpeg.encode_jpeg_batch(images, quality=q, subsampling=sub, restart_interval='row')[0]
        a, c = jpeg.decode_jpeg_batch([plain], dev)[0], jpeg.decode_jpeg_batch([rows], dev)[0]
        row['restart_rows_decodes_equal'] = bool(torch.equal(a, c))
        row['restart_rows_bytes'] = len(rows)
        row['decode_no_restart'] = host_ms(lambda: jpeg.decode_jpeg_batch([plain], dev), max(3, args.repeats // 2))
        row['decode_restart_rows'] = host_ms(lambda: jpeg.decode_jpeg_batch([rows], dev), max(3, args.repeats // 2))
      results.append(row)
      print(f"{name:12s} q{q} {sub}: transform {row['transform']['median_ms']:.3f}  measure "
            f"{row['measure']['median_ms']:.3f}  pack count {row['pack_count']['median_ms']:.3f}  write "
            f"{row['pack_write']['median_ms']:.3f}  all {row['all_phases']['median_ms']:.3f}"
            f"  end to end {row['end_to_end']['median_ms']:.2f} ms  Pillow "
            f"{row.get('pillow_one_thread', {}).get('median_ms', float('nan')):.1f} ms  {row['bytes']} bytes"
            f"  equal {row.get('equals_pillow')}", flush=True)
  line = json.dumps({'tool': 'jpeg_encode_bench', 'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats,
                     'results': results})
  print(line)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
