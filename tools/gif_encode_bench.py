"""The device GIF encode on a roll-out's shape: one video of 8 frames at 512 x 1024 x 3, and a batch
of eight such videos.

Per case: the device's files equal encode_gif_host's for one video first; then, per stage
(histogram, look-up table, index plane, LZW, pack), the device time of one launch from device events
around --launches launches queued back to back on a table uploaded once (median, min, max of
--repeats such windows, after a warm-up); the bytes each stage must move, and for the three
streaming stages (histogram, index plane, pack) their share of the HBM peak bench.py uses; for LZW
the pixels per microsecond of one strip (a strip's pixels over the launch time when every strip is
resident at once, else not stated) and of the launch; the whole `encode_gif_batch` call (upload,
launches, both host synchronisations, the median cut, containers) by the host clock; and the same
frames through Pillow's save(..., save_all=True) on one host thread where Pillow is importable,
otherwise through encode_gif_host -- the comparison, never the code under test.  A table and one
JSON line (--json FILE).

  python tools/gif_encode_bench.py [--repeats 5] [--launches 10] [--json FILE]
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

from se3ds_amd.utils import gif  # noqa: E402

try:
  from PIL import Image
except ImportError:
  Image = None

HBM_PEAK_GBS = 8000.0    # as bench.py has it
CASES = [('one_video', 8, 512, 1024, 1), ('eight_videos', 8, 512, 1024, 8)]   # name, frames, height, width, batch
RESIDENT_STRIPS = 256 * 5    # 256 CUs, five 32 KiB tables in a CU's 160 KiB of LDS


def scene(t, h, w, rng):
  """A drifting panorama: smooth gradients plus band-limited texture, uint8 (t, h, w, 3)."""
  y, x = np.mgrid[0:h, 0:w].astype(np.float32)
  base = np.stack([128 + 90 * np.sin(x / w * 6.28 * f + p) * np.cos(y / h * 3.14 * g)
                   for f, g, p in ((1, 1, 0.0), (2, 1, 1.0), (1, 2, 2.0))], -1)
  noise = rng.normal(0, 1, (h // 4 + 1, w // 4 + 1, 3)).astype(np.float32)
  frame = np.clip(base + np.kron(noise, np.ones((4, 4, 1), np.float32))[:h, :w] * 10, 0, 255).astype(np.uint8)
  return np.stack([np.roll(frame, 16 * i, axis=1) for i in range(t)])


def stats(xs):
  return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs)}


def device_ms(fn, repeats, launches):
  out = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
      fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b) / launches)
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


def pillow_encode(video):
  frames = [Image.fromarray(f) for f in video]
  buf = io.BytesIO()
  frames[0].save(buf, 'GIF', save_all=True, append_images=frames[1:], duration=100, loop=0)
  return buf.getvalue()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--launches', type=int, default=10)
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('gif_encode_bench: no GPU; a time measured anywhere else says nothing')
  torch.set_num_threads(1)
  dev = torch.device('cuda', torch.cuda.current_device())
  rng = np.random.default_rng(0)
  results = []
  for name, t, h, w, batch in CASES:
    distinct = [scene(t, h, w, rng) for _ in range(min(batch, 2))]
    videos = [torch.from_numpy(distinct[i % len(distinct)]).to(dev) for i in range(batch)]
    pixels = batch * t * h * w
    row = {'case': name, 'frames': t, 'height': h, 'width': w, 'batch': batch, 'pixels': pixels}
    files = gif.encode_gif_batch(videos)
    row['bytes'] = sum(len(f) for f in files)
    tick = time.perf_counter()
    want = gif.encode_gif_host(distinct[0])
    row['encode_gif_host_one_video_ms'] = (time.perf_counter() - tick) * 1e3
    if files[0] != want:
      sys.exit(f'gif_encode_bench: {name}: the device file differs from encode_gif_host\'s; nothing is timed')
    if Image is not None:
      per = host_ms(lambda: pillow_encode(distinct[0]), 3)
      row['pillow_one_thread'] = {k: v * batch for k, v in per.items()}
      row['pillow_bytes_one_video'] = len(pillow_encode(distinct[0]))

    b = gif.GifBatch(videos, 32)
    row['workspace_bytes'], row['out_bytes'], strips = int(b.workspace_bytes), int(b.out_bytes), int(b.offsets[5] - b.offsets[4]) // 4
    row['strips'] = strips
    b.histogram()
    hists = b.histograms().cpu().numpy().view(np.uint32)
    tick = time.perf_counter()
    cut = [gif.median_cut(hists[i]) for i in range(batch)]
    row['median_cut_host_ms'] = (time.perf_counter() - tick) * 1e3
    palettes, used = np.stack([p for p, _ in cut]), np.array([u for _, u in cut], np.int32)
    stages = [('histogram', b.histogram), ('lut', lambda: b.lut(palettes, used)), ('index', b.index),
              ('lzw', b.lzw), ('pack', b.pack)]
    for _, fn in stages:    # warm-up, and every stage's input in place
      fn()
    torch.cuda.synchronize()
    packed = sum(len(f) for f in files) - batch * (13 + 768 + 19 + 1) - batch * t * 19   # the sub-blocks
    moved = {'histogram': 3 * pixels, 'lut': batch * (32768 + 768), 'index': 4 * pixels,
             'lzw': pixels + packed, 'pack': 2 * packed}
    for key, fn in stages:
      row[key] = device_ms(fn, args.repeats, args.launches)
      row[key]['bytes'] = moved[key]
      if key in ('histogram', 'index', 'pack'):
        row[key]['hbm_fraction'] = moved[key] / (row[key]['median_ms'] * 1e-3) / 1e9 / HBM_PEAK_GBS
    lzw_us = row['lzw']['median_ms'] * 1e3
    row['lzw']['pixels_per_us'] = pixels / lzw_us
    if strips <= RESIDENT_STRIPS:
      row['lzw']['pixels_per_us_per_strip'] = gif.strip_rows(w) * w / lzw_us
    del b
    row['end_to_end'] = host_ms(lambda: gif.encode_gif_batch(videos), args.repeats)
    results.append(row)
    print(f"{name:12s}: histogram {row['histogram']['median_ms']:.3f} ({row['histogram']['hbm_fraction']:.1%} of HBM)"
          f"  lut {row['lut']['median_ms']:.3f}  index {row['index']['median_ms']:.3f} "
          f"({row['index']['hbm_fraction']:.1%})  lzw {row['lzw']['median_ms']:.3f} "
          f"({row['lzw'].get('pixels_per_us_per_strip', float('nan')):.1f} px/us a strip)  pack "
          f"{row['pack']['median_ms']:.3f} ({row['pack']['hbm_fraction']:.1%})  median cut "
          f"{row['median_cut_host_ms']:.1f}  end to end {row['end_to_end']['median_ms']:.1f} ms  Pillow "
          f"{row.get('pillow_one_thread', {}).get('median_ms', float('nan')):.0f} ms  host encoder "
          f"{row['encode_gif_host_one_video_ms'] * batch:.0f} ms  {row['bytes']} bytes", flush=True)
  line = json.dumps({'tool': 'gif_encode_bench', 'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats,
                     'launches': args.launches, 'results': results})
  print(line)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
