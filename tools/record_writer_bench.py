"""Writes B synthetic training examples at 512 x 1024 to a record file both ways and prints both
times and both file sizes.

  python tools/record_writer_bench.py [--examples 8] [--height 512] [--flush 8] [--repeats 5] [--out FILE.json]

Device: datasets/record_writer.R2RRecordWriter with profile=True -- host clocks around every group
of launches of a flush, each followed by a synchronise (encode + the download of the sizes; layout
on the host + the upload; assemble; IDAT CRC-32 + patch; record CRC-32C + patch; the download; the
file write) -- alternating with the same write without the extra synchronisations, end to end;
medians of --repeats writes, with the smallest and largest.  The file is read back
with both checksums verified and one plane decoded.
Host: only what the project had before the writer: utils/png.filter_rows_host (adaptive, on the
big-endian bytes for the 16-bit planes) + zlib level 6 for the planes, tf_records.encode_example and
tf_records.frame_record (the Python CRC-32C loop) for the file.
Without a device the host half runs alone and the device half is reported as null."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from se3ds_amd.datasets import indoor_datasets, record_writer  # noqa: E402
from se3ds_amd.utils import png, tf_records  # noqa: E402


def example(h, seed):
  """One example's seven planes: a gradient + noise panorama and its shifted copy as guidance, smooth
  16-bit depths with sensor-like noise, blob masks, a blocky label map."""
  rng = np.random.default_rng(seed)
  w = 2 * h
  x, y = np.arange(w)[None, :], np.arange(h)[:, None]
  base = (0.6 * x / w + 0.3 * y / h)[:, :, None] + np.array([0.0, 0.03, 0.06])
  image = np.clip((base + rng.normal(0, 3 / 255, (h, w, 3))) * 255, 0, 255).astype(np.uint8)
  depth = np.clip((0.2 + 0.5 * np.abs(np.sin(x / 97.0) * np.cos(y / 61.0))) * 65535 +
                  rng.normal(0, 40, (h, w)), 0, 65535).astype(np.uint16)
  blobs = lambda t: (np.kron(rng.random((max(h // 32, 1), max(w // 32, 1))), np.ones((32, 32)))[:h, :w] > t)
  mask = blobs(0.3)
  return dict(image=image, depth=depth,
              proj_image=np.where(mask[:, :, None], np.roll(image, 9, axis=1), 0).astype(np.uint8),
              proj_depth=np.where(mask, np.roll(depth, 9, axis=1), 0).astype(np.uint16),
              proj_mask=(mask * 255).astype(np.uint8), blurred_mask=blobs(0.9).astype(np.uint8),
              segmentation=(np.kron(rng.integers(0, 42, (max(h // 64, 1), max(w // 64, 1))),
                                    np.ones((64, 64), np.int64))[:h, :w]).astype(np.uint8))


def host_png(pixels):
  """A PNG file from the parent's pieces: the NumPy filters, zlib level 6, the chunk writer."""
  if pixels.dtype == np.uint16:
    depth, channels = 16, 1
    raw = np.ascontiguousarray(pixels.astype('>u2')).view(np.uint8).reshape(pixels.shape[0], -1, 2)
  else:
    depth, channels = 8, 1 if pixels.ndim == 2 else 3
    raw = pixels.reshape(pixels.shape[0], pixels.shape[1], channels)
  filtered = png.filter_rows_host(raw, png.ADAPTIVE)
  ihdr = struct.pack('>IIBBBBB', pixels.shape[1], pixels.shape[0], depth, 0 if channels == 1 else 2, 0, 0, 0)
  return (png.SIGNATURE + png._chunk(b'IHDR', ihdr) + png._chunk(b'IDAT', zlib.compress(filtered.tobytes(), 6)) +
          png._chunk(b'IEND', b''))


def host_write(path, examples):
  clock = dict(png=0.0, example=0.0, frame=0.0)
  with open(path, 'wb') as f:
    for planes in examples:
      t = time.perf_counter()
      files = {name: host_png(px) for name, px in planes.items()}
      clock['png'] += time.perf_counter() - t
      t = time.perf_counter()
      payload = tf_records.encode_example(record_writer.example_features(files))
      clock['example'] += time.perf_counter() - t
      t = time.perf_counter()
      f.write(tf_records.frame_record(payload))
      clock['frame'] += time.perf_counter() - t
  return clock


def device_write(path, tensors, flush, profile):
  torch.cuda.synchronize()
  t = time.perf_counter()
  with record_writer.R2RRecordWriter(path, 'cuda', examples_per_flush=flush, profile=profile) as writer:
    for planes in tensors:
      writer.add(**planes)
  total = time.perf_counter() - t
  groups = {}
  for clock in writer.timings:
    for k, v in clock.items():
      groups[k] = groups.get(k, 0.0) + v
  return total, groups


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--examples', type=int, default=8)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--flush', type=int, default=8, help='examples per flush of the device writer')
  ap.add_argument('--host-examples', type=int, default=None, help='examples the host path writes (default: all)')
  ap.add_argument('--repeats', type=int, default=5, help='device writes of each kind; medians are reported')
  ap.add_argument('--out', default=None, help='also write the JSON result to this file')
  args = ap.parse_args()
  h = args.height
  examples = [example(h, s) for s in range(args.examples)]
  raw_bytes = sum(px.nbytes for px in examples[0].values())
  result = dict(examples=args.examples, height=h, width=2 * h, examples_per_flush=args.flush,
                raw_bytes_per_example=raw_bytes)
  with tempfile.TemporaryDirectory() as tmp:
    host_n = args.examples if args.host_examples is None else min(args.host_examples, args.examples)
    path = os.path.join(tmp, 'train-host.tfrecord')
    t = time.perf_counter()
    clock = host_write(path, examples[:host_n])
    result['host'] = dict(examples=host_n, seconds=time.perf_counter() - t, file_bytes=os.path.getsize(path),
                          seconds_by_stage=clock)
    assert len(list(tf_records.read_records(path, verify=False))) == host_n
    print(f"host:   {host_n} examples, {result['host']['seconds']:.3f} s, {result['host']['file_bytes']} bytes "
          + ', '.join(f'{k} {v:.3f} s' for k, v in clock.items()), flush=True)
    if not torch.cuda.is_available():
      result['device'] = None
      print('device: none here -- the device half needs an MI355X')
    else:
      to_dev = lambda px: torch.from_numpy(px.view(np.int16) if px.dtype == np.uint16 else px).cuda()
      tensors = [{k: to_dev(v) for k, v in planes.items()} for planes in examples]
      path = os.path.join(tmp, 'train-device.tfrecord')
      device_write(path, tensors[:1], 1, False)   # warm-up: allocator, kernels' code objects
      runs, profiled_runs = [], []   # alternating, so that both see the same machine
      for _ in range(args.repeats):
        profiled_runs.append(device_write(path, tensors, args.flush, True))
        runs.append(device_write(path, tensors, args.flush, False)[0])
      total = float(np.median(runs))
      profiled = float(np.median([p[0] for p in profiled_runs]))
      groups = {k: float(np.median([p[1][k] for p in profiled_runs])) for k in profiled_runs[0][1]}
      records = list(tf_records.read_records(path, verify='device'))
      assert len(records) == args.examples
      feature = indoor_datasets.IMAGE_PLANES['depth'][0]
      back = png.decode_png_batch({'depth': [tf_records.parse_example(records[-1])[feature][0]]}, 'cuda')
      assert torch.equal(back['depth'][0], tensors[-1]['depth']), 'the written depth does not decode to its samples'
      result['device'] = dict(examples=args.examples, repeats=args.repeats, seconds=total,
                              seconds_min=min(runs), seconds_max=max(runs), seconds_profiled=profiled,
                              file_bytes=os.path.getsize(path), seconds_by_group=groups)
      print(f"device: {args.examples} examples, median of {args.repeats}: {total:.4f} s (min {min(runs):.4f}, max "
            f"{max(runs):.4f}; {profiled:.4f} s with a synchronise per group), "
            f"{result['device']['file_bytes']} bytes " + ', '.join(f'{k} {v:.4f} s' for k, v in groups.items()))
  line = json.dumps({'record_writer_bench': result})
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
