"""Times the device .ply writer (csrc/ply.hip, utils/ply.py) against the host loop on the points of a
real unprojection: a synthetic depth panorama through equirectangular_to_pointcloud, 512 x 1024
(2^19 points) and 1024 x 2048 (2^21 points).

  python tools/ply_bench.py [--repeats 5] [--host-points 200000] [--dir DIR] [--json FILE]

Kernels: the three launches of se3ds_ply_ascii apart and the binary launch, by device events.  Whole
write_ply calls by the host clock, to files in DIR (default: the temporary directory, a local disk):
the device encoder (b), the host loop (a) on the first --host-points points (it is linear in the
points: 72 bytes and one str.format each; the full sizes take seconds to minutes) and (b) again, so
that the spread of (b) against itself stands next to the difference from (a).  Prints a table and one
JSON line; --json also writes it to a file."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.utils import pano_utils, ply  # noqa: E402

DEV = torch.device('cuda:0')


def cloud(height, seed):
  """(4, H * 2H) coordinates and (H * 2H, 3) int32 colours of a room-like panorama: smooth depth in
  [0.1, 0.9], every pixel valid, a position added as the model does."""
  g = torch.Generator().manual_seed(seed)
  width = 2 * height
  v = torch.linspace(0, 1, height).view(height, 1)
  u = torch.linspace(0, 1, width).view(1, width)
  depth = (0.5 + 0.3 * torch.sin(6.2832 * u) * torch.cos(3.1416 * v) + 0.1 * torch.rand((height, width), generator=g))
  rgb = torch.randint(0, 256, (1, height, width, 3), generator=g, dtype=torch.int32)
  position = torch.tensor([[1.25, -0.5, 0.75]])
  xyz1, feats = pano_utils.equirectangular_to_pointcloud(rgb.to(DEV), depth.clamp(0.1, 0.9)[None].to(DEV), -1.0, 10.0,
                                                         interpolation_method='nearest', position=position.to(DEV))
  return xyz1[0].contiguous(), feats[0].to(torch.int32).contiguous()


def device_ms(fn, repeats):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(repeats):
    start.record()
    fn()
    end.record()
    end.synchronize()
    times.append(start.elapsed_time(end))
  return float(np.median(times))


def wall_ms(fn, repeats):
  times = []
  for _ in range(repeats):
    t = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t) * 1e3)
  return times


def kernels(coords, rgb, repeats):
  L = _lib.lib()
  m = coords.shape[1]
  text = torch.empty((m * L.se3ds_ply_max_line_bytes(),), dtype=torch.uint8, device=DEV)
  count = torch.zeros((2,), dtype=torch.int64, device=DEV)
  ws = torch.empty((L.se3ds_ply_ascii_workspace_bytes(m),), dtype=torch.uint8, device=DEV)

  def ascii(phases):
    _lib.check(L.se3ds_ply_ascii(coords.data_ptr(), coords.stride(0), rgb.data_ptr(), _lib.dtype_code(rgb), m,
                                 text.data_ptr(), text.numel(), count.data_ptr(), ws.data_ptr(), ws.numel(), phases,
                                 _lib.stream()), 'ply_ascii')

  def binary():
    _lib.check(L.se3ds_ply_binary(coords.data_ptr(), coords.stride(0), rgb.data_ptr(), _lib.dtype_code(rgb), m,
                                  text.data_ptr(), text.numel(), count[1:].data_ptr(), _lib.stream()), 'ply_binary')

  out = {'records_ms': device_ms(lambda: ascii(1), repeats), 'scan_ms': device_ms(lambda: ascii(2), repeats),
         'emit_ms': device_ms(lambda: ascii(4), repeats), 'ascii_ms': device_ms(lambda: ascii(7), repeats),
         'binary_ms': device_ms(binary, repeats)}
  out['ascii_bytes'] = int(count[0].item())
  out['ascii_ns_per_value'] = out['ascii_ms'] * 1e6 / (6 * m)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--host-points', type=int, default=200000)
  ap.add_argument('--dir', default=tempfile.gettempdir())
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'ply_bench needs an MI355X'
  rows = {}
  with tempfile.TemporaryDirectory(dir=args.dir) as d:
    path = os.path.join(d, 'cloud.ply')
    for height in (512, 1024):
      coords, rgb = cloud(height, seed=height)
      m = coords.shape[1]
      row = {'points': m}
      row.update(kernels(coords, rgb, args.repeats))
      device = lambda format='ascii': ply.write_ply(path, coords, rgb, format=format, encoder='device')
      device()   # pinned buffers, workspaces
      b1 = wall_ms(device, args.repeats)
      h = min(args.host_points, m)
      a = wall_ms(lambda: ply.write_ply(path, coords[:, :h], rgb[:h]), 1)
      host_bytes = os.path.getsize(path)
      b2 = wall_ms(device, args.repeats)
      row['file_bytes'] = os.path.getsize(path)
      row['device_write_ms'] = float(np.median(b1 + b2))
      row['device_write_spread_ms'] = abs(float(np.median(b1)) - float(np.median(b2)))
      row['device_ns_per_point'] = row['device_write_ms'] * 1e6 / m
      row['host_points'] = h
      row['host_write_ms'] = a[0]
      row['host_ns_per_point'] = a[0] * 1e6 / h
      row['host_bytes_per_point'] = host_bytes / h
      device('binary_little_endian')
      row['binary_write_ms'] = float(np.median(wall_ms(lambda: device('binary_little_endian'), args.repeats)))
      row['binary_file_bytes'] = os.path.getsize(path)
      # where the device path's time goes: the download and the file write of the same bytes, apart
      text = torch.empty((row['ascii_bytes'],), dtype=torch.uint8, device=DEV)
      host = torch.empty((row['ascii_bytes'],), dtype=torch.uint8, pin_memory=True)

      def download():
        host.copy_(text, non_blocking=True)
        torch.cuda.current_stream().synchronize()

      def file_write():
        with open(path, 'wb') as f:
          f.write(memoryview(host.numpy()))
          f.flush()
          os.fsync(f.fileno())

      row['download_ms'] = float(np.median(wall_ms(download, args.repeats)))
      row['file_write_ms'] = float(np.median(wall_ms(file_write, args.repeats)))
      # the device file equals the host loop's on the points the host wrote
      ply.write_ply(path, coords[:, :h], rgb[:h], encoder='device')
      got = open(path, 'rb').read()
      ply.write_ply(path, coords[:, :h], rgb[:h])
      assert got == open(path, 'rb').read(), 'the device file differs from the host loop\'s'
      rows[f'{height} x {2 * height}'] = row
      print(f'{height} x {2 * height}: ' + ', '.join(f'{k} {v:.3f}' if isinstance(v, float) else f'{k} {v}'
                                                     for k, v in row.items()), flush=True)
  line = json.dumps({'ply_bench': rows})
  print(line)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
