"""Times the device PNG encoder (csrc/png_encode.hip) against the host encoders on the sheets a
TensorBoard log event writes: one 2048 x 4096 x 3 sheet (16 panoramas of 512 x 1024, 4 x 4) and a
nine-sheet event, on gradient + noise panoramas and on a mask-like sheet.

  python tools/png_encode_bench.py [--repeats 5] [--host-sheets 1]

Device: quantise (se3ds_grid_quantize), the strips, the packing, the download, the host container,
each timed apart (device events around the launches; a host clock around what ends in a
synchronise), and encode_png_batch end to end.  Host: GANManager's `_encode_png` (filter 0, zlib
level 6) and utils/png.encode_png_host (adaptive filters, Z_RLE) on the same pixels.  Prints a
table and one JSON line."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.trainers.gan_manager import _encode_png  # noqa: E402
from se3ds_amd.utils import image_grid, png  # noqa: E402

H, W, NY, NX = 512, 1024, 4, 4


def panoramas(seed):
  """16 float panoramas: a gradient + sigma-3 noise (in 1/255 units), what a generated image is to
  a compressor."""
  g = torch.Generator().manual_seed(seed)
  x = torch.linspace(0, 1, W).view(1, 1, W, 1) * 0.6 + torch.linspace(0, 1, H).view(1, H, 1, 1) * 0.3
  x = x + torch.tensor([0.0, 0.03, 0.06]).view(1, 1, 1, 3) + torch.randn((NY * NX, H, W, 3), generator=g) * (3 / 255)
  return x.clamp(0, 1)


def masks(seed):
  """16 one-channel masks: blobs of ones on zeros, as proj_mask is."""
  g = torch.Generator().manual_seed(seed)
  low = torch.rand((NY * NX, 1, H // 32, W // 32), generator=g)
  return (torch.nn.functional.interpolate(low, size=(H, W), mode='bilinear') > 0.5).float().permute(0, 2, 3, 1)


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


def host_ms(fn, repeats):
  times = []
  for _ in range(repeats):
    t = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t) * 1e3)
  return float(np.median(times))


def device_stages(sheets, repeats):
  """The stages of encode_png_batch apart, for uint8 device sheets (H, W, 3)."""
  L = _lib.lib()
  n = len(sheets)
  table = png.encode_table([x.data_ptr() for x in sheets],
                           [(x.shape[0], x.shape[1] * x.shape[2], x.shape[2]) for x in sheets],
                           [png.ADAPTIVE] * n)
  ws_bytes = L.se3ds_png_encode_workspace_bytes(table.ctypes.data, n)
  out_bytes = L.se3ds_png_encode_out_bytes(table.ctypes.data, n)
  head = (8 * n + 15) & ~15
  table_dev = torch.from_numpy(table.reshape(-1)).cuda()
  workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device='cuda')
  result = torch.empty((head + out_bytes,), dtype=torch.uint8, device='cuda')
  host = torch.empty((head + out_bytes,), dtype=torch.uint8, pin_memory=True)

  def launch(phases):
    _lib.check(L.se3ds_png_encode(_lib.ptr(table_dev), table.ctypes.data, n, _lib.ptr(workspace), ws_bytes,
                                  _lib.ptr(result) + head, out_bytes, _lib.ptr(result), phases,
                                  _lib.stream()), 'se3ds_png_encode')

  def download():
    host.copy_(result, non_blocking=True)
    torch.cuda.current_stream().synchronize()

  def container():
    buf = host.numpy()
    sizes = buf[:8 * n].view(np.uint32).reshape(n, 2)
    return [png.png_container(int(r[1]), int(r[2]) // int(r[3]), int(r[3]),
                              b'\x78\x01' + buf[head + int(r[6]):head + int(r[6]) + int(s[0])].tobytes() +
                              struct.pack('>I', int(s[1]))) for r, s in zip(table, sizes)]

  out = {'strips_ms': device_ms(lambda: launch(1), repeats), 'pack_ms': device_ms(lambda: launch(2), repeats),
         'download_ms': host_ms(download, repeats), 'container_ms': host_ms(container, repeats)}
  out['strips'] = int(table[-1, 5]) + -(-int(table[-1, 1]) // png.strip_rows(int(table[-1, 2])))
  out['bytes'] = sum(len(f) for f in container())
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--host-sheets', type=int, default=1, help='sheets the host encoders are timed on')
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'png_encode_bench needs an MI355X'
  rows = {}
  for kind, make, channels in (('panoramas', panoramas, 3), ('masks', masks, 1)):
    floats = [make(s).cuda() for s in range(9)]
    quantise = lambda k: [image_grid.get_grid_image(x, NY * NX, None, out_c=3)[0] for x in floats[:k]]
    for count in (1, 9):
      sheets = quantise(count)
      row = {'quantise_ms': device_ms(lambda: quantise(count), args.repeats)}
      row.update(device_stages(sheets, args.repeats))
      row['end_to_end_ms'] = host_ms(lambda: png.encode_png_batch(sheets), args.repeats)
      row['raw_bytes'] = sum(x.numel() for x in sheets)
      if count == 1:
        pixels = [x.cpu().numpy() for x in sheets[:args.host_sheets]]
        row['host_level6_ms'] = host_ms(lambda: [_encode_png(p) for p in pixels], 1) / len(pixels)
        row['host_rle_ms'] = host_ms(lambda: [png.encode_png_host(p) for p in pixels], 1) / len(pixels)
        row['host_level6_bytes'] = len(_encode_png(pixels[0]))
        row['host_rle_bytes'] = len(png.encode_png_host(pixels[0]))
        decoded = png.decode_png_batch({'x': png.encode_png_batch(sheets[:1])}, 'cuda')['x'][0]
        assert torch.equal(decoded, sheets[0]), 'the device PNG does not decode to its pixels'
      rows[f'{kind} x {count}'] = row
      print(f'{kind} x {count}: ' + ', '.join(f'{k} {v:.2f}' if isinstance(v, float) else f'{k} {v}'
                                              for k, v in row.items()), flush=True)
  print(json.dumps({'png_encode_bench': rows}))


if __name__ == '__main__':
  main()
