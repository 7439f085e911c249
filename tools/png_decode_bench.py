"""The PNG decode of one training batch: 8 examples x the seven planes of R2RImageDataset._parse at
512 x 1024 (two 8-bit RGB, two 16-bit grey, three 8-bit grey: 56 PNGs), synthesised here from a
seed.  Every row's filter type is chosen as an encoder's heuristic does (the type with the least
sum of absolute signed residuals); on the RGB planes (shading, object edges, a little sensor
noise) that is Paeth for most rows, then Up and Sub; the histogram is part of the result.

Reported, each named for what it is:
  inflate   host milliseconds of parse_png (chunk walk, CRC, zlib inflate, filter-type check) per
            plane on ONE thread, per plane kind; and the wall time of the whole batch on a pool of
            1 / 2 / 4 / 8 / 16 threads (zlib releases the GIL), from which panoramas/s follow
  upload    the one pinned host-to-device copy of the table + all filtered streams (device events)
  kernel    se3ds_png_unfilter over the 56 planes already resident (device events over many
            launches after warm-up), and the whole decode_png_batch call from PngPlanes (host clock
            around a device synchronise)
The decoded planes are compared with the synthesised pixels before anything is timed.

--inflate device | both adds the same batch with the inflate on the device (`se3ds_png_inflate`):
  device_inflate_kernel_ms   the inflate launch over the 56 compressed streams already resident
  device_unfilter_kernel_ms  the reconstruction behind it, from the inflate's workspace
  device_upload_mib / _ms    the one pinned copy of both tables + the COMPRESSED streams
  decode_png_batch_device_ms the whole decode_png_batch(inflate='device') call from PngStreams
--inflate host (the default) reports what the tool always did; `both` is the comparison DESIGN.md
section 3.8 asks for: device_inflate_kernel_ms against inflate_pool[4].batch_ms on one machine.

  python tools/png_decode_bench.py [--inflate host|device|both] [--iters 50] [--rounds 3] [--out FILE.json]
"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.datasets import indoor_datasets  # noqa: E402
from se3ds_amd.utils import png  # noqa: E402

H, W, BATCH = 512, 1024, 8


def heuristic_filter(raw: np.ndarray, bpp: int):
  """uint8 (H, row_bytes) -> (filtered stream, per-row types): all five candidates per row, the one
  with the least sum of |signed residual| wins (the usual encoder heuristic).  Vectorised: filtering
  only reads the unfiltered neighbours."""
  x = raw.astype(np.int16)
  a = np.zeros_like(x)
  a[:, bpp:] = x[:, :-bpp]
  b = np.zeros_like(x)
  b[1:] = x[:-1]
  c = np.zeros_like(x)
  c[1:, bpp:] = x[:-1, :-bpp]
  p = a + b - c
  pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
  paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
  cands = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)
  cost = np.abs(cands.view(np.int8).astype(np.int32)).sum(axis=2)
  types = cost.argmin(axis=0).astype(np.uint8)
  rows = cands[types, np.arange(raw.shape[0])]
  return np.concatenate([types[:, None], rows], axis=1).tobytes(), types


def synth_example(rng):
  """Pixel arrays of one example: smooth shading + block edges + slight noise (RGB), smooth ramps
  (depth), blocky masks and labels."""
  yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
  out = {}
  for k in ('image', 'proj_image'):
    base = [127 + 100 * np.sin(xx / rng.uniform(40, 200) + ch) * np.cos(yy / rng.uniform(40, 200))
            for ch in range(3)]
    edges = np.kron(rng.integers(-40, 40, (H // 16, W // 32)), np.ones((16, 32)))[..., None]
    noise = rng.normal(0, 0.4, (H, W, 3))
    out[k] = np.clip(np.stack(base, -1) + edges + noise, 0, 255).astype(np.uint8)
  for k in ('depth', 'proj_depth'):
    d = 20000 + 15000 * np.sin(xx / rng.uniform(100, 300)) * np.sin(yy / rng.uniform(80, 200))
    out[k] = np.clip(d + rng.normal(0, 40, (H, W)), 0, 65535).astype(np.uint16)
  blocks = rng.integers(0, 42, (H // 32, W // 32), dtype=np.uint8)
  out['segmentation'] = np.kron(blocks, np.ones((32, 32), np.uint8))
  out['proj_mask'] = (np.kron(rng.integers(0, 4, (H // 16, W // 16), dtype=np.uint8),
                              np.ones((16, 16), np.uint8)) > 0).astype(np.uint8) * np.uint8(255)
  out['blurred_mask'] = (np.kron(rng.integers(0, 20, (H // 64, W // 64), dtype=np.uint8),
                                 np.ones((64, 64), np.uint8)) == 0).astype(np.uint8)
  out['proj_image'] = out['proj_image'] * (out['proj_mask'][..., None] > 0)
  out['proj_depth'] = out['proj_depth'] * (out['proj_mask'] > 0)
  return out


def encode(pixels: np.ndarray):
  import struct
  import zlib
  depth = 16 if pixels.dtype == np.uint16 else 8
  colour = 2 if pixels.ndim == 3 else 0
  bpp = (3 if colour == 2 else 1) * depth // 8
  raw = (pixels.astype('>u2').view(np.uint8) if depth == 16 else pixels).reshape(H, -1)
  stream, types = heuristic_filter(raw, bpp)

  def chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data))
  buf = (png.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, colour, 0, 0, 0)) +
         chunk(b'IDAT', zlib.compress(stream, 6)) + chunk(b'IEND', b''))
  return buf, types


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
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default=None)
  ap.add_argument('--inflate', choices=('host', 'device', 'both'), default='host')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('png_decode_bench needs an MI355X: a CPU run cannot give a time')
  dev = torch.device('cuda:0')
  rng = np.random.default_rng(1)
  keys = list(indoor_datasets.RAW_DTYPES)
  pixels = [synth_example(rng) for _ in range(BATCH)]
  encoded, hist = {k: [] for k in keys}, {k: np.zeros(5, np.int64) for k in keys}
  for ex in pixels:
    for k in keys:
      buf, types = encode(ex[k])
      encoded[k].append(buf)
      hist[k] += np.bincount(types, minlength=5)
  res = dict(batch=BATCH, height=H, width=W, planes=BATCH * len(keys),
             encoded_mib=sum(len(b) for v in encoded.values() for b in v) / 2 ** 20,
             filter_type_rows={k: hist[k].tolist() for k in keys})

  # ---- correctness first
  got = png.decode_png_batch(encoded, dev)
  torch.cuda.synchronize()
  for k in keys:
    want = np.stack([ex[k] for ex in pixels])
    g = got[k].cpu().numpy()
    g = g.view(np.uint16) if g.dtype == np.int16 else g
    if not (g == want).all():
      raise SystemExit(f'{k}: decoded planes differ from the synthesised pixels')
  res['equal_to_source'] = True
  res['inflate'] = a.inflate
  if a.inflate in ('device', 'both'):
    device_inflate(a, res, dev, keys, encoded, got)
  if a.inflate in ('host', 'both'):
    host_inflate(a, res, dev, keys, encoded, pixels)
  line = json.dumps(res)
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(line + '\n')


def device_inflate(a, res, dev, keys, encoded, want):
  """The batch with the inflate on the device; `want`: the host path's decode of the same PNGs."""
  got = png.decode_png_batch(encoded, dev, inflate='device')
  for k in keys:
    if not torch.equal(got[k], want[k]):
      raise SystemExit(f"{k}: inflate='device' differs from inflate='host'")
  streams = [png.parse_png_container(b) for k in keys for b in encoded[k]]
  L = _lib.lib()
  n = len(streams)
  itab = np.zeros((n, L.se3ds_png_inflate_fields()), np.int64)
  utab = np.zeros((n, L.se3ds_png_unfilter_fields()), np.int64)
  offset = (itab.nbytes + utab.nbytes + 15) & ~15
  ws, outs = 0, []
  for i, p in enumerate(streams):
    inflated = p.height * (1 + p.row_bytes)
    outs.append(torch.empty(p.height * p.row_bytes, dtype=torch.uint8, device=dev))
    itab[i] = (offset, len(p.compressed), ws, inflated, 1 + p.row_bytes)
    utab[i] = (ws, outs[-1].data_ptr(), p.height, p.row_bytes, p.bytes_per_pixel, int(p.bit_depth == 16))
    offset += (len(p.compressed) + 15) & ~15
    ws += (inflated + 15) & ~15
  staging = torch.empty((offset,), dtype=torch.uint8, pin_memory=True)
  host = staging.numpy()
  host[:itab.nbytes] = itab.reshape(-1).view(np.uint8)
  host[itab.nbytes:itab.nbytes + utab.nbytes] = utab.reshape(-1).view(np.uint8)
  for row, p in zip(itab, streams):
    host[row[0]:row[0] + row[1]] = np.frombuffer(p.compressed, np.uint8)
  dbuf = torch.empty((offset,), dtype=torch.uint8, device=dev)
  workspace = torch.empty((ws,), dtype=torch.uint8, device=dev)
  status = torch.empty((n,), dtype=torch.int32, device=dev)
  upload = lambda: dbuf.copy_(staging, non_blocking=True)
  inflate = lambda: _lib.check(L.se3ds_png_inflate(dbuf.data_ptr(), offset, workspace.data_ptr(), ws,
                                                   itab.ctypes.data, n, status.data_ptr(), _lib.stream()),
                               'se3ds_png_inflate')
  unfilter = lambda: _lib.check(L.se3ds_png_unfilter(workspace.data_ptr(), ws, dbuf.data_ptr() + itab.nbytes,
                                                     utab.ctypes.data, n, _lib.stream()),
                                'se3ds_png_unfilter')
  for _ in range(2):
    upload()
    inflate()
    unfilter()
  torch.cuda.synchronize()
  if status.any():
    raise SystemExit(f'device inflate status words: {status.tolist()}')
  iters = max(1, a.iters // 5)   # the inflate is the long kernel of this tool
  res['device_upload_mib'] = offset / 2 ** 20
  res['device_upload_ms'] = [time_ms(upload, a.iters) for _ in range(a.rounds)]
  res['device_inflate_kernel_ms'] = [time_ms(inflate, iters) for _ in range(a.rounds)]
  res['device_unfilter_kernel_ms'] = [time_ms(unfilter, a.iters) for _ in range(a.rounds)]
  by_key = {k: streams[i * BATCH:(i + 1) * BATCH] for i, k in enumerate(keys)}
  whole = []
  for _ in range(a.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
      png.decode_png_batch(by_key, dev, inflate='device')
    whole.append((time.perf_counter() - t0) * 200)
  res['decode_png_batch_device_ms'] = whole


def host_inflate(a, res, dev, keys, encoded, pixels):
  # ---- inflate: one thread per plane kind, then the batch on pools
  per_plane = {}
  for k in keys:
    t0 = time.perf_counter()
    for _ in range(a.rounds):
      for buf in encoded[k]:
        png.parse_png(buf)
    per_plane[k] = (time.perf_counter() - t0) * 1e3 / (a.rounds * BATCH)
  res['inflate_ms_per_plane_one_thread'] = per_plane
  res['inflate_ms_per_example_one_thread'] = sum(per_plane.values())
  flat = [b for k in keys for b in encoded[k]]
  pools = {}
  for threads in (1, 2, 4, 8, 16):
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
      list(pool.map(png.parse_png, flat))   # warm
      best = 1e30
      for _ in range(a.rounds):
        t0 = time.perf_counter()
        planes = list(pool.map(png.parse_png, flat))
        best = min(best, time.perf_counter() - t0)
    pools[threads] = dict(batch_ms=best * 1e3, panoramas_per_s=BATCH / best)
  res['inflate_pool'] = pools

  # ---- upload and kernel, apart
  by_key = {k: planes[i * BATCH:(i + 1) * BATCH] for i, k in enumerate(keys)}
  L = _lib.lib()
  table = np.zeros((len(planes), L.se3ds_png_unfilter_fields()), np.int64)
  offset = (table.nbytes + 15) & ~15
  outs = []
  for i, p in enumerate(planes):
    outs.append(torch.empty(p.height * p.row_bytes, dtype=torch.uint8, device=dev))
    table[i] = (offset, outs[-1].data_ptr(), p.height, p.row_bytes, p.bytes_per_pixel,
                int(p.bit_depth == 16))
    offset += (len(p.filtered) + 15) & ~15
  staging = torch.empty((offset,), dtype=torch.uint8, pin_memory=True)
  host = staging.numpy()
  host[:table.nbytes] = table.reshape(-1).view(np.uint8)
  for row, p in zip(table, planes):
    host[row[0]:row[0] + len(p.filtered)] = np.frombuffer(p.filtered, np.uint8)
  dbuf = torch.empty((offset,), dtype=torch.uint8, device=dev)
  upload = lambda: dbuf.copy_(staging, non_blocking=True)
  kernel = lambda: _lib.check(L.se3ds_png_unfilter(dbuf.data_ptr(), offset, dbuf.data_ptr(),
                                                   table.ctypes.data, len(planes), _lib.stream()),
                              'se3ds_png_unfilter')
  for _ in range(3):
    upload()
    kernel()
  torch.cuda.synchronize()
  res['upload_mib'] = offset / 2 ** 20
  res['upload_ms'] = [time_ms(upload, a.iters) for _ in range(a.rounds)]
  res['kernel_ms'] = [time_ms(kernel, a.iters) for _ in range(a.rounds)]
  for i, p in enumerate(planes):   # the timed launches still compute the right thing
    k = keys[i // BATCH]
    want = pixels[i % BATCH][k]
    g = outs[i].cpu().numpy()
    g = g.view(np.uint16) if p.bit_depth == 16 else g
    if not (g.reshape(want.shape) == want).all():
      raise SystemExit(f'{k}: timed launch differs from the synthesised pixels')
  whole = []
  for _ in range(a.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
      png.decode_png_batch(by_key, dev)
    torch.cuda.synchronize()
    whole.append((time.perf_counter() - t0) * 100)
  res['decode_png_batch_from_planes_ms'] = whole


if __name__ == '__main__':
  main()
