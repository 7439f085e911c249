"""Throughput of the device CRC-32C (se3ds_crc32c_multi, csrc/crc32c.hip) on three inputs:

  one      one range of 256 MiB
  blocks   4096 ranges of 64 KiB
  records  a TFRecord-like mix: 8-byte length fields and payloads of 100 KB - 2 MB at the offsets a
           file gives them (arbitrary alignment), 64 MiB in total

For each: a few ranges are checked against `tf_bundle.crc32c` first (the host loop, on at most 64 KiB
each).  Then the two launches of one call are timed with device events after warm-up -- the table
and the workspace are on the device beforehand, as they are when a caller reuses them -- over
`--iters` calls per window and `--rounds` windows; the median window and the spread are reported, as
GB/s and as the fraction of the HBM read roofline (`--hbm-gbs`, 8000 for the MI355X).  The buffers
are far larger than the caches, so every call reads its bytes from HBM.  The same bytes are also
uploaded from pinned host memory with `--iters` copies per window: verification hides under the copy
if its time is below the upload's.  Next to them: the ~5 MB/s host loop it replaces, timed on 1 MiB.

  python tools/crc32c_bench.py [--rounds 5] [--iters 20] [--hbm-gbs 8000] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.utils import crc32c as C  # noqa: E402
from se3ds_amd.utils import tf_bundle  # noqa: E402

DEV = torch.device('cuda:0')


def time_ms(fn, iters):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / iters


def inputs():
  mib = 1 << 20
  yield 'one', 256 * mib, [0], [256 * mib]
  yield 'blocks', 256 * mib, [i * 65536 for i in range(4096)], [65536] * 4096
  rng = np.random.default_rng(0)
  offs, lens, pos = [], [], 0
  while pos < 64 * mib:
    n = int(rng.integers(100_000, 2_000_001))
    offs += [pos, pos + 12]
    lens += [8, n]
    pos += 12 + n + 4
  yield 'records', pos, offs, lens


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--hbm-gbs', type=float, default=8000.0, help='HBM read roofline in GB/s')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('crc32c_bench needs an MI355X: a CPU run cannot give a time')
  L = _lib.lib()
  stream = torch.cuda.current_stream().cuda_stream
  sample = np.random.default_rng(1).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
  t0 = time.perf_counter()
  tf_bundle.crc32c(sample)
  host_mbs = 1.0 / (time.perf_counter() - t0) * (len(sample) / 1e6)
  results = []
  for name, size, offs, lens in inputs():
    g = torch.Generator(device=DEV).manual_seed(3)
    buf = torch.randint(0, 256, (size,), dtype=torch.uint8, device=DEV, generator=g)
    # exactness first, on ranges short enough for the host loop
    picks = [i for i, n in enumerate(lens) if n <= 65536][:4] or [0]
    check_offs = [offs[i] for i in picks] + [offs[-1] + max(lens[-1] - 50000, 0)]
    check_lens = [min(lens[i], 65536) for i in picks] + [min(lens[-1], 50000)]
    got = C.crc32c_device(buf, check_offs, check_lens).tolist()
    for o, n, c in zip(check_offs, check_lens, got):
      assert tf_bundle.crc32c(buf[o:o + n].cpu().numpy().tobytes()) == c, (name, o, n)
    table = C.build_table(offs, lens)
    n = table.shape[0]
    table_dev = torch.from_numpy(table).to(DEV)
    crc = torch.empty((n,), dtype=torch.int32, device=DEV)
    ws = torch.empty((int(L.se3ds_crc32c_workspace_bytes(int(sum(lens)), n)),), dtype=torch.uint8, device=DEV)

    def call():
      _lib.check(L.se3ds_crc32c_multi(buf.data_ptr(), size, table_dev.data_ptr(), table.ctypes.data, n,
                                      crc.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'crc32c_multi')
    pinned = torch.empty((size,), dtype=torch.uint8).pin_memory()
    pinned.copy_(buf)
    dst = torch.empty_like(buf)
    upload = lambda: dst.copy_(pinned, non_blocking=True)
    for _ in range(3):
      call()
      upload()
    torch.cuda.synchronize()
    first = crc.clone()
    kernel, copy = [], []
    for _ in range(a.rounds):   # alternating, in one process
      kernel.append(time_ms(call, a.iters))
      copy.append(time_ms(upload, a.iters))
    assert torch.equal(crc, first)   # deterministic
    nbytes = float(sum(lens))
    k_ms, c_ms = statistics.median(kernel), statistics.median(copy)
    results.append(dict(input=name, ranges=n, bytes=int(nbytes), crc_ms=round(k_ms, 4),
                        crc_ms_min_max=[round(min(kernel), 4), round(max(kernel), 4)],
                        crc_gbs=round(nbytes / k_ms / 1e6, 1),
                        hbm_fraction=round(nbytes / k_ms / 1e6 / a.hbm_gbs, 4),
                        upload_ms=round(c_ms, 4), upload_gbs=round(size / c_ms / 1e6, 1),
                        crc_over_upload=round(k_ms / c_ms, 4)))
    del buf, dst, pinned
  out = dict(tool='crc32c_bench', block_bytes=L.se3ds_crc32c_block_bytes(), rounds=a.rounds, iters=a.iters,
             hbm_gbs=a.hbm_gbs, host_loop_mbs=round(host_mbs, 2), results=results)
  line = json.dumps(out)
  print(line)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
