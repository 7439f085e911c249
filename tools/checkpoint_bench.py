"""What a checkpoint costs the training step: GANManager.save_checkpoint (state_dict() + np.savez, the
yardstick) against GANManager.save_checkpoint_async on the same model, machine and directory
(DESIGN.md section 3.12).  One JSON line:

  sync_save_s        wall time of save_checkpoint, between device synchronisations
  async_stall_ms     what the training stream waits for in the async save, between HIP events on that
                     stream: the snapshot copy ('device'; also as a fraction of the HBM copy roofline,
                     2 x bytes moved) or the wait for the last device-to-host copy ('direct')
  async_call_s       how long the host is inside save_checkpoint_async
  async_total_s      from the call until the file is in place
  crc_gbs            se3ds_crc32z_multi over all member ranges of the snapshot, device events, and its
                     fraction of the HBM read roofline
  d2h_gbs            one staging slab, device to pinned host memory, device events
  file_write_gbs     the slab written to --dir as often as the checkpoint is large, fsync included
  step_ms_idle / step_ms_writing   train_g_d with no save in flight / while the writer runs

The first save of each kind is a warm-up (allocations, code objects); medians of --rounds follow.  The
async file is then read back and compared with the synchronous one, array by array.

  python tools/checkpoint_bench.py --gen-dims 32 --image-size 256 --dir /tmp/ckpt [--snapshot device]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from se3ds_amd import _lib, bench_step  # noqa: E402
from se3ds_amd.trainers import async_checkpoint  # noqa: E402
from se3ds_amd.utils import crc32c as C  # noqa: E402
from se3ds_amd.utils import npz_writer  # noqa: E402

DEV = torch.device('cuda:0')


def events_ms(fn, iters):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / iters


def wall_s(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return time.perf_counter() - t0


def med(xs, digits=4):
  return round(statistics.median(xs), digits) if xs else None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gen-dims', type=int, default=128)
  ap.add_argument('--image-size', type=int, default=512)
  ap.add_argument('--batch', type=int, default=8)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  ap.add_argument('--dir', required=True)
  ap.add_argument('--snapshot', default='device', choices=['device', 'direct'])
  ap.add_argument('--staging-bytes', type=int, default=2 * (256 << 20))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--steps', type=int, default=10, help='train_g_d steps per timed window')
  ap.add_argument('--hbm-gbs', type=float, default=8000.0, help='HBM roofline in GB/s')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('checkpoint_bench needs an MI355X: a CPU run cannot give a time')
  os.makedirs(a.dir, exist_ok=True)
  gan = bench_step.build_gan(types.SimpleNamespace(
      image_size=a.image_size, dtype=a.dtype,
      gin_bindings=[f'image_models.ResNetGenerator.gen_dims = {a.gen_dims}']), DEV, 1)
  batch = bench_step.synth_batch(a.batch, a.image_size, 1234, DEV)
  arenas, _ = async_checkpoint.arena_members(gan)
  state_bytes = sum(4 * n for _, rows in arenas for _, _, n, _ in rows)
  out = dict(tool='checkpoint_bench', gen_dims=a.gen_dims, image_size=a.image_size, batch=a.batch,
             dtype=a.dtype, snapshot=a.snapshot, staging_bytes=a.staging_bytes, rounds=a.rounds,
             hbm_gbs=a.hbm_gbs, state_bytes=state_bytes, members=sum(len(rows) for _, rows in arenas) + 3)

  def step():
    gan.train_g_d(batch)
    gan.global_step += 1

  for _ in range(3):
    step()
  torch.cuda.synchronize()
  sync_path, async_path = os.path.join(a.dir, 'bench-sync.npz'), os.path.join(a.dir, 'bench-async.npz')

  # ---- the yardstick, then the async save, alternating
  sync_s, stall_ms, call_s, total_s = [], [], [], []
  for r in range(a.rounds + 1):   # round 0 warms up
    s = wall_s(lambda: gan.save_checkpoint(sync_path))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    handle = gan.save_checkpoint_async(async_path, snapshot=a.snapshot, staging_bytes=a.staging_bytes)
    t1 = time.perf_counter()
    handle.wait()
    t2 = time.perf_counter()
    torch.cuda.synchronize()
    if r:
      sync_s.append(s)
      stall_ms.append(handle.stall_events[0].elapsed_time(handle.stall_events[1]))
      call_s.append(t1 - t0)
      total_s.append(t2 - t0)
    if r < a.rounds:
      os.remove(async_path)   # the directory never holds more than two checkpoints, a .tmp included
  out.update(sync_save_s=med(sync_s), sync_save_s_all=[round(x, 4) for x in sync_s],
             async_stall_ms=med(stall_ms), async_stall_ms_all=[round(x, 4) for x in stall_ms],
             async_call_s=med(call_s), async_total_s=med(total_s), async_total_s_all=[round(x, 4) for x in total_s],
             file_bytes=os.path.getsize(async_path))
  out['stall_over_sync_save'] = round(statistics.median(stall_ms) / 1e3 / statistics.median(sync_s), 6)
  if a.snapshot == 'device':
    out['snapshot_copy_hbm_fraction'] = round(2 * state_bytes / statistics.median(stall_ms) / 1e6 / a.hbm_gbs, 4)

  # ---- same contents (the state has not changed between the two saves of the last round)
  with np.load(sync_path) as want, np.load(async_path) as got:
    assert sorted(want.files) == sorted(got.files)
    for k in want.files:
      x, y = want[k], got[k]   # np.load checks the CRC-32 the device computed
      assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
  out['async_equals_sync'] = True
  os.remove(sync_path)

  # ---- the CRC call alone, over the members as the save lays them out
  ck = gan._checkpointer
  if a.snapshot == 'device':
    buf, base, offs, lens = ck.snapshot, 0, [], []
    for arena, rows in arenas:
      offs += [base + 4 * o for _, o, _, _ in rows]
      lens += [4 * n for _, _, n, _ in rows]
      base = async_checkpoint._align(base + 4 * arena.numel())
  else:
    arena, rows = max(arenas, key=lambda ar: ar[0].numel())
    buf = arena.detach().view(torch.uint8)
    offs, lens = [4 * o for _, o, _, _ in rows], [4 * n for _, _, n, _ in rows]
  seeds = [zlib.crc32(npz_writer.npy_header((n // 4,), np.float32)) for n in lens]
  table = C.build_table(offs, lens, seeds)
  L, n = _lib.lib(), table.shape[0]
  table_dev = torch.from_numpy(table).to(DEV)
  crc = torch.empty((n,), dtype=torch.int32, device=DEV)
  ws = torch.empty((int(L.se3ds_crc32z_workspace_bytes(int(sum(lens)), n)),), dtype=torch.uint8, device=DEV)
  stream = torch.cuda.current_stream().cuda_stream

  def crc_call():
    _lib.check(L.se3ds_crc32z_multi(buf.data_ptr(), buf.numel(), table_dev.data_ptr(), table.ctypes.data, n,
                                    crc.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'crc32z_multi')
  for _ in range(3):
    crc_call()
  crc_ms = [events_ms(crc_call, 5) for _ in range(a.rounds)]
  k = int(np.argmax(lens))   # exactness of the largest member against zlib, once
  assert int(crc[k].item()) & 0xffffffff == zlib.crc32(buf[offs[k]:offs[k] + lens[k]].cpu().numpy().tobytes(), seeds[k])
  crc_bytes = float(sum(lens))
  out.update(crc_ranges=n, crc_bytes=int(crc_bytes), crc_ms=med(crc_ms),
             crc_gbs=round(crc_bytes / statistics.median(crc_ms) / 1e6, 1),
             crc_hbm_fraction=round(crc_bytes / statistics.median(crc_ms) / 1e6 / a.hbm_gbs, 4))

  # ---- one slab device -> pinned host, and the slab to the directory
  slab = ck.slabs[0]
  nslab = min(slab.numel(), buf.numel())
  d2h = lambda: slab[:nslab].copy_(buf[:nslab], non_blocking=True)
  for _ in range(2):
    d2h()
  d2h_ms = [events_ms(d2h, 3) for _ in range(a.rounds)]
  out['d2h_gbs'] = round(nslab / statistics.median(d2h_ms) / 1e6, 2)
  view, scratch = memoryview(slab.numpy())[:nslab], os.path.join(a.dir, 'bench-write.bin')
  write_s = []
  for _ in range(a.rounds):
    t0 = time.perf_counter()
    with open(scratch, 'wb') as f:
      for _ in range(max(state_bytes // nslab, 1)):
        f.write(view)
      f.flush()
      os.fsync(f.fileno())
    write_s.append(time.perf_counter() - t0)
  out['file_write_gbs'] = round(max(state_bytes // nslab, 1) * nslab / statistics.median(write_s) / 1e9, 3)
  os.remove(scratch)

  # ---- the step with the writer idle and with it running
  idle, writing, steps_per_save = [], [], []
  for _ in range(a.rounds):
    idle.append(wall_s(lambda: [(step(), torch.cuda.synchronize()) for _ in range(a.steps)]) * 1e3 / a.steps)
    torch.cuda.synchronize()
    t0, made = time.perf_counter(), 0
    handle = gan.save_checkpoint_async(async_path, snapshot=a.snapshot, staging_bytes=a.staging_bytes)
    while not handle.done or made == 0:   # whole steps that start while the writer runs
      step()
      torch.cuda.synchronize()
      made += 1
    writing.append((time.perf_counter() - t0) * 1e3 / made)
    steps_per_save.append(made)
    handle.wait()
  out.update(step_ms_idle=med(idle, 3), step_ms_writing=med(writing, 3), steps_per_save=steps_per_save)
  for p in (sync_path, async_path):
    if os.path.exists(p):
      os.remove(p)
  gan.wait_for_checkpoint()
  line = json.dumps(out)
  print(line)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
