"""Checkpoints written off the training step (GANManager.save_checkpoint_async).

The file is the .npz of `GANManager.save_checkpoint` -- the keys and arrays of `state_dict()` -- but
nothing of it passes through `state_dict()`: every variable and every optimiser slot is a contiguous
fp32 range of one of the ten arenas (theta and state of generator, discriminator and EMA generator,
m and v of the two optimisers), so

  training stream   snapshot='device': the ten arenas are copied back to back (16-byte aligned) into
                    one snapshot allocation, kept between saves.  That copy is all the step waits for.
                    snapshot='direct': nothing is copied; the side stream reads the live arenas and
                    the training stream waits for the last device-to-host copy instead.
  side stream       one se3ds_crc32z_multi call per source buffer over all member ranges, seeded
                    with the zlib.crc32 of each member's .npy header, n uint32 read back; then the
                    source goes to two pinned staging slabs in alternation, one event per slab.
  writer thread     the one background thread of a save: it issues the side stream's work, waits for
                    a slab's event, hands the slab to utils/npz_writer (the bytes are only ever
                    passed to write()) and refills it.

Host memory in flight is the two slabs.  An exception in the thread is kept in the handle and raised
by wait()."""
import threading
import zlib

import numpy as np
import torch

from se3ds_amd.utils import crc32c as crc_dev
from se3ds_amd.utils import npz_writer

ALIGN = 16


class CheckpointHandle:
  """What save_checkpoint_async returns.  done: the file is in place or the save has failed;
  wait(): blocks until then and raises what the writer raised."""

  def __init__(self, path):
    self.path = path
    self.error = None
    self.stall_events = None   # (start, end) HIP events on the training stream around what it waits for
    self._thread = None
    self._copies_issued = threading.Event()

  @property
  def done(self):
    return self._thread is None or not self._thread.is_alive()

  def wait(self):
    if self._thread is not None:
      self._thread.join()
    if self.error is not None:
      raise self.error
    return self.path


def _align(n):
  return (n + ALIGN - 1) // ALIGN * ALIGN


def arena_members(manager):
  """[(arena tensor, [(key, element offset, elements, shape)])] for the ten arenas, members in offset
  order, and the host members [(key, int64 0-d array)]: together the keys of state_dict()."""
  arenas = []
  for prefix, model in (('generator', manager.generator), ('discriminator', manager.discriminator),
                        ('ema_generator', manager.ema_generator)):
    st = model.store
    for which, arena in (('theta', st.theta), ('state', st.state)):
      rows = sorted((o, n, f'{prefix}/{name}') for name, (w, o, n) in st.offsets.items() if w == which)
      arenas.append((arena, [(key, o, n, tuple(st.views[key[len(prefix) + 1:]].shape)) for o, n, key in rows]))
  for prefix, opt in (('g_optimizer', manager.g_optimizer), ('d_optimizer', manager.d_optimizer)):
    st = opt.model.store
    rows = sorted((o, n, name, tuple(shape)) for name, (o, n, shape) in st._off_tr.items())
    for slot, arena in (('m', opt.m), ('v', opt.v)):
      arenas.append((arena, [(f'{prefix}/{name}/{slot}', o, n, shape) for o, n, name, shape in rows]))
  host = [('global_step', np.asarray(manager.global_step, np.int64)),
          ('g_optimizer/iter', np.asarray(manager.g_optimizer.iterations, np.int64)),
          ('d_optimizer/iter', np.asarray(manager.d_optimizer.iterations, np.int64))]
  return arenas, host


class AsyncCheckpointer:
  """The snapshot allocation, the staging slabs and the side stream of one GANManager, kept between
  saves, and the save in flight."""

  def __init__(self, manager):
    self.manager = manager
    self.device = manager.strategy.device
    self.side = torch.cuda.Stream(self.device)
    self.snapshot = None
    self.slabs = None
    self.inflight = None

  def wait(self):
    handle, self.inflight = self.inflight, None
    if handle is not None:
      handle.wait()

  def save(self, path, snapshot='device', staging_bytes=2 * (256 << 20), writer_hook=None, after=None):
    if snapshot not in ('device', 'direct'):
      raise ValueError(f"snapshot: 'device' or 'direct', got {snapshot!r}")
    slab_bytes = int(staging_bytes) // 2 // ALIGN * ALIGN
    if slab_bytes < ALIGN:
      raise ValueError(f'staging_bytes {staging_bytes}: two slabs of at least {ALIGN} bytes')
    self.wait()   # one save at a time: the snapshot and the slabs are its own; raises its failure
    arenas, host = arena_members(self.manager)
    handle = CheckpointHandle(path)
    train = torch.cuda.current_stream(self.device)
    start, ready = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # sources: [(uint8 device buffer, [(key, byte offset, bytes, shape)])]
    if snapshot == 'device':
      bases, total = [], 0
      for arena, _ in arenas:
        bases.append(total)
        total = _align(total + 4 * arena.numel())
      if self.snapshot is None or self.snapshot.numel() != total:
        self.snapshot = torch.empty((total,), dtype=torch.uint8, device=self.device)
      start.record(train)
      for base, (arena, _) in zip(bases, arenas):
        self.snapshot[base:base + 4 * arena.numel()].copy_(arena.detach().view(torch.uint8))
      ready.record(train)
      handle.stall_events = (start, ready)
      sources = [(self.snapshot, [(key, base + 4 * o, 4 * n, shape)
                                  for base, (_, rows) in zip(bases, arenas) for key, o, n, shape in rows])]
    else:
      ready.record(train)
      sources = [(arena.detach().view(torch.uint8), [(key, 4 * o, 4 * n, shape) for key, o, n, shape in rows])
                 for arena, rows in arenas]
    if self.slabs is None or self.slabs[0].numel() != slab_bytes:
      self.slabs = [torch.empty((slab_bytes,), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    handle._thread = threading.Thread(
        target=self._run, args=(handle, sources, host, ready, slab_bytes, writer_hook, after),
        name='se3ds-checkpoint-writer', daemon=True)
    handle._thread.start()
    self.inflight = handle
    if snapshot == 'direct':   # the step may not change what the side stream still reads
      handle._copies_issued.wait()
      start.record(train)
      train.wait_stream(self.side)   # ends with the last device-to-host copy
      end = torch.cuda.Event(enable_timing=True)
      end.record(train)
      handle.stall_events = (start, end)
    return handle

  # ------------------------------------------------------------------------- the writer thread
  def _run(self, handle, sources, host, ready, slab_bytes, writer_hook, after):
    try:
      torch.cuda.set_device(self.device)
      self.side.wait_event(ready)
      # the plan: slab k holds bytes [lo, hi) of source s; a member is a list of pieces of slabs
      plan, members = [], []
      for s, (buf, rows) in enumerate(sources):
        first = len(plan)
        for lo in range(0, buf.numel(), slab_bytes):
          plan.append((s, lo, min(lo + slab_bytes, buf.numel())))
        headers = [npz_writer.npy_header(shape, np.float32) for _, _, _, shape in rows]
        crcs = crc_dev.crc32z_device(buf, [b for _, b, _, _ in rows], [n for _, _, n, _ in rows],
                                     [zlib.crc32(h) for h in headers], stream=self.side) if rows else []
        for (key, b, n, _), header, crc in zip(rows, headers, crcs):
          pieces = []
          while n > 0:
            k = first + b // slab_bytes
            take = min(n, plan[k][2] - b)
            pieces.append((k, b - plan[k][1], take))
            b, n = b + take, n - take
          members.append((key + '.npy', header, pieces, int(crc)))
      slabs = [t.numpy() for t in self.slabs]
      events = [torch.cuda.Event(), torch.cuda.Event()]
      state = dict(issued=0, current=-1)

      def issue():
        k = state['issued']
        if k < len(plan):
          s, lo, hi = plan[k]
          with torch.cuda.stream(self.side):
            self.slabs[k % 2][:hi - lo].copy_(sources[s][0][lo:hi], non_blocking=True)
            events[k % 2].record(self.side)
        state['issued'] = k + 1
        if state['issued'] >= len(plan):
          handle._copies_issued.set()

      def chunks(pieces):
        for k, off, n in pieces:
          while state['current'] < k:   # hand the consumed slab back, take the next
            if state['current'] >= 0:
              issue()
            state['current'] += 1
            events[state['current'] % 2].synchronize()
            if writer_hook is not None:
              writer_hook()
          yield memoryview(slabs[k % 2])[off:off + n]

      issue(), issue()

      def all_members():
        for key, value in host:
          yield npz_writer.array_member(key, value)
        for name, header, pieces, crc in members:
          yield name, header, chunks(pieces), crc

      npz_writer.write_npz(handle.path, all_members())
      if after is not None:
        after()
    except BaseException as e:   # kept for wait(), the next save and the end of train
      handle.error = e
    finally:
      handle._copies_issued.set()
      self.side.synchronize()
