"""CRC-32C on the device (csrc/crc32c.hip): the checksum of TFRecord frames (utils/tf_records.py) and
of checkpoint-bundle tensors (utils/tf_bundle.py) at memory speed instead of the ~5 MB/s of the
Python byte loop `tf_bundle.crc32c`, which stays the yardstick of the tests.

  crc32c_device(buf, offsets, lengths)   raw CRCs of many byte ranges of one device buffer, one call
  crc32c_host_slabs(items)               the same for host buffers: packed into bounded slabs, one
                                         upload and one call per slab
  crc32z_device(buf, offsets, lengths, seeds)   the zip / zlib CRC-32 (`zlib.crc32(range, seed)`) of
                                         many ranges, one call: the members of a checkpoint archive
                                         (trainers/gan_manager.py save_checkpoint_async)

Values are the raw (unmasked) CRC, as `tf_bundle.crc32c` returns it.  There is no host fallback: a
buffer that is not on the device raises."""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd.utils._staging import cuda_device

SLAB_ALIGN = 16   # items start on 16-byte boundaries of their slab

_workspaces = {}   # (device index, stream) -> uint8 tensor


def build_table(offsets, lengths, seeds=None) -> np.ndarray:
  """The int64 [n][2] table (byte offset, length) of `se3ds_crc32c_multi`, from two equally long
  sequences; with `seeds` the [n][3] table (byte offset, length, seed) of `se3ds_crc32z_multi`.  Pure
  host code; the ranges themselves are validated against the buffer by the library."""
  off = np.asarray(offsets, dtype=np.int64).reshape(-1)
  length = np.asarray(lengths, dtype=np.int64).reshape(-1)
  if off.shape != length.shape:
    raise ValueError(f'{off.shape[0]} offsets for {length.shape[0]} lengths')
  cols = [off, length]
  if seeds is not None:
    seed = np.asarray(seeds).reshape(-1)
    if seed.shape != off.shape:
      raise ValueError(f'{seed.shape[0]} seeds for {off.shape[0]} offsets')
    if seed.size and (int(seed.min()) < 0 or int(seed.max()) > 0xffffffff):
      raise ValueError('a seed is a CRC: 0 .. 2**32 - 1')
    cols.append(seed.astype(np.int64))
  return np.ascontiguousarray(np.stack(cols, axis=1))


def _workspace(dev, stream_handle, nbytes):
  key = (dev.index, stream_handle)
  ws = _workspaces.get(key)
  if ws is None or ws.numel() < nbytes:
    ws = torch.empty((max(int(nbytes), 4096),), dtype=torch.uint8, device=dev)
    _workspaces[key] = ws
  return ws


def crc32c_device(buf: torch.Tensor, offsets, lengths, stream=None) -> np.ndarray:
  """uint32 [n]: the CRC-32C of buf[offsets[i] : offsets[i] + lengths[i]] for every i, computed on
  the device in one call.  `buf` is a contiguous device torch.uint8 tensor; offsets and lengths need
  no alignment, ranges may overlap, length 0 gives 0.  stream: a torch.cuda.Stream (default: the
  current one).  Reads the result back, which waits for that stream."""
  return _device('crc32c', buf, build_table(offsets, lengths), stream)


def crc32z_device(buf: torch.Tensor, offsets, lengths, seeds=None, stream=None) -> np.ndarray:
  """uint32 [n]: `zlib.crc32(buf[offsets[i] : offsets[i] + lengths[i]], seeds[i])` for every i -- the
  zip CRC-32, continued from the CRC of a prefix the host has already hashed -- computed on the
  device in one call.  seeds None: all 0, the plain CRC-32.  A length 0 gives its seed.  Otherwise
  the contract of `crc32c_device`."""
  table = build_table(offsets, lengths, np.zeros(np.size(offsets), np.int64) if seeds is None else seeds)
  return _device('crc32z', buf, table, stream)


def _device(kind, buf, table, stream):
  _lib.require_cuda(buf)
  if buf.dtype != torch.uint8 or not buf.is_contiguous():
    raise ValueError(f'{kind}_device takes a contiguous torch.uint8 tensor')
  n = table.shape[0]
  if n == 0:
    return np.zeros((0,), np.uint32)
  nbytes = int(buf.numel())
  if nbytes == 0:   # nothing to read: only empty ranges are possible
    if table[:, :2].any():
      raise _lib.Se3dsHipError(f'{kind}_device: a range leaves the empty buffer')
    return table[:, 2].astype(np.uint32) if table.shape[1] == 3 else np.zeros((n,), np.uint32)
  L = _lib.lib()
  multi, workspace_bytes = getattr(L, f'se3ds_{kind}_multi'), getattr(L, f'se3ds_{kind}_workspace_bytes')
  with torch.cuda.device(buf.device), torch.cuda.stream(stream if stream is not None
                                                         else torch.cuda.current_stream(buf.device)):
    handle = torch.cuda.current_stream().cuda_stream
    table_dev = torch.from_numpy(table).to(buf.device)
    crc = torch.empty((n,), dtype=torch.int32, device=buf.device)
    ws_bytes = int(workspace_bytes(int(table[:, 1].sum()), n))
    ws = _workspace(buf.device, handle, ws_bytes)
    _lib.check(multi(buf.data_ptr(), nbytes, table_dev.data_ptr(), table.ctypes.data, n, crc.data_ptr(),
                     ws.data_ptr(), ws.numel(), handle), f'{kind}_multi')
    out = crc.cpu().numpy()
  return out.view(np.uint32)


def _as_bytes(item) -> np.ndarray:
  if isinstance(item, np.ndarray):
    a = np.ascontiguousarray(item).reshape(-1)
    return a.view(np.uint8)
  return np.frombuffer(item, dtype=np.uint8)


def pack_slabs(sizes: Sequence[int], slab_bytes: int) -> List[Tuple[List[int], List[int], int]]:
  """Plans the slabs of `crc32c_host_slabs`: [(item indices, their byte offsets in the slab, slab
  size)], items in input order, every item on a SLAB_ALIGN boundary.  A slab ends before the item
  that would take it beyond `slab_bytes`; an item larger than that is a slab of its own.  Pure host."""
  if slab_bytes < 1:
    raise ValueError(f'slab_bytes {slab_bytes}')
  slabs, idx, offs, used = [], [], [], 0
  for i, size in enumerate(sizes):
    size = int(size)
    start = (used + SLAB_ALIGN - 1) // SLAB_ALIGN * SLAB_ALIGN
    if idx and start + size > slab_bytes:
      slabs.append((idx, offs, used))
      idx, offs, start = [], [], 0
    idx.append(i)
    offs.append(start)
    used = start + size
  if idx:
    slabs.append((idx, offs, used))
  return slabs


def crc32c_host_slabs(items, slab_bytes: int = 256 << 20, device=None) -> np.ndarray:
  """uint32 [len(items)]: the CRC-32C of every item's bytes (bytes-like objects or NumPy arrays, the
  latter as they lie in memory), in input order.  The items are packed into slabs of at most
  `slab_bytes`, each uploaded once and checked with one device call, so the host memory in flight is
  one slab whatever the total."""
  dev = cuda_device(device, 'crc32c_host_slabs')
  views = [_as_bytes(x) for x in items]
  out = np.zeros((len(views),), np.uint32)
  for idx, offs, used in pack_slabs([v.size for v in views], slab_bytes):
    if used == 0:
      continue
    if len(idx) == 1:
      slab = views[idx[0]]
    else:
      slab = np.zeros((used,), np.uint8)
      for i, o in zip(idx, offs):
        slab[o:o + views[i].size] = views[i]
    buf = torch.from_numpy(slab if slab.flags.writeable else slab.copy()).to(dev)
    out[idx] = crc32c_device(buf, offs, [views[i].size for i in idx])
  return out
