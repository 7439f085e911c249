"""The host half the device codecs share (utils/png.py, utils/jpeg.py, datasets/record_writer.py,
utils/crc32c.py): descriptor tables and payloads packed at 16-byte-aligned offsets into one pinned
buffer and copied up once, so that the kernels address `base + offset`; the check that the target
is a device; the read-back of status words or results behind an event.  The alignment rule lives
here and nowhere else: the kernels load and store 16 bytes a lane from these offsets."""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from se3ds_amd import _lib


def aligned(n: int) -> int:
  """n rounded up to a multiple of 16."""
  return (n + 15) & ~15


def layout(sizes: Sequence[int], start: int = 0) -> Tuple[List[int], int]:
  """-> (offsets, total): part i of `sizes[i]` bytes lies at the next 16-byte boundary at or behind
  `start` and the parts before it; total, the end of the last part, is aligned as well.  A part of
  no bytes takes the offset of the part behind it."""
  offsets, at = [], aligned(start)
  for size in sizes:
    offsets.append(at)
    at = aligned(at + int(size))
  return offsets, at


def cuda_device(device, who: str, does: str = 'computes') -> torch.device:
  """`device` (None: the current one) as a torch.device with its index filled in; Se3dsHipError
  naming the caller `who` and what it `does` if it is no device."""
  dev = torch.device('cuda' if device is None else device)
  if dev.type != 'cuda':
    raise _lib.Se3dsHipError(f'{who} {does} on an MI355X (cuda) device; got {dev}.  '
                             'There is no CPU fallback.')
  return dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())


def upload(parts, dev) -> Tuple[torch.Tensor, List[int]]:
  """C-contiguous NumPy arrays or bytes-like objects -> (uint8 device tensor, the offset of every
  part in it, as `layout` of their sizes gives them): one pinned buffer, one asynchronous copy on
  the current stream of `dev`.  A caller whose tables hold these offsets takes them from `layout`
  first.  The padding between the parts is left as the allocator gave it."""
  views = [p.reshape(-1).view(np.uint8) if isinstance(p, np.ndarray) else np.frombuffer(p, np.uint8)
           for p in parts]
  offsets, total = layout([v.size for v in views])
  with torch.cuda.device(dev):
    staging = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    for at, v in zip(offsets, views):
      host[at:at + v.size] = v
    # The copy, and the kernels the caller queues behind it, are on the current stream; the caching
    # allocators (pinned and device) hand a freed block out again only behind that work.
    return staging.to(dev, non_blocking=True), offsets


class Readback:
  """A device tensor on its way to a pinned host tensor, on the current stream of its device, with
  an event behind the copy: `wait()` synchronises with that event alone and returns the NumPy view."""

  def __init__(self, src: torch.Tensor):
    with torch.cuda.device(src.device):
      self._host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
      self._host.copy_(src, non_blocking=True)
      self._event = torch.cuda.Event()
      self._event.record()

  def wait(self) -> np.ndarray:
    self._event.synchronize()
    return self._host.numpy()
