"""Point-cloud `.ply` files: the writer behind `SE3DSModel.write_memory_as_pointcloud` (reference
models/models.py:154-178) and a reader for exactly what it writes.

  write_ply(filename, coords, rgb, format='ascii', encoder='host', slab_points=1 << 20)
  read_ply(filename) -> (xyz float32 (M, 3), rgb int32 (M, 3))   host NumPy arrays

Two formats, one header that differs in its format line only: 'ascii' is the reference's file, one
line `x y z r g b \\n` per point; 'binary_little_endian' is 15 bytes per point (float x, y, z; uchar
red, green, blue).  Two encoders:

  'host'    the reference's loop, one str.format per point on the host (the default; ascii only).
            '{}'.format(np.float32(x)) widens to a Python float and prints repr of that binary64:
            np.float32(0.1) is written as 0.10000000149011612.
  'device'  csrc/ply.hip formats the same bytes on the device (csrc/ply_format_core.h has the
            rules), `slab_points` points per call so that the workspace is bounded whatever the size
            of the memory.  Each slab's bytes go to one of two pinned buffers and are written to the
            file while the device formats the next slab.  The file is written as `<filename>.tmp` and
            renamed at the end; on an error the temporary file is removed and nothing is left under
            the final name.  A colour outside [0, 255] cannot be a uchar: the binary format raises
            ValueError (the ascii format prints whatever integer it is given, as the host loop does).

Shapes and dtypes are checked first (ValueError), then the device: encoder='device' raises
`_lib.Se3dsHipError` for a CPU tensor (there is no CPU fallback for the kernels); the host loop copies
its input to the host anyway and takes tensors of any device."""
import os

import numpy as np
import torch

from se3ds_amd import _lib

FORMATS = ('ascii', 'binary_little_endian')
ENCODERS = ('host', 'device')
BINARY_RECORD = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])
MAX_SLAB_POINTS = 1 << 24   # csrc/ply_format_core.h kMaxPoints


def header(points: int, format: str = 'ascii') -> str:
  """The reference's header, character for character (the space in `format ascii 1.0 \\n` included)."""
  if format not in FORMATS:
    raise ValueError(f'format: one of {FORMATS} is needed, got {format!r}')
  return ('ply\nformat %s 1.0 \n' % format + 'element vertex %d\n' % points +
          'property float x\nproperty float y\nproperty float z\n'
          'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')


def _check(coords, rgb, format, encoder, slab_points):
  if format not in FORMATS:
    raise ValueError(f'format: one of {FORMATS} is needed, got {format!r}')
  if encoder not in ENCODERS:
    raise ValueError(f'encoder: one of {ENCODERS} is needed, got {encoder!r}')
  if format != 'ascii' and encoder != 'device':
    raise ValueError(f"format {format!r} is written by encoder='device' only")
  for t, name in ((coords, 'coords'), (rgb, 'rgb')):
    if not isinstance(t, torch.Tensor):
      raise ValueError(f'{name}: a torch tensor is needed, got {type(t).__name__}')
  if coords.dim() != 2 or coords.shape[0] not in (3, 4):
    raise ValueError(f'coords: (3, M) or (4, M) is needed, got {tuple(coords.shape)}')
  if coords.dtype != torch.float32:
    raise ValueError(f'coords: unsupported dtype {coords.dtype} (float32)')
  if rgb.dim() != 2 or rgb.shape[1] != 3 or rgb.shape[0] != coords.shape[1]:
    raise ValueError(f'rgb: ({coords.shape[1]}, 3) is needed, got {tuple(rgb.shape)}')
  if rgb.dtype not in (torch.int32, torch.uint8):
    raise ValueError(f'rgb: unsupported dtype {rgb.dtype} (int32 or uint8)')
  if isinstance(slab_points, bool) or not isinstance(slab_points, int) or not 1 <= slab_points <= MAX_SLAB_POINTS:
    raise ValueError(f'slab_points: an int in [1, {MAX_SLAB_POINTS}] is needed, got {slab_points!r}')


def _write_host(filename, coords, rgb):
  xyz = coords[0:3].cpu().numpy().T
  rgb = rgb.cpu().numpy()
  with open(filename, 'w') as fp:
    fp.write(header(xyz.shape[0]))
    for i in range(xyz.shape[0]):
      fp.write('{} {} {} {} {} {} \n'.format(xyz[i, 0], xyz[i, 1], xyz[i, 2], rgb[i, 0],
                                             rgb[i, 1], rgb[i, 2]))


class _Slabs:
  """Formats slabs of points on the device: launch() queues a slab's kernels, download() queues the
  copy of its bytes into a pinned buffer behind them and returns (buffer, byte count, event), so the
  caller can write slab i to the file while slab i + 1 runs."""

  def __init__(self, coords, rgb, format, slab_points):
    self.coords, self.rgb, self.format = coords, rgb, format
    self.m = coords.shape[1]
    self.slab = min(slab_points, max(self.m, 1))
    self.dev = coords.device
    self.L = _lib.lib()
    self.per_point = self.L.se3ds_ply_max_line_bytes() if format == 'ascii' else BINARY_RECORD.itemsize
    # a dump is rare and its buffers are large: they live for the call, not in a module cache
    self.text = torch.empty((self.slab * self.per_point + 16,), dtype=torch.uint8, device=self.dev)
    ws_bytes = int(self.L.se3ds_ply_ascii_workspace_bytes(self.slab)) if format == 'ascii' else 16
    self.ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=self.dev)
    self.count = torch.zeros((2,), dtype=torch.int64, device=self.dev)   # [0] bytes, [1] flag (low int32)
    self.pinned = [None, None]

  def _pinned(self, k, nbytes):
    if self.pinned[k] is None or self.pinned[k].numel() < nbytes:
      self.pinned[k] = torch.empty((max(nbytes, 1 << 16),), dtype=torch.uint8, pin_memory=True)
    return self.pinned[k]

  def launch(self, first):
    """Queues the kernels of the slab that starts at `first`; returns its number of points."""
    n = min(self.slab, self.m - first)
    L, coords, rgb = self.L, self.coords, self.rgb
    src = coords.data_ptr() + 4 * first
    colours = rgb.data_ptr() + first * 3 * rgb.element_size()
    if self.format == 'ascii':
      _lib.check(L.se3ds_ply_ascii(src, coords.stride(0), colours, _lib.dtype_code(rgb), n, self.text.data_ptr(),
                                   self.text.numel(), self.count.data_ptr(), self.ws.data_ptr(), self.ws.numel(), 7,
                                   _lib.stream()), 'ply_ascii')
    else:
      self.count[1:].zero_()
      _lib.check(L.se3ds_ply_binary(src, coords.stride(0), colours, _lib.dtype_code(rgb), n, self.text.data_ptr(),
                                    self.text.numel(), self.count[1:].data_ptr(), _lib.stream()), 'ply_binary')
    return n

  def download(self, k, n):
    """Waits for the slab's byte count, queues the copy of its bytes into pinned buffer k."""
    if self.format == 'ascii':
      nbytes = int(self.count[0].item())
    else:
      if int(self.count[1].item()) != 0:
        raise ValueError('rgb: a colour outside [0, 255] cannot be written as uchar')
      nbytes = n * BINARY_RECORD.itemsize
    host = self._pinned(k, nbytes)
    host[:nbytes].copy_(self.text[:nbytes], non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    return host, nbytes, event


def _write_device(filename, coords, rgb, format, slab_points):
  m = coords.shape[1]
  tmp = filename + '.tmp'
  f = open(tmp, 'wb')
  try:
    f.write(header(m, format).encode('ascii'))
    if m > 0:
      with torch.cuda.device(coords.device):
        slabs = _Slabs(coords, rgb, format, slab_points)
        pending = None
        for k, first in enumerate(range(0, m, slabs.slab)):
          n = slabs.launch(first)
          if pending is not None:          # the previous slab's bytes go to the file while this one runs
            host, nbytes, event = pending
            event.synchronize()
            f.write(memoryview(host.numpy())[:nbytes])
          pending = slabs.download(k & 1, n)
        host, nbytes, event = pending
        event.synchronize()
        f.write(memoryview(host.numpy())[:nbytes])
    f.flush()
    os.fsync(f.fileno())
    f.close()
    os.replace(tmp, filename)
  except BaseException:
    f.close()
    if os.path.exists(tmp):
      os.remove(tmp)
    raise


def write_ply(filename, coords, rgb, format='ascii', encoder='host', slab_points=1 << 20):
  """Writes the points coords (3 or 4, M) float32 (rows x, y, z; a fourth row is ignored) with the
  colours rgb (M, 3) int32 or uint8 to `filename`; encoder='device' needs both on the device.  A
  non-contiguous input is copied to a contiguous one first (rows of a (4, M) memory are used in
  place)."""
  _check(coords, rgb, format, encoder, slab_points)
  filename = os.fspath(filename)
  if encoder == 'host':
    return _write_host(filename, coords, rgb)
  _lib.require_cuda(coords, rgb)
  if coords.stride(1) != 1 or coords.stride(0) < coords.shape[1]:
    coords = coords.contiguous()
  rgb = rgb.contiguous()
  _write_device(filename, coords, rgb, format, slab_points)


def _parse_header(data: bytes):
  for format in FORMATS:
    head = ('ply\nformat %s 1.0 \nelement vertex ' % format).encode('ascii')
    if not data.startswith(head):
      continue
    end = data.find(b'\n', len(head))
    digits = data[len(head):end] if end > 0 else b''
    if not digits.isdigit():
      break
    full = header(int(digits), format).encode('ascii')
    if data.startswith(full) and full[len(head):].startswith(digits + b'\n'):
      return format, int(digits), len(full)
    break
  raise ValueError('not a .ply header that write_ply writes')


def read_ply(filename):
  """Reads a file that write_ply wrote: (xyz float32 (M, 3), rgb int32 (M, 3)), host NumPy arrays.
  ASCII values go through NumPy's correctly rounded decimal-to-binary64 conversion and a cast to
  float32, which is exact: each text is the shortest binary64 representation of a float32 value.  (A
  NaN comes back as the default quiet NaN: the text `nan` carries neither sign nor payload.)  Any
  other header, a short or a long body raise ValueError."""
  with open(os.fspath(filename), 'rb') as f:
    data = f.read()
  format, m, start = _parse_header(data)
  body = data[start:]
  if format == 'ascii':
    tokens = body.split()
    if len(tokens) != 6 * m or body.count(b'\n') != m:
      raise ValueError(f'{m} lines of six values are expected, got {len(tokens)} values')
    try:
      values = np.array(tokens, dtype='S').astype(np.float64).reshape(m, 6)
    except ValueError as e:
      raise ValueError(f'a value of the body is no number: {e}')
    return values[:, :3].astype(np.float32), values[:, 3:].astype(np.int64).astype(np.int32)
  if len(body) != m * BINARY_RECORD.itemsize:
    raise ValueError(f'{m * BINARY_RECORD.itemsize} bytes of records are expected, got {len(body)}')
  rec = np.frombuffer(body, dtype=BINARY_RECORD)
  xyz = np.stack([rec['x'], rec['y'], rec['z']], axis=1).astype(np.float32) if m else np.zeros((0, 3), np.float32)
  rgb = np.stack([rec['red'], rec['green'], rec['blue']], axis=1).astype(np.int32) if m else np.zeros((0, 3), np.int32)
  return xyz, rgb
