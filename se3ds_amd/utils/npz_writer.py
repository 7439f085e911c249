"""A stored-zip `.npz` writer that takes every member's CRC-32 as given.

`np.savez` and `zipfile` always run zlib's CRC-32 over the data on one CPU.  A checkpoint written
from `GANManager.save_checkpoint_async` already has the checksum of every member from the device
(`utils/crc32c.crc32z_device`), so the container is written by hand: per member a local file header,
the `.npy` header and the raw little-endian data (method 0, stored; no data descriptor, every CRC is
known before its member is written), then the central directory and the end record.  ZIP64 extra
fields and the ZIP64 end record / locator appear whenever a size, an offset or the member count needs
them, or always with `force_zip64=True` (both paths are then testable at a few kilobytes).

The writer streams: members are handed over as (name, npy header, iterator of byte chunks, crc) in
file order, and nothing is kept but the directory entries.  It writes `<path>.tmp`, fsyncs and
`os.replace`s, so a reader never sees a partial file; on an exception the temporary file is removed
and `<path>` is left as it was.  `np.load` checks every member's CRC when it reads it
(`BadZipFile: Bad CRC-32`), which makes it an independent check of the checksums given.

Pure host code: no device, no thread, no process."""
import io
import os
import struct
import zlib

import numpy as np

_U16, _U32 = 0xffff, 0xffffffff
_DATE, _TIME = (1 << 5) | 1, 0   # 1980-01-01 00:00:00: files of equal contents are equal


def npy_header(shape, dtype) -> bytes:
  """The version 1.0 `.npy` header (magic included) that this NumPy writes for a C-contiguous array
  of `shape` and `dtype`, without allocating it."""
  probe = np.broadcast_to(np.zeros((), dtype), tuple(shape))   # zero strides: no memory
  d = np.lib.format.header_data_from_array_1_0(probe)
  d['fortran_order'] = False
  f = io.BytesIO()
  np.lib.format.write_array_header_1_0(f, d)
  return f.getvalue()


def _data_bytes(header: bytes) -> int:
  f = io.BytesIO(header)
  if np.lib.format.read_magic(f) != (1, 0):
    raise ValueError('a version 1.0 .npy header is expected')
  shape, _, dtype = np.lib.format.read_array_header_1_0(f)
  if f.read(1):
    raise ValueError('bytes behind the .npy header')
  if dtype.hasobject:
    raise ValueError('object arrays have no raw data')
  return int(np.prod(shape, dtype=np.int64)) * dtype.itemsize


def array_member(key, array):
  """(name, npy header, chunks, crc) of a host array, checksummed with zlib: the small host members
  of a checkpoint, and what the tests compare the given-CRC path against."""
  a = np.ascontiguousarray(array)
  if a.dtype.byteorder == '>':
    a = a.astype(a.dtype.newbyteorder('<'))
  header = npy_header(np.shape(array), a.dtype)
  data = a.tobytes()
  return key + '.npy', header, (data,), zlib.crc32(data, zlib.crc32(header))


def _zip64_extra(*values):
  return struct.pack('<HH', 1, 8 * len(values)) + b''.join(struct.pack('<Q', v) for v in values)


def write_npz(path, members, force_zip64=False):
  """Writes `path` from an iterable of (name, npy header, iterator of byte chunks, crc): crc is
  zlib.crc32 of the header followed by the data, the chunks (bytes-like, any sizes) add up to the
  data size the header states.  Returns the number of bytes written."""
  path = os.fspath(path)
  tmp = path + '.tmp'
  entries = []   # (name bytes, crc, size, offset, zip64)
  f = open(tmp, 'wb')
  try:
    pos = 0
    for name, header, chunks, crc in members:
      raw_name = name.encode('utf-8')
      flags = 0 if raw_name.isascii() else 0x800
      size = len(header) + _data_bytes(header)
      big = force_zip64 or size >= _U32
      extra = _zip64_extra(size, size) if big else b''
      f.write(struct.pack('<IHHHHHIIIHH', 0x04034b50, 45 if big else 20, flags, 0, _TIME, _DATE,
                          int(crc) & _U32, _U32 if big else size, _U32 if big else size,
                          len(raw_name), len(extra)) + raw_name + extra + header)
      written = len(header)
      for chunk in chunks:
        view = memoryview(chunk).cast('B')
        written += view.nbytes
        if written > size:
          break
        f.write(view)
      if written != size:
        raise ValueError(f'{name}: {written} bytes handed over, the header states {size}')
      entries.append((raw_name, flags, int(crc) & _U32, size, pos, big))
      pos += 30 + len(raw_name) + len(extra) + size
    cd_offset = pos
    for raw_name, flags, crc, size, offset, big in entries:
      far = force_zip64 or offset >= _U32
      values = ([size, size] if big else []) + ([offset] if far else [])
      extra = _zip64_extra(*values) if values else b''
      f.write(struct.pack('<IHHHHHHIIIHHHHHII', 0x02014b50, 45 if values else 20, 45 if values else 20,
                          flags, 0, _TIME, _DATE, crc, _U32 if big else size, _U32 if big else size,
                          len(raw_name), len(extra), 0, 0, 0, 0, _U32 if far else offset) + raw_name + extra)
      pos += 46 + len(raw_name) + len(extra)
    cd_size, n = pos - cd_offset, len(entries)
    if force_zip64 or n >= _U16 or cd_size >= _U32 or cd_offset >= _U32:
      f.write(struct.pack('<IQHHIIQQQQ', 0x06064b50, 44, 45, 45, 0, 0, n, n, cd_size, cd_offset))
      f.write(struct.pack('<IIQI', 0x07064b50, 0, pos, 1))
      pos += 56 + 20
      n, cd_size, cd_offset = _U16, _U32, _U32
    f.write(struct.pack('<IHHHHIIH', 0x06054b50, 0, 0, n, n, cd_size, cd_offset, 0))
    pos += 22
    f.flush()
    os.fsync(f.fileno())
    f.close()
    os.replace(tmp, path)
    return pos
  except BaseException:
    f.close()
    if os.path.exists(tmp):
      os.remove(tmp)
    raise


def write_bytes_atomic(path, data) -> None:
  """`data` to `path` the way write_npz lands its file: `<path>.tmp`, fsync, `os.replace`; on an
  exception the temporary file is removed."""
  tmp = path + '.tmp'
  try:
    with open(tmp, 'wb') as f:
      f.write(data)
      f.flush()
      os.fsync(f.fileno())
    os.replace(tmp, path)
  except BaseException:
    if os.path.exists(tmp):
      os.remove(tmp)
    raise


def savez(path, arrays, force_zip64=False):
  """`np.savez(path, **arrays)` through this writer, checksums from zlib: the same member names and
  arrays."""
  return write_npz(path, (array_member(k, v) for k, v in arrays.items()), force_zip64=force_zip64)
