"""Reader / writer of TFRecord files, `tf.train.Example` and `TensorProto`, without TensorFlow --
the container formats of the published R2R data (`train*.tfrecord`, datasets/base_dataset.py:52-77,
datasets/indoor_datasets.py:125-247 and :626-719).  Pure Python and NumPy; the CRC-32C, varint and
protobuf helpers are those of utils/tf_bundle.py.

PARITY UNPINNED: TensorFlow is not installed and no real record ships with the reference, so this
follows the published formats (tensorflow/core/lib/io/record_writer.cc,
tensorflow/core/example/{example,feature}.proto, tensorflow/core/framework/{tensor,tensor_shape,
types}.proto) from their specification; tests/test_tf_records.py pins what can be pinned here:
hand-assembled byte literals, the known-answer Example, writer -> reader round trips.  It stays
unpinned until a real record is at hand.

Formats, as implemented:
  record      uint64 LE length | uint32 LE masked CRC-32C of those 8 bytes | payload |
              uint32 LE masked CRC-32C of the payload
  Example     {1: Features{1: map entry{1: key, 2: Feature}}},
              Feature{1: BytesList{1: bytes...} | 2: FloatList{1: float...} | 3: Int64List{1: int64...}};
              the numeric lists packed (one length-delimited field) or unpacked (one field per value)
  TensorProto {1: dtype, 2: TensorShapeProto{2: Dim{1: size}}, 4: tensor_content}
"""
import os
import struct
from typing import Dict, Iterable, Iterator, List, Tuple, Union

import numpy as np

from se3ds_amd.utils.tf_bundle import (_get_varint, _pb_bytes, _pb_fields, _pb_varint, _put_varint,
                                       crc32c, mask_crc, unmask_crc)

# tensorflow/core/framework/types.proto, the four that datasets/indoor_datasets.py parses
TENSOR_DTYPES = {1: np.float32, 3: np.int32, 4: np.uint8, 9: np.int64}
_TENSOR_CODES = {np.dtype(v): k for k, v in TENSOR_DTYPES.items()}
# TensorProto fields that carry values outside tensor_content
_VALUE_FIELDS = {5: 'float_val', 6: 'double_val', 7: 'int_val', 8: 'string_val', 9: 'scomplex_val',
                 10: 'int64_val', 11: 'bool_val', 12: 'dcomplex_val', 13: 'half_val',
                 14: 'resource_handle_val', 15: 'variant_val', 16: 'uint32_val', 17: 'uint64_val'}


# ------------------------------------------------------------------------------- records
def read_records(path: str, verify: Union[bool, str] = True,
                 device_batch_bytes: int = 64 << 20) -> Iterator[bytes]:
  """The payloads of a TFRecord file, in file order.  A truncated file raises ValueError naming the
  path and the offset of the record; with `verify`, so does a wrong length or payload CRC.

  verify='device': both checksums of every record are computed on the device (utils/crc32c.py)
  instead of by the Python byte loop.  Records are read until `device_batch_bytes` are pending, the
  batch is uploaded once and its 2 ranges per record -- the 8-byte length field and the payload --
  are checked in one call; then the payloads are yielded.  Errors are those of the host path, text
  and offset included, and every record in front of the bad one is yielded first."""
  if isinstance(verify, str):
    if verify != 'device':
      raise ValueError(f"verify {verify!r}: True, False or 'device'")
    yield from _read_records_device(path, int(device_batch_bytes))
    return
  with open(path, 'rb') as f:
    offset = 0
    while True:
      head = f.read(12)
      if not head:
        return
      if len(head) < 12:
        raise ValueError(f'{path}: truncated record header at offset {offset}')
      length, = struct.unpack_from('<Q', head, 0)
      if verify and unmask_crc(struct.unpack_from('<I', head, 8)[0]) != crc32c(head[:8]):
        raise ValueError(f'{path}: length checksum mismatch at offset {offset}')
      body = f.read(length + 4)
      if len(body) < length + 4:
        raise ValueError(f'{path}: truncated record at offset {offset} '
                         f'({len(body)} of {length + 4} bytes)')
      payload = body[:length]
      if verify and unmask_crc(struct.unpack_from('<I', body, length)[0]) != crc32c(payload):
        raise ValueError(f'{path}: payload checksum mismatch at offset {offset}')
      yield payload
      offset += 12 + length + 4


def _read_records_device(path: str, batch_bytes: int) -> Iterator[bytes]:
  """read_records(verify='device').  A record whose length field is damaged cannot be told from a
  sound one before its checksum is known, so the reader never trusts a length beyond the end of the
  file: whatever ends the reading (end of file, a truncation, a length that does not fit) first
  has the pending records checked in file order, and the first bad checksum wins, as it does on
  the host, where it is met first."""
  import torch
  from se3ds_amd.utils import crc32c as crc32c_dev

  pending = []   # (offset, 8 length bytes, stored length crc, payload or None, stored payload crc)

  def flush():
    if not pending:
      return
    parts, offs, lens, pos = [], [], [], 0
    for _, head8, _, payload, _ in pending:
      for piece in (head8,) if payload is None else (head8, payload):
        parts.append(piece)
        offs.append(pos)
        lens.append(len(piece))
        pos += len(piece)
    slab = torch.frombuffer(bytearray(b''.join(parts)), dtype=torch.uint8).cuda()
    crcs = iter(crc32c_dev.crc32c_device(slab, offs, lens).tolist())
    batch = list(pending)
    pending.clear()
    for offset, _, want_len, payload, want_payload in batch:
      if unmask_crc(want_len) != next(crcs):
        raise ValueError(f'{path}: length checksum mismatch at offset {offset}')
      if payload is None:   # the header of a record whose body could not be read
        return
      if unmask_crc(want_payload) != next(crcs):
        raise ValueError(f'{path}: payload checksum mismatch at offset {offset}')
      yield payload

  with open(path, 'rb') as f:
    size = os.fstat(f.fileno()).st_size
    offset = pending_bytes = 0
    while True:
      head = f.read(12)
      if not head:
        yield from flush()
        return
      if len(head) < 12:
        yield from flush()
        raise ValueError(f'{path}: truncated record header at offset {offset}')
      length, = struct.unpack_from('<Q', head, 0)
      want_len, = struct.unpack_from('<I', head, 8)
      left = size - (offset + 12)
      body = f.read(min(length + 4, max(left, 0)))
      if len(body) < length + 4:
        pending.append((offset, head[:8], want_len, None, 0))
        yield from flush()   # raises if the length itself is damaged
        raise ValueError(f'{path}: truncated record at offset {offset} '
                         f'({len(body)} of {length + 4} bytes)')
      pending.append((offset, head[:8], want_len, body[:length], struct.unpack_from('<I', body, length)[0]))
      pending_bytes += 8 + length
      offset += 12 + length + 4
      if pending_bytes >= batch_bytes:
        yield from flush()
        pending_bytes = 0


def frame_record(rec: bytes) -> bytes:
  """One record as it stands in a file: length, its masked CRC-32C, payload, its masked CRC-32C."""
  rec = bytes(rec)
  head = struct.pack('<Q', len(rec))
  return (head + struct.pack('<I', mask_crc(crc32c(head))) + rec +
          struct.pack('<I', mask_crc(crc32c(rec))))


def frame_with_crcs(rec: bytes, length_crc: int, payload_crc: int) -> bytes:
  """frame_record from the raw (unmasked) CRC-32C of the 8 length bytes and of the payload."""
  return (struct.pack('<QI', len(rec), mask_crc(int(length_crc))) + bytes(rec) +
          struct.pack('<I', mask_crc(int(payload_crc))))


def write_records(path: str, records: Iterable[bytes], checksums: str = 'host',
                  slab_bytes: int = 256 << 20, device=None):
  """The inverse of read_records.  checksums='host' (the default): the Python byte loop of
  `frame_record`.  checksums='device': both CRC-32C of every record come from the device
  (`utils.crc32c.crc32c_host_slabs`), for payloads that are made on the host -- an evaluation
  trajectory of `datasets.record_writer.encode_trajectory_example` is some 100 MB; records are
  gathered until `slab_bytes` are pending, then checked in one go and written.  The bytes of the
  file are the same either way.  The file is written as `<path>.tmp` and renamed at the end; on an
  error the temporary file is removed and nothing is left under `path`."""
  if checksums not in ('host', 'device'):
    raise ValueError(f"checksums: 'host' or 'device', got {checksums!r}")
  tmp = path + '.tmp'
  f = open(tmp, 'wb')
  try:
    if checksums == 'host':
      for rec in records:
        f.write(frame_record(rec))
    else:
      from se3ds_amd.utils import crc32c as crc32c_dev

      def flush(pending):
        items = [x for rec in pending for x in (struct.pack('<Q', len(rec)), rec)]
        crcs = crc32c_dev.crc32c_host_slabs(items, slab_bytes=slab_bytes, device=device)
        for i, rec in enumerate(pending):
          f.write(frame_with_crcs(rec, crcs[2 * i], crcs[2 * i + 1]))

      pending, held = [], 0
      for rec in records:
        pending.append(bytes(rec))
        held += len(pending[-1]) + 8
        if held >= slab_bytes:
          flush(pending)
          pending, held = [], 0
      if pending:
        flush(pending)
    f.close()
    os.replace(tmp, path)
  except BaseException:
    f.close()
    if os.path.exists(tmp):
      os.remove(tmp)
    raise


# ------------------------------------------------------------------------------- Example
def _signed64(v: int) -> int:
  return v - (1 << 64) if v >= 1 << 63 else v


def _parse_feature(buf: bytes):
  value = None
  for num, wt, v in _pb_fields(buf):
    if wt != 2:
      raise ValueError(f'Feature field {num}: wire type {wt}')
    if num == 1:
      value = [x for n2, _, x in _pb_fields(v) if n2 == 1]
    elif num == 2:
      out = []
      for n2, wt2, x in _pb_fields(v):
        if n2 != 1:
          continue
        if wt2 == 2:      # packed
          if len(x) % 4:
            raise ValueError('packed float_list of a length that is no multiple of 4')
          out.append(np.frombuffer(x, '<f4'))
        elif wt2 == 5:    # unpacked fixed32
          out.append(np.array([x], '<u4').view('<f4'))
        else:
          raise ValueError(f'float_list value of wire type {wt2}')
      value = (np.concatenate(out) if out else np.zeros((0,), np.float32)).astype(np.float32)
    elif num == 3:
      out = []
      for n2, wt2, x in _pb_fields(v):
        if n2 != 1:
          continue
        if wt2 == 2:      # packed varints
          pos = 0
          while pos < len(x):
            y, pos = _get_varint(x, pos)
            out.append(_signed64(y & 0xffffffffffffffff))
        elif wt2 == 0:
          out.append(_signed64(x & 0xffffffffffffffff))
        else:
          raise ValueError(f'int64_list value of wire type {wt2}')
      value = np.array(out, np.int64)
  return value


def parse_example(buf: bytes) -> Dict[str, Union[List[bytes], np.ndarray]]:
  """{name: value} of a serialized tf.train.Example: list[bytes], float32 array or int64 array.  A
  Feature with no kind set is left out (tf.io.parse_single_example then applies the default)."""
  out = {}
  try:
    for num, wt, features in _pb_fields(buf):
      if num != 1 or wt != 2:
        continue
      for n2, wt2, entry in _pb_fields(features):
        if n2 != 1 or wt2 != 2:
          continue
        key, feature = None, b''
        for n3, _, v in _pb_fields(entry):
          if n3 == 1:
            key = v.decode()
          elif n3 == 2:
            feature = v
        if key is None:
          raise ValueError('Features map entry without a key')
        value = _parse_feature(feature)
        if value is not None:
          out[key] = value
  except (IndexError, struct.error) as e:
    raise ValueError(f'malformed Example: {e}') from None
  return out


def encode_example(features: Dict[str, object]) -> bytes:
  """A serialized tf.train.Example in the form TensorFlow writes: numeric lists packed, entries in
  the order of the dict.  bytes / str / list of bytes -> bytes_list, floating arrays -> float_list,
  integer arrays -> int64_list."""
  entries = b''
  for key, value in features.items():
    if isinstance(value, (bytes, bytearray, str)):
      value = [value]
    if isinstance(value, (list, tuple)) and value and isinstance(value[0], (bytes, bytearray, str)):
      items = [v.encode() if isinstance(v, str) else bytes(v) for v in value]
      feature = _pb_bytes(1, b''.join(_pb_bytes(1, v) for v in items))
    else:
      a = np.asarray(value).reshape(-1)
      if a.dtype.kind == 'f':
        feature = _pb_bytes(2, _pb_bytes(1, a.astype('<f4').tobytes()))
      elif a.dtype.kind in 'iub':
        packed = b''.join(_put_varint(int(x) & 0xffffffffffffffff) for x in a)
        feature = _pb_bytes(3, _pb_bytes(1, packed))
      else:
        raise ValueError(f'{key}: no Feature kind for {a.dtype}')
    entries += _pb_bytes(1, _pb_bytes(1, key.encode()) + _pb_bytes(2, feature))
  return _pb_bytes(1, entries)


# ---------------------------------------------------------------------------- TensorProto
def parse_tensor(buf: bytes, dtype) -> np.ndarray:
  """tf.io.parse_tensor(buf, out_type=dtype) for float32 / int32 / uint8 / int64 tensors stored in
  tensor_content.  NotImplementedError: values outside tensor_content (names the field), another
  dtype, or a dtype that differs from the one asked for."""
  code, shape, content = 0, [], None
  try:
    for num, wt, v in _pb_fields(buf):
      if num == 1:
        code = v
      elif num == 2:
        for n2, _, dim in _pb_fields(v):
          if n2 == 2:
            size = 0
            for n3, _, x in _pb_fields(dim):
              if n3 == 1:
                size = _signed64(x)
            shape.append(size)
          elif n2 == 3 and dim:
            raise ValueError('TensorProto of unknown rank')
      elif num == 4:
        content = v
      elif num in _VALUE_FIELDS:
        raise NotImplementedError(f'TensorProto carries its values in {_VALUE_FIELDS[num]} '
                                  f'(field {num}), not in tensor_content')
  except (IndexError, struct.error) as e:
    raise ValueError(f'malformed TensorProto: {e}') from None
  if code not in TENSOR_DTYPES:
    raise NotImplementedError(f'TensorProto dtype code {code} (supported: float32 = 1, int32 = 3, '
                              'uint8 = 4, int64 = 9)')
  want = np.dtype(dtype)
  have = np.dtype(TENSOR_DTYPES[code])
  if want != have:
    raise NotImplementedError(f'TensorProto holds {have}, {want} was asked for')
  if any(d < 0 for d in shape):
    raise ValueError(f'TensorProto shape {shape}')
  count = int(np.prod(shape, dtype=np.int64)) if shape else 1
  content = b'' if content is None else content
  if len(content) != count * have.itemsize:
    raise ValueError(f'tensor_content of {len(content)} bytes for {have} {tuple(shape)}')
  return np.frombuffer(content, have.newbyteorder('<')).astype(have).reshape(shape)


def serialize_tensor(array) -> bytes:
  """tf.io.serialize_tensor for the four dtypes parse_tensor reads."""
  a = np.asarray(array)
  if a.dtype not in _TENSOR_CODES:
    raise NotImplementedError(f'no TensorProto dtype code for {a.dtype} here')
  dims = b''.join(_pb_bytes(2, _pb_varint(1, int(d))) for d in a.shape)
  raw = np.ascontiguousarray(a).astype(a.dtype.newbyteorder('<'), copy=False).tobytes()
  return _pb_varint(1, _TENSOR_CODES[a.dtype]) + _pb_bytes(2, dims) + _pb_bytes(4, raw)


# ------------------------------------------------------------------- parse_single_example
class FixedLenFeature:
  """tf.io.FixedLenFeature: kind 'string' / 'int64' / 'float32'; default_value None = required."""
  _REQUIRED = object()

  def __init__(self, shape, dtype: str, default_value=_REQUIRED):
    if dtype not in ('string', 'int64', 'float32'):
      raise ValueError(f'FixedLenFeature dtype {dtype}')
    self.shape = tuple(shape)
    self.dtype = dtype
    self.default_value = default_value

  @property
  def required(self):
    return self.default_value is FixedLenFeature._REQUIRED


def _matches(value, dtype: str) -> bool:
  if dtype == 'string':
    return isinstance(value, list)
  return isinstance(value, np.ndarray) and value.dtype == (np.int64 if dtype == 'int64' else np.float32)


def apply_features(parsed: Dict[str, object], spec: Dict[str, FixedLenFeature]) -> Dict[str, object]:
  """tf.io.parse_single_example's FixedLenFeature handling over a parse_example result: a missing
  feature takes its default (ValueError if it has none), and so does a present one whose list is
  empty, which TensorFlow treats as missing; any other must hold exactly prod(shape) values of the
  spec's kind.  `[]` yields a scalar (bytes, int or float32)."""
  out = {}
  for name, f in spec.items():
    count = int(np.prod(f.shape, dtype=np.int64)) if f.shape else 1
    value = parsed.get(name)
    if value is None or len(value) == 0:
      if f.required:
        raise ValueError(f'feature {name} is required but missing')
      value = f.default_value
      if f.dtype == 'string':
        value = [v.encode() if isinstance(v, str) else v
                 for v in (value if isinstance(value, (list, tuple)) else [value])]
      else:
        value = np.asarray(value, np.int64 if f.dtype == 'int64' else np.float32).reshape(-1)
    elif not _matches(value, f.dtype):
      raise ValueError(f'feature {name}: expected {f.dtype}')
    if len(value) != count:
      raise ValueError(f'feature {name}: {len(value)} values, shape {list(f.shape)} holds {count}')
    if f.dtype == 'string':
      out[name] = value[0] if not f.shape else np.array(value, dtype=object).reshape(f.shape)
    elif not f.shape:
      out[name] = value[0].item() if f.dtype == 'int64' else np.float32(value[0])
    else:
      out[name] = value.reshape(f.shape)
  return out
