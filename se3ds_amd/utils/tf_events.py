"""Writer / reader of TensorBoard event files without TensorFlow: what tf.summary.create_file_writer,
tf.summary.scalar and tf.summary.image leave on disk for the reference's utils/logger.py.  An event
file is a TFRecord file (utils/tf_records.py frames it, masked CRC-32C included) of serialized
`Event` messages.

PARITY UNPINNED: TensorBoard is not installed, so this follows the published definitions
(tensorflow/core/util/event.proto, tensorflow/core/framework/summary.proto) from their text, and
tests/test_png_encode_cpu.py pins what can be pinned here: a decoder written from the field numbers,
writer -> reader round trips, the record framing.  It stays unpinned until a real TensorBoard reads
a file.

Messages, as written:
  Event          {1: wall_time (double), 2: step (int64), 3: file_version (string) | 5: summary}
  Summary        {1: value (repeated Value)}
  Value          {1: tag (string), 2: simple_value (float) | 4: image (Summary.Image)}
  Summary.Image  {1: height, 2: width, 3: colorspace (channels), 4: encoded_image_string (the PNG)}
The first record of a file is an Event with file_version "brain.Event:2"; every summary call
writes one Event with one Value.  The simple_value / Summary.Image forms are the ones TensorBoard
reads directly."""
import os
import socket
import struct
import time
from typing import Dict, Iterator, Tuple, Union

from se3ds_amd.utils import tf_records
from se3ds_amd.utils.tf_bundle import _pb_bytes, _pb_fields, _pb_varint, _put_varint

FILE_VERSION = 'brain.Event:2'


def _pb_double(num: int, v: float) -> bytes:
  return _put_varint((num << 3) | 1) + struct.pack('<d', v)


def _pb_float(num: int, v: float) -> bytes:
  return _put_varint((num << 3) | 5) + struct.pack('<f', v)


def encode_event(wall_time: float, step: int = 0, file_version: str = None, value: bytes = None) -> bytes:
  """A serialized Event; `value` is a serialized Summary.Value."""
  out = _pb_double(1, float(wall_time))
  if step:
    out += _pb_varint(2, int(step))
  if file_version is not None:
    out += _pb_bytes(3, file_version.encode())
  if value is not None:
    out += _pb_bytes(5, _pb_bytes(1, value))
  return out


def scalar_value(tag: str, value: float) -> bytes:
  return _pb_bytes(1, tag.encode()) + _pb_float(2, float(value))


def image_value(tag: str, png_bytes: bytes, height: int, width: int, channels: int) -> bytes:
  image = (_pb_varint(1, int(height)) + _pb_varint(2, int(width)) + _pb_varint(3, int(channels)) +
           _pb_bytes(4, bytes(png_bytes)))
  return _pb_bytes(1, tag.encode()) + _pb_bytes(4, image)


class EventFileWriter:
  """events.out.tfevents.<10-digit seconds>.<hostname> under `logdir` (created if missing); the
  version record is written at once.  Not thread-safe; records reach the file on flush / close."""

  def __init__(self, logdir: str):
    os.makedirs(logdir, exist_ok=True)
    now = time.time()
    self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), socket.gethostname()))
    self._file = open(self.path, 'ab')
    self._write(encode_event(now, file_version=FILE_VERSION))
    self.flush()

  def _write(self, event: bytes):
    if self._file is None:
      raise ValueError(f'{self.path} is closed')
    self._file.write(tf_records.frame_record(event))

  def add_scalar(self, tag: str, value: float, step: int):
    self._write(encode_event(time.time(), step, value=scalar_value(tag, value)))

  def add_image(self, tag: str, png_bytes: bytes, height: int, width: int, step: int,
                channels: int = None):
    """channels (Summary.Image.colorspace): read from the PNG's IHDR when not given."""
    if channels is None:
      channels = 3 if bytes(png_bytes[25:26]) == b'\x02' else 1
    self._write(encode_event(time.time(), step, value=image_value(tag, png_bytes, height, width, channels)))

  def flush(self):
    if self._file is not None:
      self._file.flush()

  def close(self):
    if self._file is not None:
      self._file.close()
      self._file = None


def _signed64(v: int) -> int:
  return v - (1 << 64) if v >= 1 << 63 else v


def decode_event(buf: bytes) -> Tuple[float, int, str, Dict[str, Union[float, Tuple[int, int, bytes]]]]:
  """-> wall_time, step, file_version ('' if none), {tag: float | (height, width, png)}."""
  wall_time, step, version, values = 0.0, 0, '', {}
  for num, wt, v in _pb_fields(buf):
    if num == 1 and wt == 1:
      wall_time, = struct.unpack('<d', struct.pack('<Q', v))
    elif num == 2 and wt == 0:
      step = _signed64(v)
    elif num == 3 and wt == 2:
      version = v.decode()
    elif num == 5 and wt == 2:
      for n2, wt2, value in _pb_fields(v):
        if n2 != 1 or wt2 != 2:
          continue
        tag, content = '', None
        for n3, wt3, x in _pb_fields(value):
          if n3 == 1 and wt3 == 2:
            tag = x.decode()
          elif n3 == 2 and wt3 == 5:
            content, = struct.unpack('<f', struct.pack('<I', x))
          elif n3 == 4 and wt3 == 2:
            image = {n4: x4 for n4, _, x4 in _pb_fields(x)}
            content = (image.get(1, 0), image.get(2, 0), image.get(4, b''))
        if content is not None:
          values[tag] = content
  return wall_time, step, version, values


def read_events(path: str) -> Iterator[Tuple[float, int, Dict[str, Union[float, Tuple[int, int, bytes]]]]]:
  """(wall_time, step, {tag: float | (height, width, png)}) per record of an event file, the
  version record (an empty dict) included; record checksums are verified.  ValueError if the file
  does not begin with the version record."""
  for i, rec in enumerate(tf_records.read_records(path, verify=True)):
    wall_time, step, version, values = decode_event(rec)
    if i == 0 and version != FILE_VERSION:
      raise ValueError(f'{path}: the first record is not the {FILE_VERSION} version record')
    yield wall_time, step, values
