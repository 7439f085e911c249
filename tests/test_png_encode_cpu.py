"""The device PNG encoder and the TensorBoard writer without a GPU: csrc/deflate_core.h as a
stand-alone host program (tools/deflate_host_check.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer against CPython's zlib, the Adler-32 combine, the host-side rejection of
bad tables, the NumPy encoder, the event file format and the logger.  The kernels run in
tests/test_png_encode_gpu.py."""
import os
import re
import socket
import struct
import zlib

import numpy as np
import pytest

import _png_encode_ref as R
import _png_ref
from se3ds_amd import _lib
from se3ds_amd.utils import logger as logger_lib
from se3ds_amd.utils import png, tf_events, tf_records


def _fibonacci_histogram():
  """20 symbols with the Fibonacci counts 1, 2, 3, 5, ...; the end-of-block symbol is the sequence's
  other 1, so an unlimited Huffman code is a chain 20 bits deep."""
  fib = [1, 2]
  while len(fib) < 20:
    fib.append(fib[-1] + fib[-2])
  grouped = np.concatenate([np.full(c, 3 * i + 1, np.uint8) for i, c in enumerate(reversed(fib))])
  data = np.empty_like(grouped)   # even places first, then odd ones: no byte repeats its neighbour,
  half = (len(grouped) + 1) // 2  # so there are no runs and the block holds literals only
  data[0::2], data[1::2] = grouped[:half], grouped[half:]
  assert not np.any(data[1:] == data[:-1])
  return data.tobytes()


def _literal_code_lengths(stream):
  """The literal/length code lengths of a stream that starts with a dynamic block in the encoder's
  form (RFC 1951 3.2.7 with the fixed code-length code: symbol s is the 4-bit code word s)."""
  bits = np.unpackbits(np.frombuffer(stream, np.uint8), bitorder='little')
  assert list(bits[1:3]) == [0, 1], 'not a dynamic block'
  field = lambda at, n: int(sum(int(b) << i for i, b in enumerate(bits[at:at + n])))
  nlit, ndist, nclen = field(3, 5) + 257, field(8, 5) + 1, field(13, 4) + 4
  assert (ndist, nclen) == (1, 19)
  clen = [field(17 + 3 * i, 3) for i in range(19)]
  assert clen == [0, 0, 0] + [4] * 16
  at = 17 + 57
  lens = [int(sum(int(b) << (3 - i) for i, b in enumerate(bits[at + 4 * k:at + 4 * k + 4])))
          for k in range(nlit + 1)]
  assert lens[-1] == 1   # the one distance code
  return lens[:-1]


def test_encoder_core_as_a_sanitised_host_program(tmp_path):
  """Built with AddressSanitizer + UndefinedBehaviorSanitizer (reports are fatal, the runtimes
  linked statically, nothing loaded into Python) the core must turn every corpus entry into a
  stream that zlib inflates to exactly the input, with the input's Adler-32, within the bound."""
  exe = R.build_host_program(tmp_path, sanitize=True)
  rng = np.random.default_rng(0)
  noise = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
  fib = _fibonacci_histogram()
  strips = {
      'empty': b'', 'one byte': b'\x07', 'all values once': bytes(range(256)), 'fibonacci': fib,
      'single distinct literal': b'\x05' * 40, 'noise': noise,
      'run to the strip end': bytes(rng.integers(0, 256, 500, dtype=np.uint8)) + b'\xee' * 300,
      'not final': (b'xy' * 10 + b'\0' * 9, False),
  }
  for n in (2, 3, 258, 259, 260, 261, 262, 517, 65535):
    strips[f'repeat {n}'] = b'\x09' * n
  ramp = ((np.arange(64)[None, :, None] * 3 + np.arange(40)[:, None, None] +
           rng.integers(0, 4, (40, 64, 3))) % 256).astype(np.uint8)
  images = {f'ramp mode {m}': (ramp, m) for m in range(6)}
  images['grey adaptive'] = (ramp[:, :, :1].copy(), R.ADAPTIVE)
  images['two strips'] = (rng.integers(0, 8, (70, 341, 3)).astype(np.uint8), R.ADAPTIVE)   # 63 rows a strip
  images['one pixel'] = (np.array([[[200]]], np.uint8), R.ADAPTIVE)
  cases = {**strips, **images}
  results = dict(zip(cases, R.run_host_program(exe, list(cases.values()), tmp_path)))
  for name, case in cases.items():
    stream, s1, s2 = results[name]
    if name in images:
      filtered = R.filter_rows(*case)[1]
      data, final = filtered.tobytes(), True
      bound = sum(R.OVERHEAD + len(s) for s in R.strips_of(filtered, filtered.shape[1] - 1))
    else:
      data, final = case if isinstance(case, tuple) else (case, True)
      bound = R.OVERHEAD + len(data)
    assert len(stream) <= bound, name
    adler = zlib.adler32(data)
    assert (s2 << 16) | s1 == adler, name
    assert stream[-4:] == b'\x00\x00\xff\xff', name   # the empty stored block: byte-aligned end
    if not final:   # no BFINAL yet: the stream goes on
      partial = zlib.decompressobj()
      assert partial.decompress(b'\x78\x01' + stream) == data and not partial.eof, name
      stream += b'\x01\x00\x00\xff\xff'
    assert zlib.decompress(b'\x78\x01' + stream + struct.pack('>I', adler)) == data, name
  # incompressible: one stored block, exactly at the bound
  assert len(results['noise'][0]) == 65535 + R.OVERHEAD and results['noise'][0][0] == 0
  # the run limits: 1 literal + matches of at most 258
  assert len(results['repeat 65535'][0]) < 400
  # the length limit engaged and left a complete code
  lens = [l for l in _literal_code_lengths(results['fibonacci'][0]) if l]
  assert len(lens) == 21 and max(lens) == 15 and sum(2 ** (15 - l) for l in lens) == 2 ** 15
  # a dynamic block where it pays: the ramp under Sub
  assert len(results['ramp mode 1'][0]) < 0.5 * ramp.size


def test_adler_combine_matches_zlib():
  L = _lib.lib()
  rng = np.random.default_rng(1)
  for n in (0, 1, 2, 5552, 70001):
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for split in sorted({0, min(1, n), n // 2, n}):
      a, b = zlib.adler32(data[:split]), zlib.adler32(data[split:])
      assert L.se3ds_adler32_combine(a, b, n - split) == zlib.adler32(data), (n, split)
  ones = b'\xff' * 200000   # the sums wrap many times
  assert L.se3ds_adler32_combine(zlib.adler32(ones[:131071]), zlib.adler32(ones[131071:]),
                                 len(ones) - 131071) == zlib.adler32(ones)


def test_bad_tables_are_rejected_before_the_device():
  L = _lib.lib()
  assert L.se3ds_png_encode_fields() == 8
  max_row = L.se3ds_png_encode_max_row_bytes()
  assert max_row >= 24576
  fake = 1 << 20   # never dereferenced: every call below fails on the host

  def call(table, n=None, ws=None, out=None, table_dev=fake, workspace=fake, out_ptr=fake, sizes=fake,
           phases=3):
    n = len(table) if n is None else n
    need_ws = L.se3ds_png_encode_workspace_bytes(table.ctypes.data, n)
    need_out = L.se3ds_png_encode_out_bytes(table.ctypes.data, n)
    return L.se3ds_png_encode(table_dev, table.ctypes.data, n, workspace, need_ws if ws is None else ws,
                              out_ptr, need_out if out is None else out, sizes, phases, None)

  good = png.encode_table([fake, fake], [(65, 341 * 3, 3), (7, 64, 1)], [png.ADAPTIVE, 0])
  need = L.se3ds_png_encode_workspace_bytes(good.ctypes.data, 2)
  # 65535 // 1024 = 63 rows a strip: 2 + 1 strips of 16 bytes of records, then their slots
  assert need == 48 + 2 * ((10 + 63 * 1024 + 7) & ~7) + ((10 + 7 * 65 + 7) & ~7)
  assert L.se3ds_png_encode_out_bytes(good.ctypes.data, 2) == 20 + 65 * 1024 + 10 + 7 * 65
  BADSHAPE, WORKSPACE, UNSUPPORTED = -1, -3, -5
  assert call(good, ws=need - 1) == WORKSPACE
  assert call(good, out=L.se3ds_png_encode_out_bytes(good.ctypes.data, 2) - 1) == BADSHAPE
  assert call(good, n=0) == BADSHAPE and call(good, n=-1) == BADSHAPE
  for null in ('table_dev', 'workspace', 'out_ptr', 'sizes'):
    assert call(good, **{null: None}) == BADSHAPE, null
  assert L.se3ds_png_encode(fake, None, 2, fake, need, fake, 1 << 30, fake, 3, None) == BADSHAPE
  assert call(good, phases=0) == BADSHAPE and call(good, phases=4) == BADSHAPE

  def broken(row, column, value):
    t = good.copy()
    t[row, column] = value
    return t

  assert call(broken(0, 0, 0)) == BADSHAPE                      # null image
  assert call(broken(0, 1, 0)) == BADSHAPE                      # height
  assert call(broken(0, 2, 341 * 3 + 1)) == BADSHAPE            # row_bytes no multiple of 3
  assert call(broken(1, 3, 2)) == BADSHAPE                      # bytes per pixel
  assert call(broken(1, 4, 6)) == BADSHAPE                      # filter
  assert call(broken(1, 5, 3)) == BADSHAPE                      # first strip
  assert call(broken(1, 6, 8)) == BADSHAPE                      # out offset
  assert call(broken(1, 7, 8)) == BADSHAPE                      # slot offset
  wide = png.encode_table([fake], [(1, max_row + 1, 1)], [0])
  assert call(wide) == UNSUPPORTED and L.se3ds_png_encode_workspace_bytes(wide.ctypes.data, 1) == 0
  widest = png.encode_table([fake], [(1, max_row, 1)], [0])
  assert L.se3ds_png_encode_workspace_bytes(widest.ctypes.data, 1) > max_row
  # grid quantise: shapes are checked on the host too
  q = lambda n, c, ny, nx, out_c, dtype=_lib.F32: L.se3ds_grid_quantize(fake, dtype, n, 3, 5, c, ny, nx,
                                                                        out_c, fake, None)
  assert q(3, 3, 2, 2, 3) == BADSHAPE and q(4, 2, 2, 2, 3) == BADSHAPE and q(4, 3, 2, 2, 1) == BADSHAPE
  assert q(4, 1, 2, 2, 2) == BADSHAPE and q(4, 3, 2, 2, 3, _lib.I32) == -2
  import torch
  with pytest.raises(_lib.Se3dsHipError):
    png.encode_png_batch([torch.zeros((2, 2, 3), dtype=torch.uint8)])
  with pytest.raises(ValueError, match='filters'):
    png.encode_png_host(np.zeros((2, 2, 3), np.uint8), filters=7)


@pytest.mark.parametrize('filters', [0, 1, 2, 3, 4, 'adaptive'])
def test_host_encoder_round_trips(filters):
  rng = np.random.default_rng(7)
  for shape in ((1, 1, 1), (5, 21, 3), (7, 64, 1), (33, 41, 3)):
    ramp = np.arange(shape[1])[None, :, None] * 2 + np.arange(shape[0])[:, None, None] * 5
    pixels = ((ramp + rng.integers(0, 6, shape)) % 256).astype(np.uint8)
    plane = png.parse_png(png.encode_png_host(pixels, filters))
    assert (plane.height, plane.width, plane.bit_depth, plane.channels) == shape[:2] + (8, shape[2])
    rows = _png_ref.reconstruct(plane.filtered, plane.height, plane.row_bytes, plane.bytes_per_pixel)
    assert np.array_equal(np.asarray(rows, np.uint8).reshape(shape), pixels)
    types, filtered = R.filter_rows(pixels, png._filter_mode(filters))
    assert plane.filtered == filtered.tobytes()   # the rule of the device encoder, ties included


# ------------------------------------------------------------------------------ event files
def _fields(buf):
  """A protobuf wire decoder written for this test: [(field number, wire type, value)]."""
  out, pos = [], 0

  def varint():
    nonlocal pos
    shift = value = 0
    while True:
      byte = buf[pos]
      pos += 1
      value |= (byte & 0x7f) << shift
      shift += 7
      if byte < 0x80:
        return value

  while pos < len(buf):
    key = varint()
    number, wire = key >> 3, key & 7
    if wire == 0:
      value = varint()
    elif wire == 1:
      value = struct.unpack_from('<d', buf, pos)[0]
      pos += 8
    elif wire == 5:
      value = struct.unpack_from('<f', buf, pos)[0]
      pos += 4
    else:
      assert wire == 2
      n = varint()
      value = buf[pos:pos + n]
      pos += n
    out.append((number, wire, value))
  return out


def _decode(record):
  """Event -> (wall_time, step, file_version, [(tag, value)]) from the field numbers of event.proto
  and summary.proto: Event 1 / 2 / 3 / 5, Summary 1, Value 1 / 2 / 4, Image 1 / 2 / 3 / 4."""
  event = {n: v for n, _, v in _fields(record)}
  values = []
  for n, _, value in _fields(event.get(5, b'')):
    assert n == 1
    v = {k: x for k, _, x in _fields(value)}
    if 4 in v:
      image = {k: x for k, _, x in _fields(v[4])}
      values.append((v[1].decode(), (image[1], image[2], image[3], image[4])))
    else:
      values.append((v[1].decode(), v[2]))
  return event.get(1), event.get(2, 0), event.get(3, b'').decode(), values


def test_event_file_round_trip(tmp_path):
  w = tf_events.EventFileWriter(str(tmp_path / 'logs'))
  assert re.fullmatch(r'events\.out\.tfevents\.\d{10}\.' + re.escape(socket.gethostname()),
                      os.path.basename(w.path))
  picture = png.encode_png_host(np.arange(24, dtype=np.uint8).reshape(2, 4, 3))
  w.add_scalar('gen_loss', 1.25, 7)
  w.add_scalar('val/eval_image/fid@1', -3.5e-3, 0)
  w.add_image('train_real_img', picture, 2, 4, 2 ** 40)
  w.flush()
  records = list(tf_records.read_records(w.path, verify=True))
  assert len(records) == 4
  w.add_scalar('late', 2.0, 8)
  w.close()
  w.close()
  with pytest.raises(ValueError):
    w.add_scalar('closed', 0.0, 9)
  records = list(tf_records.read_records(w.path, verify=True))
  decoded = [_decode(r) for r in records]
  assert decoded[0][1:] == (0, 'brain.Event:2', []) and decoded[0][0] > 1.6e9
  assert decoded[1][1:] == (7, '', [('gen_loss', 1.25)])
  assert decoded[2][1:] == (0, '', [('val/eval_image/fid@1', np.float32(-3.5e-3))])
  assert decoded[3][1:] == (2 ** 40, '', [('train_real_img', (2, 4, 3, picture))])
  assert decoded[4][1:] == (8, '', [('late', 2.0)])
  events = list(tf_events.read_events(w.path))
  assert [(s, v) for _, s, v in events] == [
      (0, {}), (7, {'gen_loss': 1.25}), (0, {'val/eval_image/fid@1': np.float32(-3.5e-3)}),
      (2 ** 40, {'train_real_img': (2, 4, picture)}), (8, {'late': 2.0})]
  assert [t for t, _, _ in events] == [d[0] for d in decoded]
  # the exact bytes of a scalar event, assembled by hand
  assert tf_events.encode_event(2.0, 3, value=tf_events.scalar_value('a', 0.5)) == (
      b'\x09' + struct.pack('<d', 2.0) + b'\x10\x03' + b'\x2a\x0a' + b'\x0a\x08' + b'\x0a\x01a' +
      b'\x15' + struct.pack('<f', 0.5))
  other = tmp_path / 'plain.tfrecord'
  tf_records.write_records(str(other), [records[1]])
  with pytest.raises(ValueError, match='version record'):
    list(tf_events.read_events(str(other)))


def test_universal_logger_on_the_host(tmp_path):
  lines = []
  log = logger_lib.UniversalLogger(str(tmp_path), step=0, num_train_steps=10, logging_fn=lines.append,
                                   encoder='host')
  log.log_scalars(5, gen_loss=np.float32(1.23456), disc_loss=0.5)
  assert lines == ['[5] disc_loss = 0.500, gen_loss = 1.235']
  rng = np.random.default_rng(2)
  many = rng.integers(0, 256, (12, 3, 5, 3), dtype=np.uint8)
  one = rng.integers(0, 256, (1, 4, 6, 1), dtype=np.uint8)
  log.log_images(6, max_outputs=10, b_many=many, a_one=one)
  log.log_images(7, max_outputs=2, b_many=many)
  log.close()
  with pytest.raises(ValueError, match='encoder'):
    logger_lib.UniversalLogger(str(tmp_path), step=0, encoder='gpu')
  events = list(tf_events.read_events(log.summary_writer.path))[1:]
  assert [(s, list(v)) for _, s, v in events[:2]] == [(5, ['disc_loss']), (5, ['gen_loss'])]
  assert events[1][2]['gen_loss'] == np.float32(1.23456)
  tags = [(s, next(iter(v))) for _, s, v in events[2:]]
  assert tags == [(6, 'a_one')] + [(6, f'b_many/image/{i}') for i in range(10)] + [
      (7, 'b_many/image/0'), (7, 'b_many/image/1')]
  for (_, _, values), want in zip(events[2:], [one[0]] + list(many[:10]) + list(many[:2])):
    (h, w, data), = values.values()
    plane = png.parse_png(data)
    assert (h, w) == want.shape[:2] == (plane.height, plane.width) and plane.channels == want.shape[2]
    rows = _png_ref.reconstruct(plane.filtered, h, plane.row_bytes, plane.bytes_per_pixel)
    assert np.array_equal(np.asarray(rows, np.uint8).reshape(want.shape), want)
  # one file per logger
  assert len(os.listdir(tmp_path)) == 1
