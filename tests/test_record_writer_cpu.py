"""The record writer without a GPU: the 16-bit path of csrc/deflate_core.h as a stand-alone host program
under AddressSanitizer and UndefinedBehaviorSanitizer against zlib and a NumPy restatement of the
filters, the 16-bit host PNG encoder, the record layout against tf_records, the quantisation rule,
the host-side rejection of bad tables, and the device flush's layout replayed in NumPy.  The kernels
run in tests/test_record_writer_gpu.py."""
import hashlib
import struct
import zlib

import numpy as np
import pytest

import _png_encode_ref as R
import _png_ref
import _record_ref as Q
from se3ds_amd import _lib
from se3ds_amd.datasets import indoor_datasets, record_writer
from se3ds_amd.utils import png, tf_records
from se3ds_amd.utils.tf_bundle import crc32c, mask_crc

BADSHAPE = -1


def test_16_bit_filter_as_a_sanitised_host_program(tmp_path):
  """Every size x content x filter mode as a kind-2 corpus entry: zlib must inflate each stream to
  the filtered big-endian bytes the NumPy restatement gives, with their Adler-32, within 10 bytes a
  strip.  A kind-1 corpus gives the result file it gave before kind 2 existed."""
  exe = R.build_host_program(tmp_path, sanitize=True)
  names, entries, images = [], [], []
  for si, (h, w) in enumerate(Q.SIZES_16):
    for name, samples in Q.contents_16(h, w, seed=si).items():
      for mode in range(6):
        names.append(((h, w), name, mode))
        images.append(samples)
        entries.append(Q.corpus_entry_16(samples, mode))
  results, _ = Q.run_host_program_raw(exe, entries, tmp_path)
  for (geom, name, mode), samples, (stream, s1, s2) in zip(names, images, results):
    types, filtered = Q.filter_rows_16(samples, mode)
    data = filtered.tobytes()
    strips = R.strips_of(filtered, filtered.shape[1] - 1)
    assert len(strips) == (2 if geom == (128, 256) else 1)
    assert len(stream) <= sum(R.OVERHEAD + len(s) for s in strips), (geom, name, mode)
    assert (s2 << 16) | s1 == zlib.adler32(data), (geom, name, mode)
    assert zlib.decompress(b'\x78\x01' + stream + struct.pack('>I', zlib.adler32(data))) == data, \
        (geom, name, mode)
    if mode < 5:
      assert np.all(types == mode)
  # kinds 0 and 1 are untouched: an image's stream is that of its NumPy-filtered strips, and the
  # result file of a fixed corpus has the digest it had at the commit before this entry kind
  x, y, c = np.arange(341)[None, :, None], np.arange(70)[:, None, None], np.arange(3)
  fixed = [(((3 * x + 5 * y + 11 * c) % 256).astype(np.uint8), m) for m in range(6)]
  fixed.append((((x * x + 7 * y * c) % 251).astype(np.uint8)[:, :64, :1].copy(), R.ADAPTIVE))
  by_image = R.run_host_program(exe, fixed, tmp_path)
  for (px, mode), (stream, s1, s2) in zip(fixed, by_image):
    filtered = R.filter_rows(px, mode)[1]
    strips = R.strips_of(filtered, filtered.shape[1] - 1)
    by_strip = R.run_host_program(exe, [(s, k == len(strips) - 1) for k, s in enumerate(strips)], tmp_path)
    assert stream == b''.join(s for s, _, _ in by_strip)
  R.run_host_program(exe, fixed, tmp_path)
  digest = hashlib.sha256(open(tmp_path / 'result.bin', 'rb').read()).hexdigest()
  assert digest == KIND_1_DIGEST


KIND_1_DIGEST = '9c9d571143f5ac9569a8419e3b62d3c7fe185b8a2a559061318bb88bcfc11ac6'


def test_host_png_round_trip_16_bit():
  for si, (h, w) in enumerate(Q.SIZES_16):
    for name, samples in Q.contents_16(h, w, seed=10 + si).items():
      # (the reference decoder is a Python loop: the two-strip size takes one filter choice)
      for filters in ('adaptive', 0, 1, 2, 3, 4) if h < 128 else ('adaptive',):
        blob = png.encode_png_host(samples[:, :, None], filters)
        plane = png.parse_png(blob)
        assert (plane.height, plane.width, plane.bit_depth, plane.channels) == (h, w, 16, 1)
        assert plane.filtered == Q.filter_rows_16(samples, png._filter_mode(filters))[1].tobytes()
        got = _png_ref.decode_png(plane.filtered, h, w, 16, 1)   # reconstruct + byte swap
        assert got.dtype == np.uint16 and np.array_equal(got, samples), (h, w, name, filters)
  # what worked before is what it was
  grey = np.arange(35, dtype=np.uint8).reshape(5, 7, 1)
  assert png.png_container(5, 7, 1, b'abc') == png.png_container(5, 7, 1, b'abc', 8)
  assert png.parse_png(png.encode_png_host(grey)).bit_depth == 8
  with pytest.raises(ValueError):
    png.encode_png_host(np.zeros((4, 4, 3), np.uint16))
  with pytest.raises(ValueError):
    png.png_container(4, 4, 3, b'', 16)


def _host_examples(h, rng, count):
  w = 2 * h
  out = []
  for i in range(count):
    pix = dict(image=rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
               proj_image=rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
               depth=rng.integers(0, 65536, (h, w, 1)).astype(np.uint16),
               proj_depth=rng.integers(0, 65536, (h, w, 1)).astype(np.uint16),
               proj_mask=rng.integers(0, 2, (h, w, 1), dtype=np.uint8) * np.uint8(255),
               blurred_mask=rng.integers(0, 3, (h, w, 1), dtype=np.uint8),
               segmentation=rng.integers(0, 42, (h, w, 1), dtype=np.uint8))
    example = {k: png.encode_png_host(v) for k, v in pix.items()}
    if i != 1:   # the second example leaves everything at its default
      example.update(scan_id=b'scan%d' % i, filename=b'pano_%d.png' % i, depth_scale=12.5 + i,
                     bbox=(1, 2, 3.5, 4))
    out.append((example, pix))
  return out


def test_host_layout_is_the_one_tf_records_reads(tmp_path):
  rng = np.random.default_rng(3)
  examples = _host_examples(8, rng, 3)
  blob = record_writer.encode_records_host([e for e, _ in examples])
  assert blob == b''.join(tf_records.frame_record(tf_records.encode_example(
      record_writer.example_features(e))) for e, _ in examples)
  path = str(tmp_path / 'train-0.tfrecord')
  with open(path, 'wb') as f:
    f.write(blob)
  records = list(tf_records.read_records(path, verify=True))
  assert len(records) == 3
  ds = indoor_datasets.R2RImageDataset(preprocessed_image_height=8, return_filename=True)
  for i, (rec, (example, pix)) in enumerate(zip(records, examples)):
    parsed = tf_records.parse_example(rec)
    assert set(parsed) <= set(ds._features())   # only features `_parse` reads
    for name, (feature, channels, depth) in indoor_datasets.IMAGE_PLANES.items():
      assert parsed[feature] == [example[name]]
    out = ds._parse(rec)
    for name, (feature, channels, depth) in indoor_datasets.IMAGE_PLANES.items():
      assert (out[name].channels, out[name].bit_depth) == (channels, depth)
      assert out[name].filtered == png.parse_png(example[name]).filtered
    if i == 1:
      assert (out['scan_id'], out['filename'], out['depth_scale'], out['dataset_type']) == (b'', b'', 10.0, 0)
      assert np.array_equal(out['bbox'], [0, 0, 0, 0])
    else:
      assert (out['scan_id'], out['filename']) == (b'scan%d' % i, b'pano_%d.png' % i)
      assert out['depth_scale'] == np.float32(12.5 + i)
      assert np.array_equal(out['bbox'], np.array([1, 2, 3.5, 4], np.float32))


def test_device_layout_replayed_in_numpy():
  """What a flush does on the device -- segments gathered from the literals and the compact
  streams, CRC-32 of the IDAT chunks patched in big-endian, CRC-32C of the frames patched in masked --
  replayed in NumPy on zlib streams: the file equals encode_records_host of the same PNG files."""
  rng = np.random.default_rng(4)
  h, w = 6, 12
  compact, payloads, hosts = bytearray(), [], []
  for i in range(2):
    planes, files = {}, {}
    for name, (feature, channels, depth) in indoor_datasets.IMAGE_PLANES.items():
      px = rng.integers(0, 1 << depth, (h, w, channels)).astype(np.uint16 if depth == 16 else np.uint8)
      filtered = png.filter_rows_host(px, 1).tobytes()
      z = zlib.compressobj(6, zlib.DEFLATED, -15)     # a raw deflate stream, as the encoder's
      stream = z.compress(filtered) + z.flush()
      compact += b'\xee' * int(rng.integers(0, 5))   # the streams do not lie back to back
      planes[name] = record_writer._png_pieces(h, w * channels * depth // 8, channels * depth // 8,
                                               len(compact), len(stream), zlib.adler32(filtered))
      files[name] = png.png_container(h, w, channels, b'\x78\x01' + stream + struct.pack(
          '>I', zlib.adler32(filtered)), depth)
      compact += stream
    meta = dict(scan_id=b'abc', depth_scale=3.25) if i else {}
    payloads.append(record_writer._example_pieces(dict(planes, **meta)))
    hosts.append(dict(files, **meta))
  layout = record_writer._Layout(payloads, 37)   # a small limit: every longer range is split
  sources = [np.frombuffer(bytes(layout.literals), np.uint8), np.frombuffer(bytes(compact), np.uint8)]
  out = np.full(layout.total, 0x5a, np.uint8)
  covered = np.zeros(layout.total, np.int64)
  end = 0
  for which, at, to, length in layout.segments:
    assert 0 < length <= 37 and to >= end
    out[to:to + length] = sources[which][at:at + length]
    covered[to:to + length] += 1
    end = to + length
  assert np.all(covered == 1)   # every byte of the file has exactly one writer
  assert len(layout.idat) == 14 and len(layout.frames) == 2
  for at, length, crc_at in layout.idat:
    assert out[at:at + 4].tobytes() == b'IDAT' and crc_at == at + length
    out[crc_at:crc_at + 4] = np.frombuffer(struct.pack('>I', zlib.crc32(out[at:at + length].tobytes())), np.uint8)
  for at, n in layout.frames:
    for lo, hi in ((at, at + 8), (at + 12, at + 12 + n)):
      out[hi:hi + 4] = np.frombuffer(struct.pack('<I', mask_crc(crc32c(out[lo:hi].tobytes()))), np.uint8)
  assert out.tobytes() == record_writer.encode_records_host(hosts)


def test_quantisation_inverts_the_decoder_for_every_code():
  codes = np.arange(65536, dtype=np.uint16)
  as_division = codes.astype(np.float32) / np.float32(65535)
  as_product = codes.astype(np.float32) * (np.float32(1) / np.float32(65535))
  assert np.array_equal(Q.depth_codes(as_division), codes)
  assert np.array_equal(Q.depth_codes(as_product), codes)
  assert list(Q.depth_codes([np.nan, -1, -np.inf, 2, np.inf])) == [0, 0, 0, 65535, 65535]


def test_bad_tables_are_rejected_before_the_device():
  L = _lib.lib()
  fake = 1 << 20   # never dereferenced: every call below fails on the host
  assert L.se3ds_assemble_fields() == 4 and L.se3ds_patch_crc_fields() == 3
  limit = L.se3ds_assemble_max_segment_bytes()
  assert limit >= 4096
  sources = np.array([[fake, 100], [fake, 1000]], np.int64)

  def assemble(rows, n=None, m=2, out_bytes=500, src=sources, out=fake, table_dev=fake):
    table = np.array(rows, np.int64).reshape(-1, 4)
    return L.se3ds_assemble_segments(src.ctypes.data, m, table_dev, table.ctypes.data,
                                     len(table) if n is None else n, out, out_bytes, None)

  good = [(0, 0, 0, 100), (1, 990, 100, 10), (0, 5, 110, 0), (1, 0, 110, 390)]
  assert assemble([(0, 1, 0, 100)]) == BADSHAPE          # leaves its source
  assert assemble([(1, 991, 0, 10)]) == BADSHAPE
  assert assemble([(0, -1, 0, 10)]) == BADSHAPE
  assert assemble([(2, 0, 0, 10)]) == BADSHAPE           # no such source
  assert assemble([(-1, 0, 0, 10)]) == BADSHAPE
  assert assemble([(1, 0, 491, 10)]) == BADSHAPE         # leaves out
  assert assemble([(1, 0, -1, 10)]) == BADSHAPE
  assert assemble(good[:2] + [(1, 0, 109, 10)]) == BADSHAPE      # overlaps the one in front
  assert assemble([good[1], good[0]]) == BADSHAPE                # descending
  assert assemble(good, n=0) == BADSHAPE
  assert assemble(good, n=-1) == BADSHAPE
  assert assemble([(0, 0, 0, -1)]) == BADSHAPE
  big = np.array([[fake, 4 * limit]], np.int64)
  assert assemble([(0, 0, 0, limit + 1)], m=1, src=big, out_bytes=4 * limit) == BADSHAPE
  assert assemble(good, m=0) == BADSHAPE
  assert assemble(good, m=9) == BADSHAPE
  assert assemble(good, out=None) == BADSHAPE
  assert assemble(good, table_dev=None) == BADSHAPE
  assert assemble(good, src=np.array([[0, 100], [fake, 1000]], np.int64)) == BADSHAPE

  def patch(rows, n=None, crc_count=4, out_bytes=100, crc=fake, out=fake):
    table = np.array(rows, np.int64).reshape(-1, 3)
    return L.se3ds_patch_crc(crc, crc_count, fake, table.ctypes.data, len(table) if n is None else n,
                             out, out_bytes, None)

  for at in (97, 98, 99, 100, -1):                       # within 4 bytes of the end
    assert patch([(0, at, 0)]) == BADSHAPE
  assert patch([(4, 0, 0)]) == BADSHAPE
  assert patch([(-1, 0, 0)]) == BADSHAPE
  assert patch([(0, 0, 2)]) == BADSHAPE
  assert patch([(0, 10, 0), (1, 13, 1)]) == BADSHAPE     # overlapping
  assert patch([(0, 10, 0)], n=0) == BADSHAPE
  assert patch([(0, 10, 0)], crc=None) == BADSHAPE
  assert patch([(0, 10, 0)], out=None) == BADSHAPE

  # the planes entry: 1, 2 and 3 bytes per pixel; se3ds_png_encode still refuses 2
  def planes(table, entry='se3ds_png_encode_planes'):
    n = len(table)
    need_ws = getattr(L, entry + '_workspace_bytes')(table.ctypes.data, n)
    need_out = getattr(L, entry + '_out_bytes')(table.ctypes.data, n)
    return getattr(L, entry)(fake, table.ctypes.data, n, fake, need_ws, fake, need_out, fake, 3, None), \
        need_ws, need_out

  mixed = png.encode_table([fake] * 3, [(128, 512, 2), (7, 64, 1), (5, 63, 3)], [png.ADAPTIVE, 0, 4])
  assert L.se3ds_png_encode_planes_out_bytes(mixed.ctypes.data, 3) == \
      20 + 128 * 513 + 10 + 7 * 65 + 10 + 5 * 64
  assert L.se3ds_png_encode_planes_workspace_bytes(mixed.ctypes.data, 3) > 0
  assert planes(mixed, 'se3ds_png_encode') == (BADSHAPE, 0, 0)
  for bpp in (0, 4, 6):
    bad = mixed.copy()
    bad[0, 3] = bpp
    assert planes(bad) == (BADSHAPE, 0, 0)
  odd = png.encode_table([fake], [(4, 9, 2)], [0])   # half a sample in a row
  assert planes(odd) == (BADSHAPE, 0, 0)
  # half a pair, no pair, no pixels
  assert L.se3ds_record_planes(fake, None, None, 16, None, None, None, None) == BADSHAPE
  assert L.se3ds_record_planes(None, None, None, 16, None, None, None, None) == BADSHAPE
  assert L.se3ds_record_planes(None, fake, None, 0, None, fake, None, None) == BADSHAPE
  assert L.se3ds_record_planes(None, fake + 2, None, 16, None, fake, None, None) == BADSHAPE


def test_no_cpu_fallback(tmp_path):
  import torch
  with pytest.raises(_lib.Se3dsHipError):
    record_writer.R2RRecordWriter(str(tmp_path / 'x.tfrecord'), 'cpu')
  with pytest.raises(_lib.Se3dsHipError):
    record_writer.record_planes(proj_depth=torch.zeros((4, 4)))
  with pytest.raises(_lib.Se3dsHipError):
    png.encode_png_batch([torch.zeros((4, 4, 1), dtype=torch.int16)])
  assert not list(tmp_path.iterdir())


def test_write_records_default_is_unchanged_and_atomic(tmp_path):
  path = str(tmp_path / 'a.tfrecord')
  records = [b'', b'x', bytes(range(200))]
  tf_records.write_records(path, records)
  assert open(path, 'rb').read() == b''.join(tf_records.frame_record(r) for r in records)
  assert [p.name for p in tmp_path.iterdir()] == ['a.tfrecord']
  with pytest.raises(ValueError):
    tf_records.write_records(path, records, checksums='gpu')

  def broken():
    yield b'abc'
    raise RuntimeError('stop')
  with pytest.raises(RuntimeError):
    tf_records.write_records(str(tmp_path / 'b.tfrecord'), broken())
  assert [p.name for p in tmp_path.iterdir()] == ['a.tfrecord']
