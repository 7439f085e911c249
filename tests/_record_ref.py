"""Shared by tests/test_record_writer_cpu.py and tests/test_record_writer_gpu.py: the kind-2 (16-bit)
corpus entries of tools/deflate_host_check.cpp, 16-bit test images, and NumPy restatements of the
rules of csrc/records.hip, written from include/se3ds_hip.h -- not from the kernels."""
import os
import struct
import subprocess

import numpy as np

import _png_encode_ref as R

SIZES_16 = [(1, 1), (2, 3), (7, 64), (128, 256)]   # 1 + 2 * 256 = 513 bytes a row: 127 rows a strip


def contents_16(h, w, seed):
  """{name: uint16 (h, w)}: zeros, a ramp whose steps cross byte boundaries, noise."""
  rng = np.random.default_rng(seed)
  x, y = np.arange(w)[None, :], np.arange(h)[:, None]
  return {'zeros': np.zeros((h, w), np.uint16),
          'ramp': ((250 + 3 * x + 255 * y) % 65536).astype(np.uint16),
          'noise': rng.integers(0, 65536, (h, w)).astype(np.uint16)}


def big_endian_bytes(samples):
  """uint16 (h, w) -> uint8 (h, w, 2): the bytes PNG stores, most significant first."""
  return np.stack([samples >> 8, samples & 0xff], axis=2).astype(np.uint8)


def filter_rows_16(samples, mode):
  """PNG filtering of a 16-bit grey image: the 8-bit rule on its big-endian bytes, 2 bytes a pixel."""
  return R.filter_rows(big_endian_bytes(samples), mode)


def corpus_entry_16(samples, mode):
  """Kind 2: the header of kind 1 with 2 bytes per pixel, then the samples little-endian."""
  h, w = samples.shape
  return struct.pack('<5I', 2, h, 2 * w, 2, mode) + samples.astype('<u2').tobytes()


def run_host_program_raw(exe, entries, directory, name='corpus16'):
  """As R.run_host_program for corpus entries that are already packed -> ([(stream, s1, s2)], the
  result file's bytes)."""
  corpus = os.path.join(str(directory), name + '.bin')
  result = os.path.join(str(directory), name + '.result')
  with open(corpus, 'wb') as f:
    f.write(b'DEFC' + struct.pack('<I', len(entries)) + b''.join(entries))
  r = subprocess.run([exe, corpus, result], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert f'{len(entries)} cases OK' in r.stdout
  buf = open(result, 'rb').read()
  out, pos = [], 0
  for _ in entries:
    n, s1, s2 = struct.unpack_from('<3I', buf, pos)
    out.append((buf[pos + 12:pos + 12 + n], s1, s2))
    pos += 12 + n
  assert pos == len(buf)
  return out, buf


def depth_codes(d):
  """float32 -> uint16: floor((double)d * 65535 + 0.5) clamped to [0, 65535], NaN -> 0."""
  with np.errstate(invalid='ignore'):
    q = np.floor(np.asarray(d, np.float32).astype(np.float64) * 65535 + 0.5)
    q = np.where(np.isnan(q), 0, np.clip(q, 0, 65535))
  return q.astype(np.uint16)


def rgb_codes(v):
  """float32 -> uint8: truncated toward zero, clamped to [0, 255]; void, negative and NaN -> 0."""
  v = np.asarray(v, np.float32)
  with np.errstate(invalid='ignore'):
    q = np.where(np.isnan(v), 0, np.clip(v, 0, 255))
  return np.trunc(q).astype(np.uint8)


def mask_codes(m):
  return np.where(np.asarray(m, np.float32) == 1, 255, 0).astype(np.uint8)


def neighbours(values):
  """float32 values with the float32 just below and just above each."""
  v = np.asarray(values, np.float32)
  return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])
