"""Shared by tests/test_png_encode_cpu.py and tests/test_png_encode_gpu.py: the corpus format of
tools/deflate_host_check.cpp, its build, and a NumPy restatement of the PNG filters and of the
adaptive rule (smallest sum of |int8(residual)|, ties to the lowest type), written from the PNG
specification, section 9 -- not from csrc/deflate_core.h."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tools', 'deflate_host_check.cpp')
ADAPTIVE = 5
OVERHEAD = 10   # stored-block header + the empty stored block that ends a strip


def strip_rows(row_bytes):
  return max(1, 65535 // (1 + row_bytes))


def build_host_program(directory, sanitize):
  """-> path of the compiled tools/deflate_host_check.cpp.  sanitize: AddressSanitizer +
  UndefinedBehaviorSanitizer, reports fatal, runtimes linked statically: the program stands alone."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the encoder core cannot be built for the host'
  exe = os.path.join(str(directory), 'deflate_host_check' + ('_san' if sanitize else ''))
  flags = ['-std=c++17', '-Wall', '-Wextra', '-Werror']
  if sanitize:
    flags += ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags += ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  else:
    flags += ['-O2']
  b = subprocess.run([cxx] + flags + [SOURCE, '-o', exe], capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  return exe


def corpus_file(cases):
  """cases: bytes-like (one final strip of filtered bytes), (bytes, final flag), or
  (pixels uint8 (h, w, c), filter mode)."""
  out = [b'DEFC', struct.pack('<I', len(cases))]
  for case in cases:
    if isinstance(case, tuple) and isinstance(case[0], np.ndarray):
      px, mode = case
      h, w, c = px.shape
      out.append(struct.pack('<5I', 1, h, w * c, c, mode) + np.ascontiguousarray(px).tobytes())
    else:
      data, final = case if isinstance(case, tuple) else (case, True)
      out.append(struct.pack('<3I', 0, len(data), int(final)) + bytes(data))
  return b''.join(out)


def run_host_program(exe, cases, directory):
  """-> [(stream, s1, s2)] per case."""
  corpus = os.path.join(str(directory), 'corpus.bin')
  result = os.path.join(str(directory), 'result.bin')
  with open(corpus, 'wb') as f:
    f.write(corpus_file(cases))
  r = subprocess.run([exe, corpus, result], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert f'{len(cases)} cases OK' in r.stdout
  buf = open(result, 'rb').read()
  out, pos = [], 0
  for _ in cases:
    n, s1, s2 = struct.unpack_from('<3I', buf, pos)
    out.append((buf[pos + 12:pos + 12 + n], s1, s2))
    pos += 12 + n
  assert pos == len(buf)
  return out


def _paeth(a, b, c):
  p = a + b - c
  pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
  return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(pixels, mode):
  """uint8 (h, w, c) -> (filter types (h,), filtered scan lines uint8 (h, 1 + w*c))."""
  h, w, c = pixels.shape
  cur = pixels.reshape(h, w * c).astype(np.int64)
  a = np.concatenate([np.zeros((h, c), np.int64), cur[:, :-c]], axis=1)[:, :w * c]
  b = np.concatenate([np.zeros((1, w * c), np.int64), cur[:-1]], axis=0)
  cc = np.concatenate([np.zeros((h, c), np.int64), b[:, :-c]], axis=1)[:, :w * c]
  res = np.stack([cur, cur - a, cur - b, cur - (a + b) // 2, cur - _paeth(a, b, cc)]) & 0xff   # (5, h, n)
  if mode == ADAPTIVE:
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)   # (5, h)
    types = np.argmin(cost, axis=0)                          # the first minimum: ties to the lowest
  else:
    types = np.full((h,), mode, np.int64)
  rows = res[types, np.arange(h)]
  return types.astype(np.uint8), np.concatenate([types[:, None], rows], axis=1).astype(np.uint8)


def strips_of(filtered, row_bytes):
  """The filtered scan lines (h, 1 + row_bytes) cut as the encoder cuts them -> [bytes]."""
  per = strip_rows(row_bytes)
  return [filtered[r:r + per].tobytes() for r in range(0, filtered.shape[0], per)]


GEOMETRIES = [(1, 1, 1), (1, 1, 3), (2, 3, 3), (5, 21, 3), (7, 64, 1), (33, 341, 3),
              (65, 341, 3), (129, 341, 3)]   # 1 + 341 * 3 = 1024 bytes a row: strips end mid-image
COMPRESSIBLE = ('zeros', 'horizontal ramp', 'vertical ramp', 'ramp + noise', 'one pixel per strip')


def contents(h, w, c, seed):
  """{name: uint8 (h, w, c)}: what an encoder can get wrong lies in the filters' choice (the ramps),
  the runs (zeros, the lone pixels), the stored fallback (noise) and plain literals (ramp + noise)."""
  rng = np.random.default_rng(seed)
  x = np.arange(w)[None, :, None] + np.zeros((h, 1, c), np.int64)
  y = np.arange(h)[:, None, None] + np.zeros((1, w, c), np.int64)
  lone = np.zeros((h, w, c), np.uint8)
  per = strip_rows(w * c)
  for k, r in enumerate(range(0, h, per)):   # one pixel in every strip, on its first or last row
    lone[r if k % 2 == 0 else min(r + per, h) - 1, (7 * k) % w] = 255 - k
  return {
      'zeros': np.zeros((h, w, c), np.uint8),
      # a step of 3 along the row and of 128 (the dearest residual) across rows: Sub costs 3 a byte,
      # Paeth can only tie with it and every other type costs more; the vertical ramp likewise for Up
      'horizontal ramp': ((3 * x + 128 * y + 11 * np.arange(c)) % 256).astype(np.uint8),
      'vertical ramp': ((5 * y + 128 * x + 7 * np.arange(c)) % 256).astype(np.uint8),
      'ramp + noise': ((x + 2 * y + rng.integers(0, 7, (h, w, c))) % 256).astype(np.uint8),
      'noise': rng.integers(0, 256, (h, w, c)).astype(np.uint8),
      'one pixel per strip': lone,
  }


def zlib_rle(data):
  import zlib
  z = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
  return z.compress(data) + z.flush()
