"""Writes tests/golden/jpeg_encode_fixtures.npz: the input pixels, the parameters and the file
Pillow writes (libjpeg's default baseline encoder: Annex K Huffman tables, no optimisation, no
progression) for the cases of tests/test_jpeg_encode_gpu.py, which needs no Pillow itself.
tests/test_jpeg_encode_cpu.py checks that the committed file is what this produces.

  python tools/make_jpeg_encode_golden.py          # needs Pillow

Members: `params` int64 (n, 6) = height, width, channels, quality, subsampling (0 = 4:4:4, 1 =
4:2:2, 2 = 4:2:0; grey ignores it), restart interval in MCUs (-1 = one MCU row); `file_<i>` the
file of case i; `pixels_<H>x<W>x<C>` the picture every case of that shape encodes."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _jpeg_encode_ref as E   # noqa: E402  (the test pictures only)

PATH = os.path.join(ROOT, 'tests', 'golden', 'jpeg_encode_fixtures.npz')
SIZES = [(1, 1), (2, 3), (8, 8), (8, 17), (9, 20), (20, 9), (33, 47), (40, 40), (17, 250), (64, 96)]
SUBSAMPLINGS = ['4:4:4', '4:2:2', '4:2:0']
KINDS = ['mixed', 'noise', 'smooth', 'mixed', 'noise', 'mixed', 'mixed', 'smooth', 'mixed', 'smooth']


def cases():
  """(height, width, channels, quality, subsampling index, restart) of every case."""
  out = []
  for h, w in SIZES:
    for q in (1, 50, 75, 100):
      out.append((h, w, 1, q, 2, 0))
      out += [(h, w, 3, q, s, 0) for s in range(3)]
  for h, w in ((33, 47), (40, 72)):
    for restart in (1, 2, -1, 65535):
      out += [(h, w, 3, 75, 2, restart), (h, w, 1, 50, 2, restart)]
    out.append((h, w, 3, 100, 0, 1))
  return out


def pixels(h, w, c):
  kind = KINDS[SIZES.index((h, w))] if (h, w) in SIZES else 'mixed'
  return E.scene(kind, h, w, c, seed=1000 * h + w)


def pillow_file(px, quality, sub, restart):
  from PIL import Image
  kw = {} if px.shape[2] == 1 else {'subsampling': SUBSAMPLINGS[sub]}
  if restart == -1:
    kw['restart_marker_rows'] = 1
  elif restart:
    kw['restart_marker_blocks'] = restart
  buf = io.BytesIO()
  Image.fromarray(px[..., 0] if px.shape[2] == 1 else px).save(buf, 'JPEG', quality=quality, **kw)
  return buf.getvalue()


def build():
  members = {'params': np.array(cases(), np.int64)}
  for i, (h, w, c, q, sub, restart) in enumerate(cases()):
    key = f'pixels_{h}x{w}x{c}'
    if key not in members:
      members[key] = pixels(h, w, c)
    members[f'file_{i}'] = np.frombuffer(pillow_file(members[key], q, sub, restart), np.uint8)
  return members


if __name__ == '__main__':
  np.savez_compressed(PATH, **build())
  print(PATH, os.path.getsize(PATH), 'bytes,', len(cases()), 'cases')
