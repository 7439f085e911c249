"""Writes tests/golden/jpeg_fixtures.npz: a dozen small JPEG files written by Pillow (libjpeg-turbo)
with the pixels Pillow decodes from them, so that tests/test_jpeg_cpu.py can pin the oracle's
arithmetic where Pillow is not installed.  Run from the repository root:

  python tests/golden/make_jpeg_fixtures.py
"""
import io
import os

import numpy as np
from PIL import Image

CASES = [   # name, height, width, save options (grey=True: one component)
    ('grey_9x17_q95', 9, 17, dict(grey=True, quality=95)),
    ('grey_1x1_q30', 1, 1, dict(grey=True, quality=30)),
    ('444_17x33_q95', 17, 33, dict(subsampling=0, quality=95)),
    ('444_2x3_q100', 2, 3, dict(subsampling=0, quality=100)),
    ('422_5x4_q95', 5, 4, dict(subsampling=1, quality=95)),
    ('422_33x6_q30', 33, 6, dict(subsampling=1, quality=30)),
    ('422_40x2_q100', 40, 2, dict(subsampling=1, quality=100)),
    ('420_3x5_q95', 3, 5, dict(subsampling=2, quality=95)),
    ('420_64x48_q30', 64, 48, dict(subsampling=2, quality=30)),
    ('420_17x33_opt', 17, 33, dict(subsampling=2, quality=95, optimize=True)),
    ('420_33x40_rst1', 33, 40, dict(subsampling=2, quality=95, restart_marker_blocks=1)),
    ('422_24x40_rstrow', 24, 40, dict(subsampling=1, quality=100, restart_marker_rows=1)),
]


def make(name, height, width, options, rng):
  options = dict(options)
  grey = options.pop('grey', False)
  a = rng.integers(0, 256, (height, width) if grey else (height, width, 3), dtype=np.uint8)
  if options.get('quality') == 30:
    a = (a // 64 * 64).astype(np.uint8)
  buf = io.BytesIO()
  Image.fromarray(a).save(buf, 'JPEG', **options)
  data = buf.getvalue()
  pixels = np.asarray(Image.open(io.BytesIO(data)))
  return data, pixels.reshape(height, width, -1)


def main():
  rng = np.random.default_rng(2024)
  arrays = {}
  for name, height, width, options in CASES:
    data, pixels = make(name, height, width, options, rng)
    arrays['file_' + name] = np.frombuffer(data, np.uint8)
    arrays['pixels_' + name] = pixels
  out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_fixtures.npz')
  np.savez_compressed(out, **arrays)
  print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
  main()
