"""utils/png.py on the host (the container, the inflate, every rejection) and the test-side
reference tests/_png_ref.py itself, pinned by literals worked out on paper from the PNG
specification's definitions -- not by running either implementation."""
import struct
import zlib

import numpy as np
import pytest

import _png_ref
from se3ds_amd.trainers import gan_manager
from se3ds_amd.utils import png

# The 3 x 3 grey image every literal below encodes, one filter type on all three rows.
IMAGE = [[10, 20, 30], [40, 60, 50], [200, 100, 250]]
# Worked by hand (a = left, b = above, c = above-left, 0 outside; Filt = Orig - pred mod 256):
#  Sub      row 1: 40-0, 60-40, 50-60 = -10 -> 246;  row 2: 200, 100-200 -> 156, 250-100
#  Up       row 1: 40-10, 60-20, 50-30;              row 2: 200-40, 100-60, 250-50
#  Average  row 0: pred 0, 5, 10;  row 1: (0+10)>>1 = 5, (40+20)>>1 = 30, (60+30)>>1 = 45
#           row 2: (0+40)>>1 = 20, (200+60)>>1 = 130 (a 9-bit sum) -> 100-130 = 226, (100+50)>>1 = 75
#  Paeth    row 0: pred = a;  row 1: (0,10,0) -> b = 10, (40,20,10): p = 50, pa = 10 -> a,
#           (60,30,20): p = 70, pa = 10 -> a;  row 2: (0,40,0) -> b = 40, (200,60,40): p = 220,
#           pa = 20 -> a, (100,50,60): p = 90, pa = 10, pb = 40, pc = 30 -> a
FILTERED = {
    0: [[10, 20, 30], [40, 60, 50], [200, 100, 250]],
    1: [[10, 10, 10], [40, 20, 246], [200, 156, 150]],
    2: [[10, 20, 30], [30, 40, 20], [160, 40, 200]],
    3: [[10, 15, 20], [35, 30, 5], [180, 226, 175]],
    4: [[10, 10, 10], [30, 20, 246], [160, 156, 150]],
}


def _stream(ft):
  return bytes(b for row in FILTERED[ft] for b in [ft] + row)


@pytest.mark.parametrize('ft', [0, 1, 2, 3, 4])
def test_reference_matches_hand_worked_literals(ft):
  assert _png_ref.reconstruct(_stream(ft), 3, 3, 1).tolist() == IMAGE
  assert _png_ref.apply_filters(np.array(IMAGE, np.uint8), [ft] * 3, 1) == _stream(ft)


def test_reference_paeth_ties_and_the_c_branch():
  # pb == pc < pa: (a, b, c) = (12, 6, 10): p = 8, pa = 4, pb = 2, pc = 2 -> b, not c
  assert _png_ref.paeth_predictor(12, 6, 10) == 6
  # pa == pc < pb: (6, 12, 10): p = 8, pa = 2, pb = 4, pc = 2 -> a, not c
  assert _png_ref.paeth_predictor(6, 12, 10) == 6
  # all equal -> a;  c wins only when strictly closest: (100, 50, 75): p = 75, pc = 0
  assert _png_ref.paeth_predictor(7, 7, 7) == 7
  assert _png_ref.paeth_predictor(100, 50, 75) == 75
  # the tie as an image: [[10, 6], [12, 20]] under Paeth.  Row 0: 10, 6 - 10 = 252.  Row 1:
  # (0, 10, 0) -> b = 10: 12 - 10 = 2; (12, 6, 10) -> b = 6: 20 - 6 = 14 (c would give 20 - 10).
  stream = bytes([4, 10, 252, 4, 2, 14])
  assert _png_ref.reconstruct(stream, 2, 2, 1).tolist() == [[10, 6], [12, 20]]
  # bytes per pixel 2: a and c are two bytes back.  Sub on [1, 2, 3, 4]: 1, 2, 3 - 1, 4 - 2
  assert _png_ref.reconstruct(bytes([1, 1, 2, 2, 2]), 1, 4, 2).tolist() == [[1, 2, 3, 4]]
  assert _png_ref.decode_png(bytes([0, 1, 2]), 1, 1, 16, 1).tolist() == [[258]]


# ---------------------------------------------------------------------------------- container
def test_encode_png_output_parses():
  rng = np.random.default_rng(0)
  for c in (1, 3):
    pixels = rng.integers(0, 256, (5, 7, c), dtype=np.uint8)
    plane = png.parse_png(gan_manager._encode_png(pixels))
    assert plane[:4] == (5, 7, 8, c) and plane.row_bytes == 7 * c and plane.bytes_per_pixel == c
    rows = np.frombuffer(plane.filtered, np.uint8).reshape(5, 1 + 7 * c)
    assert (rows[:, 0] == 0).all() and (rows[:, 1:] == pixels.reshape(5, -1)).all()


def test_idat_chunks_are_concatenated_and_ancillary_chunks_ignored():
  rng = np.random.default_rng(1)
  pixels = rng.integers(0, 65536, (6, 9)).astype(np.uint16)
  one = png.parse_png(_png_ref.encode_png(pixels, [4, 3, 2, 1, 0, 4]))
  many = png.parse_png(_png_ref.encode_png(pixels, [4, 3, 2, 1, 0, 4], idat_split=5))
  assert _png_ref.encode_png(pixels, [0] * 6, idat_split=5).count(b'IDAT') == 5
  assert one == many and one[:4] == (6, 9, 16, 1) and one.bytes_per_pixel == 2
  assert (_png_ref.decode_png(many.filtered, 6, 9, 16, 1) == pixels).all()
  stream = _png_ref.apply_filters(_png_ref.raw_bytes(pixels), [1] * 6, 2)
  with_text = _png_ref.container(9, 6, 16, 0, stream, extra=[(b'tEXt', b'k\x00v'), (b'gAMA', bytes(4))])
  assert png.parse_png(with_text).filtered == stream


def _grey(width=3, height=2, depth=8, colour=0, bpp=1, **kw):
  return _png_ref.container(width, height, depth, colour, bytes(height * (1 + width * bpp)), **kw)


@pytest.mark.parametrize('depth,colour,bpp,name', [
    (8, 3, 1, 'palette'), (8, 4, 2, 'greyscale with alpha'), (8, 6, 4, 'truecolour with alpha'),
    (16, 6, 8, 'truecolour with alpha'), (4, 0, 1, 'bit depth 4'), (1, 0, 1, 'bit depth 1'),
    (16, 2, 6, 'truecolour at bit depth 16')])
def test_unsupported_kinds_name_the_kind(depth, colour, bpp, name):
  extra = [(b'PLTE', bytes(6))] if colour == 3 else []
  with pytest.raises(NotImplementedError, match=name):
    png.parse_png(_grey(depth=depth, colour=colour, bpp=bpp, extra=extra))


def test_interlaced_is_not_implemented():
  with pytest.raises(NotImplementedError, match='interlaced'):
    png.parse_png(_grey(interlace=1))


def test_malformed_inputs_raise_value_error():
  good = _grey()
  png.parse_png(good)
  bad = {
      'signature': b'\x89PNX' + good[4:],
      'empty': b'',
      'truncated': good[:-5],
      'no IEND': good[:-12],
      'chunk crc': good[:20] + bytes([good[20] ^ 1]) + good[21:],
      'no IHDR first': good[:8] + _png_ref.chunk(b'tEXt', b'a\x00b') + good[8:],
      'no IDAT': good[:33] + _png_ref.chunk(b'IEND', b''),
      'colour type 5': _grey(colour=5),
      'bit depth 3': _grey(depth=3),
      'rgb at depth 4': _grey(depth=4, colour=2),
      'zero width': _png_ref.container(0, 2, 8, 0, bytes(2)),
      'interlace 2': _grey(interlace=2),
      'unknown critical chunk': _grey(extra=[(b'ABCD', b'')]),
      'stream too short': _png_ref.container(3, 2, 8, 0, bytes(7)),
      'stream too long': _png_ref.container(3, 2, 8, 0, bytes(9)),
      'not zlib': good[:33] + _png_ref.chunk(b'IDAT', b'garbage!') + _png_ref.chunk(b'IEND', b''),
      'filter type 5': _png_ref.container(3, 2, 8, 0, bytes([0, 1, 2, 3, 5, 1, 2, 3])),
      'filter type 255': _png_ref.container(3, 2, 8, 0, bytes([255, 1, 2, 3, 0, 1, 2, 3])),
  }
  for what, buf in bad.items():
    with pytest.raises(ValueError):
      png.parse_png(buf)
      pytest.fail(f'{what}: accepted')
  ihdr_bad_len = good[:8] + _png_ref.chunk(b'IHDR', bytes(12)) + good[33:]
  with pytest.raises(ValueError):
    png.parse_png(ihdr_bad_len)
  # a data byte of 5 is no filter type: only the first byte of a scan line is checked
  assert png.parse_png(_png_ref.container(3, 2, 8, 0, bytes([0, 5, 5, 5, 4, 5, 5, 5]))).height == 2
