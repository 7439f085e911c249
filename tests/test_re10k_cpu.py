"""RE10KImageDataset without a GPU: the crop-box arithmetic (the NumPy restatement against literals,
and csrc/re10k_box_core.h as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer against the restatement), the host draws and `_parse`.  The device runs
are tests/test_re10k_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _png_ref
import _re10k_ref
from _records import image_record
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.utils import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# (r0, r1, c0, c1, H, W, pad, x_shift, y_shift) -> [x_min, y_min, x_max, y_max]
LITERALS = [
    ((3, 14, 10, 30, 20, 40, 0.0, 0.0, 0.0), [9, 3, 31, 14]),
    ((3, 14, 10, 30, 20, 40, 0.07, 0.01, -0.02), [6, 1, 34, 15]),
    ((0, 19, 0, 39, 20, 40, -0.05, 0.0, 0.0), [2, 1, 36, 18]),
    ((9, 9, 17, 17, 20, 40, -0.05, 0.02, 0.02), [19, 10, 20, 11]),
]
# H = 20, the only visible row is 19, pad = -0.05: y_min = 20, y_max = 21
OUTSIDE_CASE = (19, 19, 5, 30, 20, 40, -0.05, 0.0, 0.0)


def test_box_literals():
  for args, want in LITERALS:
    assert _re10k_ref.box(*args) == (want, _re10k_ref.OK), args
  got, status = _re10k_ref.box(*OUTSIDE_CASE)
  assert status == _re10k_ref.OUTSIDE and got[1] == 20 and got[3] == 21
  assert _re10k_ref.box(20, -1, 40, -1, 20, 40, 0.0, 0.0, 0.0)[1] == _re10k_ref.BLANK


def test_fp32_division_does_not_round_trip():
  """trunc((i / n) * n) != i in fp32 for these i: the rows and columns a division that is not
  correctly rounded (a reciprocal multiply) gets wrong."""
  def off(n):
    i = np.arange(n, dtype=F32)
    q = (i / F32(n)).astype(F32)
    return np.flatnonzero(np.trunc((q * F32(n)).astype(F32)) != i).tolist()
  assert off(100) == [53, 59]
  assert off(200) == [53, 59, 105, 106, 117, 118]
  # and the box on such an extent, pad and shifts 0: the row before it
  assert _re10k_ref.box(53, 80, 20, 180, 100, 200, 0.0, 0.0, 0.0)[0][1] == 52


def _rows(seed=7, count=4000):
  rng = np.random.default_rng(seed)
  rows = [a for a, _ in LITERALS] + [OUTSIDE_CASE, (20, -1, 40, -1, 20, 40, 0.05, 0.0, 0.0)]
  rows += [(i, 99, j, 199, 100, 200, 0.0, 0.0, 0.0) for i in (53, 59) for j in (53, 105, 118)]
  while len(rows) < count:
    h = int(rng.choice([1, 8, 20, 72, 100, 512, 1024]))
    w = 2 * h
    r0, r1 = sorted(int(v) for v in rng.integers(0, h, 2))
    c0, c1 = sorted(int(v) for v in rng.integers(0, w, 2))
    if rng.uniform() < 0.05:
      r0, r1, c0, c1 = h, -1, w, -1
    pad = F32(rng.choice([rng.uniform(-0.05, 0.1), -0.05, 0.0, 0.1]))
    half = F32(0.5) * np.abs(pad)
    xs, ys = (F32(rng.choice([rng.uniform(-half, half), -half, half])) for _ in range(2))
    rows.append((r0, r1, c0, c1, h, w, float(pad), float(xs), float(ys)))
  return rows


def test_box_core_as_a_sanitised_host_program(tmp_path):
  """csrc/re10k_box_core.h, the function the gather kernel calls, compiled as plain C++ with both
  sanitizers (reports are fatal) on 4000 seeded rows: boxes and statuses equal the restatement's.
  No sanitizer touches code loaded into Python."""
  cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
              if c and os.path.exists(c)), None)
  assert cxx, 'no C++ compiler: the box arithmetic cannot be checked on the host'
  exe = str(tmp_path / 're10k_box_check')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
  b = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off',
                      '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
                      '-Werror'] + static +
                     [os.path.join(ROOT, 'tools', 're10k_box_check.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  rows = _rows()
  bits = lambda v: format(int(np.array(v, F32).view(np.uint32)), 'x')
  text = ''.join(' '.join([str(i) for i in r[:6]] + [bits(v) for v in r[6:]]) + '\n' for r in rows)
  r = subprocess.run([exe], input=text, capture_output=True, text=True)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr
  got = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
  assert len(got) == len(rows) == 4000
  statuses = set()
  for row, g in zip(rows, got):
    want, status = _re10k_ref.box(*row)
    assert g == want + [status], row
    statuses.add(status)
  assert statuses == {0, 1, 2}
  # a malformed row is refused, not read as zeros
  r = subprocess.run([exe], input='1 2 3\n', capture_output=True, text=True)
  assert r.returncode == 2 and 'malformed' in r.stderr


# ------------------------------------------------------------------------------------ draws
class _Recorder:
  """A generator that records its calls and answers with the middle of the range."""

  def __init__(self):
    self.calls = []

  def uniform(self, low=0.0, high=1.0):
    self.calls.append((float(low), float(high)))
    return 0.5 * (low + high) if high != low else low

  def integers(self, *a, **k):
    raise AssertionError('the RE10K transform draws no integer')


def test_draw_order_and_ranges():
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=20,
                                         horizontal_mask_ratio=0.5, vertical_mask_ratio=0.25,
                                         re_10k_crop=True, pad_minval=-0.05, pad_maxval=0.1)
  rec = _Recorder()
  prm = ds.draw_params(rec, 20, 40)
  pad = F32(0.5 * (-0.05 + 0.1))
  half = float(F32(0.5) * np.abs(pad))
  # hmask ratio, hmask start, vmask ratio, vmask start, pad, x_shift, y_shift
  assert rec.calls[:3] == [(0.0, 0.5), (0.0, 40.0), (0.0, 0.25)]
  image_height = F32(20) * (F32(1) - F32(0.125))
  assert rec.calls[3] == (0.0, float(F32(20) - image_height))
  assert rec.calls[4:] == [(-0.05, 0.1), (-half, half), (-half, half)] and len(rec.calls) == 7
  assert set(prm) == {'hmask', 'vmask', 'pad', 'x_shift', 'y_shift'}
  assert prm['pad'] == float(pad) and prm['x_shift'] == 0.0 and prm['y_shift'] == 0.0
  start = F32(20.0)
  end = F32(np.mod(start + F32(40) * (F32(1) - F32(0.25)), F32(40)))
  assert prm['hmask'] == (2, float(start), float(end))
  vstart = F32(0.5 * float(F32(20) - image_height))
  assert prm['vmask'] == (float(vstart), float(vstart + image_height))
  # every value is an fp32 number
  real = ds.draw_params(np.random.default_rng(3), 20, 40)
  for v in (real['pad'], real['x_shift'], real['y_shift']) + real['hmask'][1:] + real['vmask']:
    assert float(F32(v)) == v
  assert -0.05 <= real['pad'] < 0.1 and abs(real['x_shift']) <= 0.5 * abs(real['pad'])
  assert abs(real['y_shift']) <= 0.5 * abs(real['pad'])


def test_draws_leave_the_generator_alone_for_what_is_off():
  ds = indoor_datasets.RE10KImageDataset(horizontal_mask_ratio=0.0, vertical_mask_ratio=0.0,
                                         re_10k_crop=False)
  rng = np.random.default_rng(5)
  before = rng.bit_generator.state
  prm = ds.draw_params(rng, 20, 40)
  assert rng.bit_generator.state == before
  assert prm == dict(hmask=None, vmask=None, pad=None, x_shift=None, y_shift=None)
  # the reference's default: re_10k_crop is off and no pad is drawn
  ds = indoor_datasets.RE10KImageDataset()
  assert ds.re_10k_crop is False and ds.random_crop is True
  rec = _Recorder()
  prm = ds.draw_params(rec, 20, 40)
  assert len(rec.calls) == 4 and prm['pad'] is None and prm['hmask'] and prm['vmask']
  # random_crop does not gate the draw (:419 tests re_10k_crop alone)
  rec = _Recorder()
  indoor_datasets.RE10KImageDataset(re_10k_crop=True, random_crop=False).draw_params(rec, 20, 40)
  assert len(rec.calls) == 7


# ------------------------------------------------------------------------------------ _parse
def _record(rng, mask=None, **overrides):
  mask = rng.integers(0, 3, (8, 16), dtype=np.uint8) if mask is None else mask
  feats = {'image/visible_mask': _png_ref.encode_png(mask, [int(f) for f in rng.integers(0, 5, 8)])}
  feats.update(overrides)
  rec, pix = image_record(8, rng, dataset_type=np.array([2]), **feats)
  return rec, pix, mask


def test_parse_reads_visible_mask():
  rng = np.random.default_rng(12)
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=8)
  rec, pix, mask = _record(rng, **{'image/blurred_mask': b''})   # not read: may be empty
  for inflate, kind in (('host', png.PngPlane), ('device', png.PngStream)):
    out = ds._parse(rec, inflate)
    assert set(out) == set(indoor_datasets.RE10K_RAW_DTYPES) | {'dataset_type', 'depth_scale', 'bbox'}
    assert 'blurred_mask' not in out and 'visible_mask' in out and out['dataset_type'] == 2
    assert all(isinstance(out[k], kind) for k in indoor_datasets.RE10K_RAW_DTYPES)
  out = ds._parse(rec)
  for name, (_, channels, depth) in indoor_datasets.RE10K_IMAGE_PLANES.items():
    p = out[name]
    assert (p.height, p.width, p.channels, p.bit_depth) == (8, 16, channels, depth)
    want = mask if name == 'visible_mask' else pix[name]
    assert (_png_ref.decode_png(p.filtered, 8, 16, depth, channels) == want).all(), name
  assert list(indoor_datasets.RE10K_RAW_DTYPES) == [
      'visible_mask' if k == 'blurred_mask' else k for k in indoor_datasets.RAW_DTYPES]
  # the base class still refuses the same record, and its tables did not move
  with pytest.raises(NotImplementedError, match='RE10K'):
    indoor_datasets.R2RImageDataset(image_size=4, preprocessed_image_height=8)._parse(rec)
  assert 'blurred_mask' in indoor_datasets.R2RImageDataset.RAW_DTYPES
  assert indoor_datasets.R2RImageDataset.IMAGE_PLANES is indoor_datasets.IMAGE_PLANES


def test_parse_errors():
  rng = np.random.default_rng(13)
  ds = indoor_datasets.RE10KImageDataset(image_size=4, preprocessed_image_height=8)
  rec, _ = image_record(8, rng)   # an MP3D record
  with pytest.raises(ValueError, match='dataset_type 0'):
    ds._parse(rec)
  rec, _ = image_record(8, rng, dataset_type=np.array([2]))   # no visible_mask: the default ''
  with pytest.raises(ValueError, match='^image/visible_mask: '):
    ds._parse(rec)
  rgb = _png_ref.encode_png(rng.integers(0, 256, (8, 16, 3), dtype=np.uint8), [0] * 8)
  rec, _, _ = _record(rng, **{'image/visible_mask': rgb})   # wrong kind
  with pytest.raises(ValueError, match='^image/visible_mask: 3 channel'):
    ds._parse(rec)
  small = _png_ref.encode_png(rng.integers(0, 2, (4, 8), dtype=np.uint8), [0] * 4)
  rec, _, _ = _record(rng, **{'image/visible_mask': small})
  with pytest.raises(ValueError, match='^image/visible_mask: a 4x8 plane'):
    ds._parse(rec)
