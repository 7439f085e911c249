"""The paired image metrics without a GPU: the oracle of tests/_image_metrics_ref.py against itself
and against known answers, and every refusal utils/image_metrics.py raises before it touches the
library."""
import math

import numpy as np
import pytest
import torch

import _image_metrics_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import image_metrics as im

TAPS = R.gaussian_taps()


def _cases():
  rng = np.random.default_rng(11)
  return {
      'noise 23x37x3': (R.noise((1, 23, 37, 3), 1), R.noise((1, 23, 37, 3), 2), 1.0),
      'smooth + noise 40x52x3': (R.smooth_noise((1, 40, 52, 3), 3, 0.0), R.smooth_noise((1, 40, 52, 3), 3, 0.1), 1.0),
      'flat 0.7 16x16x1': R.flat_pair_f32() + (1.0,),
      'uint8 255 vs 254 12x13x1': R.flat_pair_u8() + (255.0,),
      'uint8 random 14x19x4': (rng.integers(0, 256, (2, 14, 19, 4)).astype(np.uint8),
                               rng.integers(0, 256, (2, 14, 19, 4)).astype(np.uint8), 255.0),
  }


@pytest.mark.parametrize('name', list(_cases()))
def test_separable_and_direct_window_agree(name):
  """(i) against (ii) on the map.  1e-10: at most 1.2e-12 was measured over these cases (the worst is
  uint8 255 against 254, where d1 - d0 cancels to the last few digits)."""
  a, b, max_val = _cases()[name]
  sep, sep_cs = R.ssim_separable(a, b, max_val, TAPS)
  direct, direct_cs = R.ssim_direct(a, b, max_val, TAPS)
  assert sep.shape == (a.shape[0], a.shape[1] - 10, a.shape[2] - 10, a.shape[3])
  print(name, float(np.abs(sep - direct).max()), float(np.abs(sep_cs - direct_cs).max()))
  assert np.abs(sep - direct).max() <= 1e-10
  assert np.abs(sep_cs - direct_cs).max() <= 1e-10


def test_identical_inputs():
  for a, max_val in ((R.noise((2, 15, 17, 3), 5), 1.0), (R.flat_pair_u8()[0], 255.0)):
    index, cs = R.ssim_separable(a, a, max_val, TAPS)
    assert np.array_equal(index, np.ones_like(index)) and np.array_equal(cs, np.ones_like(cs))
    assert np.array_equal(R.psnr(a, a, max_val), np.full(a.shape[0], np.inf))


def test_constant_images():
  """Constants p, q: both variances and the covariance vanish, cs = 1 and the index is the luminance
  term (2 p q + c1) / (p^2 + q^2 + c1) -- for a window that sums to exactly 1.  With a window sum
  s = 1 - e the variance term is (p^2 + q^2) s (1 - s) and the index moves by about
  (p - q)^2 e / c2: the fp32 Gaussian taps have e = 2.8e-9 over the 2-D window, so with them the
  answer holds to 1e-12 only where (p - q)^2 < 3e-7 max_val^2 (0.25 against 0.75 is 4.7e-7 off,
  as TensorFlow's own result is).  Arbitrary p, q are therefore checked with windows that sum to
  exactly 1, the binomial taps and filter_size 1, and the Gaussian taps with a near-equal pair."""
  binomial = np.array([1, 4, 6, 4, 1], np.float32) / 16
  one = np.ones(1, np.float32)
  near = 0.5 + 2.0 ** -14
  for p, q, max_val, taps in ((0.25, 0.75, 1.0, binomial), (0.7, 0.7009765625, 1.0, binomial),
                              (255.0, 254.0, 255.0, binomial), (0.25, 0.75, 1.0, one), (255.0, 254.0, 255.0, one),
                              (0.5, near, 1.0, TAPS), (near, 0.5, 1.0, R.gaussian_taps(8, 1.0))):
    a, b = np.full((1, 13, 12, 2), p, np.float32), np.full((1, 13, 12, 2), q, np.float32)
    c1 = (0.01 * max_val) ** 2
    want = (2 * p * q + c1) / (p * p + q * q + c1)
    assert want < 1.0 - 1e-9
    index, _ = R.ssim_separable(a, b, max_val, taps)
    assert np.abs(index - want).max() <= 1e-12
    assert np.abs(R.map_means(index) - want).max() <= 1e-12


def test_psnr_of_a_constant_difference():
  for d, max_val, dtype in ((0.125, 1.0, np.float32), (3, 255.0, np.uint8)):
    a = np.full((2, 5, 7, 3), 16 * d, dtype)
    b = np.full((2, 5, 7, 3), 17 * d, dtype)
    want = 20 * math.log10(max_val) - 10 * math.log10(float(d) ** 2)
    assert np.abs(R.psnr(a, b, max_val) - want).max() <= 1e-12 * abs(want)
  assert np.array_equal(R.sqdiff_sum(np.full((1, 2, 2, 1), 255, np.uint8), np.zeros((1, 2, 2, 1), np.uint8)),
                        [4 * 65025.0])


@pytest.mark.parametrize('fs,sigma', [(11, 1.5), (8, 1.0), (1, 1.5), (15, 4.0)])
def test_taps(fs, sigma):
  taps = R.gaussian_taps(fs, sigma)
  assert taps.dtype == np.float32 and taps.shape == (fs,)
  assert np.array_equal(taps, im.gaussian_taps(fs, sigma))            # the module's own, bit for bit
  assert np.array_equal(taps, taps[::-1]) or fs == 1
  assert abs(math.fsum(taps.astype(np.float64).tolist()) - 1.0) <= fs * 2.0 ** -24   # one fp32 ulp a tap


def test_downsample_and_multiscale_oracle():
  x = np.arange(2 * 3 * 5 * 1, dtype=np.float32).reshape(2, 3, 5, 1)
  y = R.downsample2_sym(x)
  assert y.shape == (2, 2, 3, 1) and y.dtype == np.float32
  assert y[0, 0, 0, 0] == (0 + 1 + 5 + 6) / 4 and y[0, 0, 2, 0] == (4 + 4 + 9 + 9) / 4
  assert y[0, 1, 0, 0] == (10 + 11 + 10 + 11) / 4 and y[0, 1, 2, 0] == 14
  a = R.smooth_noise((1, 176, 183, 1), 9, 0.05)
  value, scales = R.ssim_multiscale(a, a, 1.0)
  assert value.shape == (1,) and abs(value[0] - 1.0) <= 1e-15 and len(scales) == 5
  assert scales[4][2] == 1 * 2        # 176 -> 11 rows, 183 -> 12 columns: a 1 x 2 map at the last scale


# ---------------------------------------------------------------------------------- refusals
def _pair(shape=(1, 16, 16, 3), dtype=torch.float32):
  return torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=dtype)


ALL = (lambda a, b, **kw: im.psnr(a, b, kw.get('max_val', 1.0)),
       lambda a, b, **kw: im.ssim(a, b, kw.get('max_val', 1.0)),
       lambda a, b, **kw: im.ssim_multiscale(a, b, kw.get('max_val', 1.0)))


@pytest.mark.parametrize('fn', ALL)
def test_refusals_common_to_all(fn, monkeypatch):
  def no_library():
    raise AssertionError('an argument error must be raised before the library is loaded')
  monkeypatch.setattr(_lib, 'lib', no_library)
  a, b = _pair((1, 200, 200, 3))
  with pytest.raises(ValueError):
    fn(a, b[:, :199])                                       # shapes differ
  with pytest.raises(ValueError):
    fn(a[0], b[0])                                          # not 4-D
  with pytest.raises(ValueError):
    fn(a, b.to(torch.uint8))                                # dtypes differ
  with pytest.raises(ValueError):
    fn(a.double(), b.double())                              # neither float32 nor uint8
  with pytest.raises(ValueError):
    fn(a.to(torch.int32), b.to(torch.int32))
  with pytest.raises(ValueError):
    fn(*_pair((1, 200, 200, 5)))                            # c outside 1..4
  with pytest.raises(ValueError):
    fn(*_pair((1, 200, 200, 0)))
  with pytest.raises(ValueError):
    fn(a, b, max_val=0.0)
  with pytest.raises(ValueError):
    fn(a, b, max_val=-1.0)
  with pytest.raises(ValueError):
    fn(a.numpy(), b.numpy())
  # valid arguments on CPU tensors: refused as the other wrappers refuse them, still without the library
  with pytest.raises(_lib.Se3dsHipError):
    fn(a, b)
  with pytest.raises(_lib.Se3dsHipError):
    fn(a.to(torch.uint8), b.to(torch.uint8), max_val=255.0)


def test_ssim_refuses_a_side_below_the_window(monkeypatch):
  monkeypatch.setattr(_lib, 'lib', lambda: (_ for _ in ()).throw(AssertionError('library loaded')))
  with pytest.raises(ValueError, match='smaller than the 11 x 11 window'):
    im.ssim(*_pair((1, 10, 16, 3)), 1.0)
  with pytest.raises(ValueError, match='smaller than the 11 x 11 window'):
    im.ssim(*_pair((1, 16, 10, 3)), 1.0)
  with pytest.raises(ValueError):
    im.ssim(*_pair((1, 7, 7, 1)), 1.0, filter_size=8, filter_sigma=1.0)
  for bad in (0, 16, 2.5):
    with pytest.raises(ValueError, match='filter_size'):
      im.ssim(*_pair(), 1.0, filter_size=bad)
  with pytest.raises(ValueError, match='filter_sigma'):
    im.ssim(*_pair(), 1.0, filter_sigma=0.0)
  with pytest.raises(_lib.Se3dsHipError):
    im.ssim(*_pair((1, 11, 11, 1)), 1.0)                    # 11 x 11 holds one window


def test_multiscale_names_the_scale_that_is_too_small(monkeypatch):
  monkeypatch.setattr(_lib, 'lib', lambda: (_ for _ in ()).throw(AssertionError('library loaded')))
  with pytest.raises(ValueError, match=r'scale 4: a 10 x 12 image'):
    im.ssim_multiscale(*_pair((1, 160, 183, 3)), 1.0)       # 160 -> 80 -> 40 -> 20 -> 10 < 11
  with pytest.raises(ValueError, match=r'scale 3: '):
    im.ssim_multiscale(*_pair((1, 176, 80, 3)), 1.0)        # 80 -> 40 -> 20 -> 10 at scale 3
  with pytest.raises(ValueError, match=r'scale 0: '):
    im.ssim_multiscale(*_pair((1, 8, 200, 3)), 1.0)
  with pytest.raises(ValueError, match='power_factors'):
    im.ssim_multiscale(*_pair((1, 176, 176, 3)), 1.0, power_factors=())
  with pytest.raises(_lib.Se3dsHipError):                   # 176 -> 88 -> 44 -> 22 -> 11: the shape check accepts it
    im.ssim_multiscale(*_pair((1, 176, 183, 3)), 1.0)
  with pytest.raises(_lib.Se3dsHipError):
    im.ssim_multiscale(*_pair((1, 22, 21, 1)), 1.0, power_factors=(0.5, 0.5))   # 11 x 11 at scale 1


def test_declarations_and_build_flags():
  from se3ds_amd.csrc import build as hip_build
  assert hip_build.PER_FILE['image_metrics.hip'] == ['-ffp-contract=off']
  c_int, c_p, c_d, c_sz, c_i64 = _lib.c_int, _lib.c_p, _lib.c_d, _lib.c_sz, _lib.c_i64
  assert _lib._SIGS['se3ds_ssim'] == (c_int, [c_p, c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_int, c_d, c_d,
                                              c_d, c_p, c_p, c_p, c_p, c_sz, c_p])
  assert _lib._SIGS['se3ds_ssim_workspace_bytes'] == (c_sz, [c_int] * 5)
  assert _lib._SIGS['se3ds_sqdiff_sum'] == (c_int, [c_p, c_p, c_int, c_int, c_i64, c_p, c_p, c_sz, c_p])
  assert _lib._SIGS['se3ds_downsample2_sym'] == (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p])
