"""PSNR, SSIM and MS-SSIM restated from their published formulas (tf.image.psnr / ssim /
ssim_multiscale; Wang et al. 2004 and 2003) in NumPy binary64, for the tests of
se3ds_amd/utils/image_metrics.py and csrc/image_metrics.hip.

  ssim_separable   (i)  the window sum as the kernel states it: horizontal pass, then vertical pass,
                        taps ascending, the first tap a product and every later tap a product and an
                        add.  NumPy rounds every elementwise product and sum separately, so this is the
                        kernel's arithmetic bit for bit.
  ssim_direct      (ii) the same index from the 2-D outer-product window, an independent order.
  psnr, sqdiff_sum (iii)
  downsample2_sym, ssim_multiscale (iv)

Means are taken with math.fsum (exact, rounded once), so a bound on the kernel's summation error
does not have to carry the oracle's as well."""
import math

import numpy as np

POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gaussian_taps(filter_size=11, filter_sigma=1.5):
  """exp(-(i - (fs - 1) / 2)^2 / (2 sigma^2)), normalised in binary64, rounded to fp32."""
  i = np.arange(filter_size, dtype=np.float64)
  d = i - (filter_size - 1) / 2
  g = np.exp(-(d * d) / (2.0 * filter_sigma * filter_sigma))
  return (g / g.sum()).astype(np.float32)


def window_sum(x, taps):
  """x (n, h, w, c) binary64 -> (n, h - fs + 1, w - fs + 1, c): rows first, then columns."""
  w = np.asarray(taps, np.float32).astype(np.float64)
  fs = len(w)
  oh, ow = x.shape[1] - fs + 1, x.shape[2] - fs + 1
  acc = w[0] * x[:, :, 0:ow]
  for t in range(1, fs):
    acc = acc + w[t] * x[:, :, t:t + ow]
  out = w[0] * acc[:, 0:oh]
  for t in range(1, fs):
    out = out + w[t] * acc[:, t:t + oh]
  return out


def window_sum_direct(x, taps):
  """The same sum from the 2-D window taps[i] * taps[j], one term at a time."""
  w = np.asarray(taps, np.float32).astype(np.float64)
  window = np.outer(w, w)
  fs = len(w)
  oh, ow = x.shape[1] - fs + 1, x.shape[2] - fs + 1
  out = np.zeros((x.shape[0], oh, ow, x.shape[3]), np.float64)
  for i in range(fs):
    for j in range(fs):
      out += window[i, j] * x[:, i:i + oh, j:j + ow]
  return out


def _index(a, b, max_val, taps, k1, k2, reducer):
  a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
  l1, l2 = k1 * max_val, k2 * max_val
  c1, c2 = l1 * l1, l2 * l2
  m0, m1 = reducer(a, taps), reducer(b, taps)
  n0 = 2.0 * m0 * m1
  d0 = m0 * m0 + m1 * m1
  lum = (n0 + c1) / (d0 + c1)
  n1 = 2.0 * reducer(a * b, taps)
  d1 = reducer(a * a + b * b, taps)
  cs = (n1 - n0 + c2) / (d1 - d0 + c2)
  return lum * cs, cs


def ssim_separable(a, b, max_val, taps, k1=0.01, k2=0.03):
  """(lum cs map, cs map), each (n, h', w', c) binary64, in the kernel's order of operations."""
  return _index(a, b, max_val, taps, k1, k2, window_sum)


def ssim_direct(a, b, max_val, taps, k1=0.01, k2=0.03):
  return _index(a, b, max_val, taps, k1, k2, window_sum_direct)


def map_means(m):
  """(n, h', w', c) -> (n, c): exact sums over the map, rounded once, divided by the count."""
  n, oh, ow, c = m.shape
  return np.array([[math.fsum(m[i, :, :, k].ravel().tolist()) / (oh * ow) for k in range(c)]
                   for i in range(n)], np.float64)


def sqdiff_sum(a, b):
  """(n,) sums of (a - b)^2: Python integers for uint8 (exact), math.fsum of binary64 terms else."""
  a, b = np.asarray(a), np.asarray(b)
  n = a.shape[0]
  if a.dtype == np.uint8:
    d = a.reshape(n, -1).astype(np.int64) - b.reshape(n, -1).astype(np.int64)
    return np.array([int((row * row).sum()) for row in d], np.float64)
  d = a.reshape(n, -1).astype(np.float64) - b.reshape(n, -1).astype(np.float64)
  return np.array([math.fsum((row * row).tolist()) for row in d], np.float64)


def psnr(a, b, max_val):
  a = np.asarray(a)
  with np.errstate(divide='ignore'):
    mse = sqdiff_sum(a, b) / (a.size // a.shape[0])
    return 20.0 * np.log10(max_val) - 10.0 * np.log10(mse)


def downsample2_sym(x):
  """(n, h, w, c) -> fp32 (n, ceil(h / 2), ceil(w / 2), c): an odd side repeats its last line, then
  ((x00 + x01) + x10) + x11 in binary64, times 0.25, rounded once to fp32."""
  x = np.asarray(x).astype(np.float64)
  x = np.pad(x, ((0, 0), (0, x.shape[1] % 2), (0, x.shape[2] % 2), (0, 0)), mode='edge')
  s = ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2]
  return (s * 0.25).astype(np.float32)


def ssim_multiscale(a, b, max_val, power_factors=POWER_FACTORS, filter_size=11, filter_sigma=1.5, k1=0.01,
                    k2=0.03):
  """((n,) MS-SSIM, per-scale list of (ssim_mean (n, c), cs_mean (n, c), map size))."""
  taps = gaussian_taps(filter_size, filter_sigma)
  a, b = np.asarray(a), np.asarray(b)
  scales, factors = [], []
  last = len(power_factors) - 1
  for k in range(len(power_factors)):
    index, cs = ssim_separable(a, b, max_val, taps, k1, k2)
    s_mean, cs_mean = map_means(index), map_means(cs)
    scales.append((s_mean, cs_mean, index.shape[1] * index.shape[2]))
    factors.append(np.maximum(s_mean if k == last else cs_mean, 0.0))
    if k < last:
      a, b = downsample2_sym(a), downsample2_sym(b)
  per_channel = np.prod(np.stack(factors, -1) ** np.asarray(power_factors, np.float64), axis=-1)
  return per_channel.mean(axis=1), scales


# ------------------------------------------------------------------------------------ test content
def noise(shape, seed):
  return np.random.default_rng(seed).random(shape, dtype=np.float32)


def smooth_noise(shape, seed, level=0.05):
  """Smooth gradients and a few waves plus uniform noise of amplitude `level`, in [0, 1]."""
  n, h, w, c = shape
  rng = np.random.default_rng(seed)
  y = np.linspace(0.0, 1.0, h, dtype=np.float64)[None, :, None, None]
  x = np.linspace(0.0, 1.0, w, dtype=np.float64)[None, None, :, None]
  phase = rng.random((n, 1, 1, c)) * 6.0
  base = 0.5 + 0.25 * np.sin(7.0 * x + phase) * np.cos(5.0 * y + 0.5 * phase) + 0.2 * (x - y)
  return np.clip(base + level * (rng.random(shape) - 0.5), 0.0, 1.0).astype(np.float32)


def flat_pair_f32(h=16, w=16):
  """flat 0.7 against flat 0.7 + N(0, 1e-3), one channel."""
  rng = np.random.default_rng(3)
  a = np.full((1, h, w, 1), 0.7, np.float32)
  return a, (a + rng.normal(0.0, 1e-3, a.shape)).astype(np.float32)


def flat_pair_u8(h=12, w=13):
  """uint8 flat 255 against flat 254, one channel."""
  return np.full((1, h, w, 1), 255, np.uint8), np.full((1, h, w, 1), 254, np.uint8)
