"""Paired image metrics on the device: how close a generated frame is to ITS ground-truth frame
(kernels: csrc/image_metrics.hip).

  psnr(a, b, max_val)                20 log10(max_val) - 10 log10(mean (a - b)^2)
  ssim(a, b, max_val, ...)           tf.image.ssim: Gaussian VALID window, mean over the map and channels
  ssim_multiscale(a, b, max_val, ...)   tf.image.ssim_multiscale: the cs of every scale but the last, the
                                     ssim of the last, each to its power factor
  sqdiff_sum, ssim_per_channel, downsample2_sym   the pieces, as the library computes them

a and b are (N, H, W, C) device tensors, both float32 or both uint8, C in 1..4.  Every sum is
binary64 in a fixed order: the same input gives the same bits.  Results are float64 device tensors;
nothing waits for the device.  All argument errors are ValueError and are raised before the library
is touched; a CPU tensor raises `_lib.Se3dsHipError` after them: there is no CPU fallback.

Not here: LPIPS, gradients, TensorFlow's fp32 rounding, more than 4 channels,
filter_size > 15."""
from typing import Sequence

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd.utils.utils import _workspace   # per purpose, device and stream; grown on demand

MAX_CHANNELS = 4
MAX_FILTER_SIZE = 15
MAX_SIDE = 32768
MAX_IMAGES = 65535
POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_DTYPES = (torch.float32, torch.uint8)

_taps = {}         # (filter_size, filter_sigma) -> fp32 taps, host


def gaussian_taps(filter_size: int = 11, filter_sigma: float = 1.5) -> np.ndarray:
  """exp(-(i - (fs - 1) / 2)^2 / (2 sigma^2)), normalised in binary64, rounded to fp32 (host)."""
  if int(filter_size) != filter_size or not 1 <= filter_size <= MAX_FILTER_SIZE:
    raise ValueError(f'filter_size: an integer in 1..{MAX_FILTER_SIZE} is needed, got {filter_size!r}')
  if not filter_sigma > 0:
    raise ValueError(f'filter_sigma: a positive number is needed, got {filter_sigma!r}')
  key = (int(filter_size), float(filter_sigma))
  taps = _taps.get(key)
  if taps is None:
    d = np.arange(key[0], dtype=np.float64) - (key[0] - 1) / 2
    g = np.exp(-(d * d) / (2.0 * key[1] * key[1]))
    taps = _taps[key] = np.ascontiguousarray((g / g.sum()).astype(np.float32))
  return taps


def _check_images(x, name):
  if not isinstance(x, torch.Tensor):
    raise ValueError(f'{name}: a torch tensor is needed, got {type(x).__name__}')
  if x.dim() != 4:
    raise ValueError(f'{name}: (N, H, W, C) is needed, got {tuple(x.shape)}')
  if x.dtype not in _DTYPES:
    raise ValueError(f'{name}: unsupported dtype {x.dtype} (float32 or uint8)')
  n, h, w, c = x.shape
  if not 1 <= c <= MAX_CHANNELS:
    raise ValueError(f'{name}: 1..{MAX_CHANNELS} channels are supported, got {c}')
  if not 1 <= n <= MAX_IMAGES or not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_SIDE:
    raise ValueError(f'{name}: 1..{MAX_IMAGES} images with sides in 1..{MAX_SIDE} are supported, got '
                     f'{tuple(x.shape)}')


def _check_pair(a, b, max_val=None):
  _check_images(a, 'a')
  _check_images(b, 'b')
  if a.shape != b.shape or a.dtype != b.dtype:
    raise ValueError(f'b: {tuple(b.shape)} {b.dtype} against an a of {tuple(a.shape)} {a.dtype}')
  if max_val is not None and not max_val > 0:
    raise ValueError(f'max_val: a positive number is needed, got {max_val!r}')


def _check_side(h, w, filter_size, scale=None):
  if h < filter_size or w < filter_size:
    where = '' if scale is None else f'scale {scale}: '
    raise ValueError(f'{where}a {h} x {w} image is smaller than the {filter_size} x {filter_size} window')


def sqdiff_sum(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
  """(N,) float64: the sum of (a - b)^2 over each image, binary64 terms in a fixed order; exact for
  uint8."""
  _check_pair(a, b)
  _lib.require_cuda(a, b)
  a, b = a.contiguous(), b.contiguous()
  n = a.shape[0]
  elems = a.numel() // n
  L = _lib.lib()
  dev = a.device
  with torch.cuda.device(dev):
    out = torch.empty((n,), dtype=torch.float64, device=dev)
    ws = _workspace('image_metrics', dev, int(L.se3ds_sqdiff_workspace_bytes(n, elems)))
    _lib.check(L.se3ds_sqdiff_sum(a.data_ptr(), b.data_ptr(), _lib.dtype_code(a), n, elems, out.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream()), 'sqdiff_sum')
  return out


def psnr(a: torch.Tensor, b: torch.Tensor, max_val: float) -> torch.Tensor:
  """(N,) float64: 20 log10(max_val) - 10 log10(mse); +inf for identical images."""
  _check_pair(a, b, max_val)
  elems = a.numel() // a.shape[0]
  mse = sqdiff_sum(a, b) / elems
  return 20.0 * float(np.log10(max_val)) - 10.0 * torch.log10(mse)


def ssim_per_channel(a: torch.Tensor, b: torch.Tensor, max_val: float, filter_size: int = 11,
                     filter_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03, return_map: bool = False):
  """(ssim_mean (N, C), cs_mean (N, C)) float64: the means of lum * cs and of cs over the
  (H - fs + 1) x (W - fs + 1) map; with return_map=True also the lum * cs map (N, H', W', C)."""
  _check_pair(a, b, max_val)
  taps = gaussian_taps(filter_size, filter_sigma)
  _check_side(a.shape[1], a.shape[2], filter_size)
  _lib.require_cuda(a, b)
  return _ssim(a.contiguous(), b.contiguous(), float(max_val), taps, float(k1), float(k2), return_map)


def _ssim(a, b, max_val, taps, k1, k2, return_map):
  n, h, w, c = a.shape
  fs = len(taps)
  L = _lib.lib()
  dev = a.device
  with torch.cuda.device(dev):
    ssim_mean = torch.empty((n, c), dtype=torch.float64, device=dev)
    cs_mean = torch.empty((n, c), dtype=torch.float64, device=dev)
    index_map = (torch.empty((n, h - fs + 1, w - fs + 1, c), dtype=torch.float64, device=dev)
                 if return_map else None)
    ws = _workspace('image_metrics', dev, int(L.se3ds_ssim_workspace_bytes(n, h, w, c, fs)))
    _lib.check(L.se3ds_ssim(a.data_ptr(), b.data_ptr(), _lib.dtype_code(a), n, h, w, c, taps.ctypes.data, fs,
                            max_val, k1, k2, ssim_mean.data_ptr(), cs_mean.data_ptr(), _lib.ptr(index_map),
                            ws.data_ptr(), ws.numel(), _lib.stream()), 'ssim')
  return (ssim_mean, cs_mean, index_map) if return_map else (ssim_mean, cs_mean)


def ssim(a: torch.Tensor, b: torch.Tensor, max_val: float, filter_size: int = 11, filter_sigma: float = 1.5,
         k1: float = 0.01, k2: float = 0.03, return_map: bool = False):
  """(N,) float64: the SSIM index of tf.image.ssim, the mean over the map and then over the channels.
  return_map=True: (ssim, map) with the lum * cs map (N, H - fs + 1, W - fs + 1, C) float64."""
  out = ssim_per_channel(a, b, max_val, filter_size, filter_sigma, k1, k2, return_map)
  value = out[0].mean(dim=1)
  return (value, out[2]) if return_map else value


def downsample2_sym(x: torch.Tensor) -> torch.Tensor:
  """(N, H, W, C) float32 or uint8 -> float32 (N, ceil(H / 2), ceil(W / 2), C): the 2 x 2 mean at
  stride 2; an odd side is first extended by repeating its last row or column."""
  _check_images(x, 'x')
  _lib.require_cuda(x)
  return _downsample(x.contiguous())


def _downsample(x):
  n, h, w, c = x.shape
  out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=torch.float32, device=x.device)
  with torch.cuda.device(x.device):
    _lib.check(_lib.lib().se3ds_downsample2_sym(x.data_ptr(), _lib.dtype_code(x), n, h, w, c, out.data_ptr(),
                                                _lib.stream()), 'downsample2_sym')
  return out


def ssim_multiscale(a: torch.Tensor, b: torch.Tensor, max_val: float,
                    power_factors: Sequence[float] = POWER_FACTORS, filter_size: int = 11,
                    filter_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03,
                    return_scales: bool = False):
  """(N,) float64: per channel prod_{k < M - 1} relu(cs_k)^w_k * relu(ssim_{M-1})^w_{M-1}, then the mean
  over the channels; scale k + 1 is downsample2_sym of scale k.  Every scale must hold the window:
  the default five scales need sides of at least 161.  return_scales=True: (value, [(ssim_mean,
  cs_mean) per scale])."""
  _check_pair(a, b, max_val)
  taps = gaussian_taps(filter_size, filter_sigma)
  factors = [float(p) for p in power_factors]
  if not factors:
    raise ValueError('power_factors: at least one scale is needed')
  h, w = a.shape[1], a.shape[2]
  for k in range(len(factors)):
    _check_side(h, w, filter_size, scale=k)
    h, w = (h + 1) // 2, (w + 1) // 2
  _lib.require_cuda(a, b)
  a, b = a.contiguous(), b.contiguous()
  scales, terms = [], []
  last = len(factors) - 1
  for k in range(len(factors)):
    s_mean, cs_mean = _ssim(a, b, float(max_val), taps, float(k1), float(k2), False)
    scales.append((s_mean, cs_mean))
    terms.append(s_mean if k == last else cs_mean)
    if k < last:
      a, b = _downsample(a), _downsample(b)
  # N * C * M scalars: float64 torch ops on the device
  stacked = torch.clamp(torch.stack(terms, dim=-1), min=0.0)
  weights = torch.tensor(factors, dtype=torch.float64, device=stacked.device)
  value = torch.prod(torch.pow(stacked, weights), dim=-1).mean(dim=1)
  return (value, scales) if return_scales else value
