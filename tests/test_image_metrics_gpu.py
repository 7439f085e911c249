"""PSNR, SSIM and MS-SSIM on the GPU (csrc/image_metrics.hip, utils/image_metrics.py) against the
binary64 restatement of tests/_image_metrics_ref.py: the SSIM map bit for bit, the means within the
bound of a binary64 sum in any order, the ABI's refusals, and the evaluator's opt-in scores."""
import csv
import os

import numpy as np
import pytest
import torch

import _image_metrics_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import image_metrics as im

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U = 2.0 ** -53


def _dev(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ssim_cases():
  """name -> (a, b, max_val, filter_size, filter_sigma).  Map sizes from the tile a workgroup owns."""
  L = _lib.lib()
  tr, tc = L.se3ds_ssim_tile_rows(), L.se3ds_ssim_tile_cols()
  assert tr >= 2 and tc >= 2
  sizes = {'1x1': (1, 1), 'one tile': (tr, tc), 'tile + 1': (tr + 1, tc + 1), 'two tiles - 1': (2 * tr - 1, 2 * tc - 1),
           'wide': (tr + 1, 3 * tc + 2)}
  cases = {}
  for s, (name, (mh, mw)) in enumerate(sizes.items()):
    h, w = mh + 10, mw + 10
    rng = np.random.default_rng(40 + s)
    cases[f'noise N=3 C=3 {name}'] = (R.noise((3, h, w, 3), 10 + s), R.noise((3, h, w, 3), 20 + s), 1.0, 11, 1.5)
    cases[f'smooth + noise C=1 {name}'] = (R.smooth_noise((2, h, w, 1), 30 + s, 0.0),
                                           R.smooth_noise((2, h, w, 1), 30 + s, 0.1), 1.0, 11, 1.5)
    cases[f'uint8 C=4 {name}'] = (rng.integers(0, 256, (2, h, w, 4)).astype(np.uint8),
                                  rng.integers(0, 256, (2, h, w, 4)).astype(np.uint8), 255.0, 11, 1.5)
  cases['flat 0.7'] = R.flat_pair_f32() + (1.0, 11, 1.5)
  cases['uint8 255 vs 254'] = R.flat_pair_u8() + (255.0, 11, 1.5)
  cases['even window'] = (R.noise((2, tr + 8, 2 * tc + 7, 3), 50), R.noise((2, tr + 8, 2 * tc + 7, 3), 51), 1.0, 8, 1.0)
  rng = np.random.default_rng(52)
  cases['window of one'] = (rng.integers(0, 256, (2, tr + 1, tc + 1, 4)).astype(np.uint8),
                            rng.integers(0, 256, (2, tr + 1, tc + 1, 4)).astype(np.uint8), 255.0, 1, 1.5)
  return cases


@pytest.fixture(scope='module')
def ssim_results():
  """name -> (oracle map, oracle cs map, device ssim_mean, cs_mean, map): every case once."""
  out = {}
  for name, (a, b, max_val, fs, sigma) in _ssim_cases().items():
    want, want_cs = R.ssim_separable(a, b, max_val, R.gaussian_taps(fs, sigma))
    s_mean, cs_mean, index_map = im.ssim_per_channel(_dev(a), _dev(b), max_val, fs, sigma, return_map=True)
    out[name] = (want, want_cs, s_mean.cpu().numpy(), cs_mean.cpu().numpy(), index_map.cpu().numpy())
  return out


def test_ssim_map_equals_the_oracle_bit_for_bit(ssim_results):
  assert len(ssim_results) == 15 + 4
  for name, (want, _, _, _, got) in ssim_results.items():
    assert got.shape == want.shape and got.dtype == np.float64, name
    assert np.array_equal(got, want), (name, float(np.abs(got - want).max()))
  assert ssim_results['noise N=3 C=3 1x1'][0].shape == (3, 1, 1, 3)


def test_ssim_means_within_the_bound_of_any_summation_order(ssim_results):
  """Terms in [-1, 1]: a binary64 sum of n of them in any order, divided by n, is within n 2^-53."""
  for name, (want, want_cs, s_mean, cs_mean, _) in ssim_results.items():
    bound = want.shape[1] * want.shape[2] * U
    err = np.abs(s_mean - R.map_means(want)).max(), np.abs(cs_mean - R.map_means(want_cs)).max()
    print(f'{name}: ssim_mean {err[0]:.3g} cs_mean {err[1]:.3g} bound {bound:.3g}')
    assert np.abs(want).max() <= 1.0 and np.abs(want_cs).max() <= 1.0, name
    assert err[0] <= bound and err[1] <= bound, (name, err, bound)
  assert ssim_results['uint8 255 vs 254'][0].shape[1:3] == (2, 3)       # a bound of 6.7e-16


def test_ssim_is_the_mean_over_the_channels():
  a, b, max_val, fs, sigma = _ssim_cases()['uint8 C=4 tile + 1']
  da, db = _dev(a), _dev(b)
  value, index_map = im.ssim(da, db, max_val, return_map=True)
  per_channel, _ = im.ssim_per_channel(da, db, max_val)
  assert value.shape == (2,) and value.dtype == torch.float64 and index_map.shape[3] == 4
  assert torch.equal(value, per_channel.mean(dim=1)) and torch.equal(value, im.ssim(da, db, max_val))
  want = R.map_means(R.ssim_separable(a, b, max_val, R.gaussian_taps())[0]).mean(axis=1)
  # the per-channel bound, and one rounding for each of the 3 adds and the division of the channel mean
  assert np.abs(value.cpu().numpy() - want).max() <= (index_map.shape[1] * index_map.shape[2] + 4) * U
  view = _dev(np.concatenate([a, a], axis=2))[:, :, :a.shape[2]]          # not contiguous
  assert not view.is_contiguous() and torch.equal(im.ssim(view, db, max_val), im.ssim(da, db, max_val))


# --------------------------------------------------------------------------------------- psnr
def _psnr_shapes():
  chunk = _lib.lib().se3ds_sqdiff_chunk()
  return [(1, 1, 1, 1), (1, 1, 257, 1), (2, 23, 37, 3), (3, 1, chunk + 1, 1), (2, 3, chunk // 4, 4)]


def test_sqdiff_sum_and_psnr_uint8_exact():
  for shape in _psnr_shapes():
    rng = np.random.default_rng(shape[2])
    a, b = (rng.integers(0, 256, shape).astype(np.uint8) for _ in range(2))
    got = im.sqdiff_sum(_dev(a), _dev(b)).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, R.sqdiff_sum(a, b)), shape
    p, want = im.psnr(_dev(a), _dev(b), 255.0).cpu().numpy(), R.psnr(a, b, 255.0)
    assert np.abs(p - want).max() <= 1e-12 * max(20 * np.log10(255.0), np.abs(want).max()), shape
  worst = np.full((1, 64, 256, 4), 255, np.uint8)                          # every term 65 025
  assert im.sqdiff_sum(_dev(worst), _dev(np.zeros_like(worst))).item() == worst.size * 65025.0


def test_sqdiff_sum_and_psnr_float32():
  for shape in _psnr_shapes():
    a, b = R.noise(shape, shape[2]), R.noise(shape, shape[2] + 1)
    got, want = im.sqdiff_sum(_dev(a), _dev(b)).cpu().numpy(), R.sqdiff_sum(a, b)
    n = a.size // a.shape[0]
    print(shape, float((np.abs(got - want) / want).max()), n * U)
    assert (np.abs(got - want) <= n * U * want).all(), shape           # non-negative terms, any order
    p, ref = im.psnr(_dev(a), _dev(b), 1.0).cpu().numpy(), R.psnr(a, b, 1.0)
    assert np.abs(p - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), shape


def test_psnr_of_identical_images_is_infinite():
  for x in (R.noise((2, 5, 7, 3), 1), np.full((1, 3, 3, 1), 9, np.uint8)):
    assert np.array_equal(im.psnr(_dev(x), _dev(x.copy()), 1.0).cpu().numpy(), np.full(x.shape[0], np.inf))


# ---------------------------------------------------------------------------------- downsample
@pytest.mark.parametrize('shape,dtype', [((2, 8, 10, 3), np.float32), ((2, 9, 10, 3), np.float32),
                                          ((2, 8, 11, 3), np.float32), ((1, 1, 1, 1), np.float32),
                                          ((2, 7, 5, 4), np.uint8), ((1, 1, 6, 2), np.uint8)])
def test_downsample2_sym(shape, dtype):
  x = R.noise(shape, 3) if dtype == np.float32 else np.random.default_rng(4).integers(0, 256, shape).astype(np.uint8)
  got = im.downsample2_sym(_dev(x))
  want = R.downsample2_sym(x)
  assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
  assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------- multiscale
def test_ssim_multiscale():
  """2 x 176 x 183 x 3: H reaches exactly 11 at the last scale, W is odd at scales 0 and 3 (183 -> 92
  -> 46 -> 23 -> 12).  rtol 1e-9: each factor is within 28 718 * 2^-53 = 3.2e-12 absolute (the map
  of scale 0 has 166 x 173 terms), 3.2e-11 relative at 0.1; the exponents sum to 1; a few ulp for pow."""
  a = R.smooth_noise((2, 176, 183, 3), 60, 0.0)
  b = R.smooth_noise((2, 176, 183, 3), 60, 0.08)
  want, scales = R.ssim_multiscale(a, b, 1.0)
  for k, (_, cs_mean, _) in enumerate(scales):
    print(f'scale {k}: cs in [{cs_mean.min():.4f}, {cs_mean.max():.4f}]')
    assert cs_mean.min() >= 0.1, k                       # a condition on the oracle
  assert scales[4][0].min() >= 0.1 and [s[2] for s in scales] == [166 * 173, 78 * 82, 34 * 36, 12 * 13, 1 * 2]
  got, got_scales = im.ssim_multiscale(_dev(a), _dev(b), 1.0, return_scales=True)
  for k, ((s_want, cs_want, terms), (s_got, cs_got)) in enumerate(zip(scales, got_scales)):
    assert np.abs(s_got.cpu().numpy() - s_want).max() <= terms * U, k
    assert np.abs(cs_got.cpu().numpy() - cs_want).max() <= terms * U, k
  assert got.shape == (2,) and got.dtype == torch.float64
  np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-9, atol=0)
  assert torch.equal(got, im.ssim_multiscale(_dev(a), _dev(b), 1.0))
  u8 = (a * 255).astype(np.uint8), (b * 255).astype(np.uint8)         # uint8 at scale 0, fp32 below it
  np.testing.assert_allclose(im.ssim_multiscale(_dev(u8[0]), _dev(u8[1]), 255.0).cpu().numpy(),
                             R.ssim_multiscale(u8[0], u8[1], 255.0)[0], rtol=1e-9, atol=0)


def test_two_calls_give_the_same_bits():
  a, b, max_val, fs, sigma = _ssim_cases()['noise N=3 C=3 wide']
  da, db = _dev(a), _dev(b)
  first = im.ssim_per_channel(da, db, max_val, return_map=True) + (im.psnr(da, db, max_val), im.sqdiff_sum(da, db))
  second = im.ssim_per_channel(da, db, max_val, return_map=True) + (im.psnr(da, db, max_val), im.sqdiff_sum(da, db))
  for x, y in zip(first, second):
    assert torch.equal(x, y)
  assert torch.equal(im.downsample2_sym(da), im.downsample2_sym(da))


# ------------------------------------------------------------------------------------- the ABI
def test_abi_refusals_launch_nothing():
  L = _lib.lib()
  bad_shape, bad_dtype, bad_ws = (_lib.ABI[k] for k in ('SE3DS_E_BADSHAPE', 'SE3DS_E_BADDTYPE', 'SE3DS_E_WORKSPACE'))
  n, h, w, c, fs = 2, 20, 24, 3, 11
  a = torch.zeros((n, h, w, c), device=DEV)
  taps = im.gaussian_taps()
  need = L.se3ds_ssim_workspace_bytes(n, h, w, c, fs)
  assert need > 0
  fill = lambda count: torch.full((count,), 7.0, dtype=torch.float64, device=DEV)
  means, cs, ws, index_map = fill(n * c), fill(n * c), fill(need // 8 + 1), fill(n * 10 * 14 * c)
  f32, u8 = _lib.F32, _lib.U8

  def ssim(**kw):
    v = dict(a=a.data_ptr(), b=a.data_ptr(), dtype=f32, n=n, h=h, w=w, c=c, taps=taps.ctypes.data, fs=fs,
             max_val=1.0, means=means.data_ptr(), cs=cs.data_ptr(), map=index_map.data_ptr(), ws=ws.data_ptr(),
             ws_bytes=need)
    v.update(kw)
    return L.se3ds_ssim(v['a'], v['b'], v['dtype'], v['n'], v['h'], v['w'], v['c'], v['taps'], v['fs'], v['max_val'],
                        0.01, 0.03, v['means'], v['cs'], v['map'], v['ws'], v['ws_bytes'], _lib.stream())

  for kw in (dict(a=None), dict(b=None), dict(taps=None), dict(means=None), dict(cs=None), dict(ws=None),
             dict(n=0), dict(n=65536), dict(h=0), dict(w=-1), dict(c=0), dict(c=5), dict(fs=0), dict(fs=16),
             dict(h=10), dict(w=10), dict(h=32769), dict(max_val=0.0), dict(max_val=-1.0), dict(max_val=float('nan')),
             dict(a=a.data_ptr() + 2), dict(means=means.data_ptr() + 4), dict(map=index_map.data_ptr() + 4)):
    assert ssim(**kw) == bad_shape, kw
  for dtype in (_lib.I32, _lib.BF16, 9):
    assert ssim(dtype=dtype) == bad_dtype
  assert ssim(ws_bytes=need - 1) == bad_ws
  for args in ((0, h, w, c, fs), (n, 10, w, c, fs), (n, h, w, 5, fs), (n, h, w, c, 16), (n, h, 32769, c, fs)):
    assert L.se3ds_ssim_workspace_bytes(*args) == 0, args

  out, sws = fill(n), fill(8)
  elems = h * w * c
  need_sq = L.se3ds_sqdiff_workspace_bytes(n, elems)
  assert 0 < need_sq <= 64
  sq = lambda pa, pb, dtype, count, e, po, pw, size: L.se3ds_sqdiff_sum(pa, pb, dtype, count, e, po, pw, size,
                                                                        _lib.stream())
  good = (a.data_ptr(), a.data_ptr(), f32, n, elems, out.data_ptr(), sws.data_ptr(), need_sq)
  for i, v in ((0, None), (1, None), (5, None), (6, None), (3, 0), (3, 65536), (4, 0), (4, 2 ** 40 + 1),
               (0, a.data_ptr() + 1), (5, out.data_ptr() + 4)):
    args = list(good)
    args[i] = v
    assert sq(*args) == bad_shape, (i, v)
  assert sq(*(good[:2] + (_lib.I32,) + good[3:])) == bad_dtype
  assert sq(*(good[:7] + (need_sq - 1,))) == bad_ws
  assert L.se3ds_sqdiff_workspace_bytes(0, elems) == 0 and L.se3ds_sqdiff_workspace_bytes(n, 0) == 0

  half = torch.full((n * 10 * 12 * c,), 7.0, device=DEV)
  down = lambda px, dtype, count, hh, ww, cc, po: L.se3ds_downsample2_sym(px, dtype, count, hh, ww, cc, po,
                                                                          _lib.stream())
  good = (a.data_ptr(), f32, n, h, w, c, half.data_ptr())
  for i, v in ((0, None), (6, None), (2, 0), (3, 0), (4, 32769), (5, 0), (5, 5), (0, a.data_ptr() + 2),
               (6, half.data_ptr() + 2)):
    args = list(good)
    args[i] = v
    assert down(*args) == bad_shape, (i, v)
  assert down(*(good[:1] + (_lib.BF16,) + good[2:])) == bad_dtype

  torch.cuda.synchronize()
  for t in (means, cs, ws, index_map, out, sws, half):
    assert bool((t == 7.0).all())                                          # nothing was launched
  assert ssim() == 0 and ssim(map=None) == 0 and ssim(dtype=u8, a=a.data_ptr() + 1, b=a.data_ptr() + 3) == 0
  torch.cuda.synchronize()


# ------------------------------------------------------------------------------- the evaluator
def _rollout_batch(n=2, t=3, h=32, w=64):
  rng = np.random.default_rng(70)
  image = np.stack([R.smooth_noise((n, h, w, 3), 71 + k, 0.05) for k in range(t)], axis=1)
  inputs = dict(image=image, depth=rng.uniform(0.05, 0.95, (n, t, h, w, 1)).astype(np.float32),
                position=(rng.standard_normal((n, t, 3)) * 0.3).astype(np.float32),
                depth_scale=np.full((n,), 20.0, np.float32))
  return {k: _dev(v) for k, v in inputs.items()}


class _ShiftedTruth:
  """A generator that returns frame k's ground truth rolled by k + 1 columns, and the depth it is given."""

  def __init__(self, batch):
    self.image, self.k = batch['image'], 0

  def __call__(self, inputs, training):
    assert training is False
    rgb = torch.roll(self.image[:, self.k], self.k + 1, dims=2).contiguous()
    self.k += 1
    return [None, None, None, inputs[0]['depth'], None, None, rgb]


def test_generated_rollout_scores_every_frame():
  from se3ds_amd.utils import eval_metric
  batch = _rollout_batch()
  out = eval_metric.generated_rollout(_ShiftedTruth(batch), batch, 3, image_metrics=True)
  assert len(out.psnr) == len(out.ssim) == 3
  for k in range(3):
    truth = batch['image'][:, k].contiguous()
    assert torch.equal(out.generated[k], torch.roll(truth, k + 1, dims=2))
    assert torch.equal(out.psnr[k], im.psnr(out.generated[k], truth, 1.0)) and out.psnr[k].shape == (2,)
    assert torch.equal(out.ssim[k], im.ssim(out.generated[k], truth, 1.0))
    assert bool(torch.isfinite(out.psnr[k]).all()) and bool(((out.ssim[k] > 0) & (out.ssim[k] < 1)).all())
  plain = eval_metric.generated_rollout(_ShiftedTruth(batch), batch, 3)
  assert list(plain.psnr) == [] and list(plain.ssim) == []
  assert plain._fields[:7] == ('generated', 'pred_depth', 'projected', 'proj_mask', 'proj_depth', 'depth_rmse',
                               'memory')
  for field in plain._fields[:6]:
    for x, y in zip(getattr(plain, field), getattr(out, field)):
      assert torch.equal(x, y), field
  generated, pred_depth, projected, proj_mask, proj_depth, rmse, memory = plain[:7]    # the old unpacking
  assert eval_metric.RolloutOutput([], [], [], [], [], [], memory).psnr == ()


def test_gan_manager_test_writes_the_image_scores(tmp_path):
  """The smallest configuration of tests/test_gan_test_loop_gpu.py, set up as tests/test_gif_gpu.py sets
  its test(...) run up."""
  import _video_input_ref as ref
  import test_gan_test_loop_gpu as loop
  from se3ds_amd import gin_lite
  from se3ds_amd.utils import inception_utils as iu
  examples = ref.synth_examples(2 * loop.BATCH, loop.T, 2 * loop.SIZE, seed=31)
  inception = iu.inception_model(init='random', seed=12, device=DEV)
  extra = sorted(f'{loop.SPLIT}/eval_image/{k}@{i}' for k in ('psnr', 'ema_psnr', 'ssim', 'ema_ssim')
                 for i in range(1, loop.SEQ))
  try:
    gan = loop._make_gan(str(tmp_path / 'plain'))
    gan.test(eval_examples=examples, unit_test=True, inception=inception, frechet='device')
    header, _ = loop._read(str(tmp_path / 'plain'))
    assert header == loop._columns()                                       # without the flag: as it was
    gan = loop._make_gan(str(tmp_path / 'scored'))
    rows = gan.test(eval_examples=examples, unit_test=True, inception=inception, frechet='device',
                    image_metrics=True)
  finally:
    gin_lite.clear_config()
  header, on_disk = loop._read(str(tmp_path / 'scored'))
  assert len(extra) == 4 * (loop.SEQ - 1)
  assert header == ['checkpoint_path', 'step'] + sorted(loop._columns()[2:] + extra)
  assert len(on_disk) == 1 and dict(on_disk[0]) == rows[0]
  loop._check_values(on_disk[0])
  for k in extra:
    v = float(on_disk[0][k])
    assert np.isfinite(v) and on_disk[0][k] == '{:.3f}'.format(v), (k, on_disk[0][k])
    assert (0 < v < 100) if 'psnr' in k else (-1 <= v <= 1), (k, v)
