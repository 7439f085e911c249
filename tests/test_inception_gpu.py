"""GPU tests of the Inception-v3 evaluator: the kernels of csrc/inception.hip against NumPy / torch-CPU,
the whole network against a torch-CPU fp64 restatement of Keras InceptionV3 (random seeded weights),
and EvalMetric end to end with a tiny generator."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _inception_ref as ref
from se3ds_amd import _lib
from se3ds_amd import gin_lite
from se3ds_amd.utils import inception_utils as iu
from se3ds_amd.utils import pano_utils

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def weights():
  return iu.random_weights(11)


def _unfused(x, rf):
  """The chain run op by op on the device: roll / flip, crop_pano, se3ds_resize, renormalise."""
  parts = []
  for b in range(x.shape[0]):
    xb = torch.roll(x[b:b + 1], int(rf[b][0]), dims=2)
    if rf[b][1]:
      xb = torch.flip(xb, dims=[2])
    parts.append(xb)
  y = pano_utils.crop_pano(torch.cat(parts), resize_to_original=False)
  y = pano_utils.resize(y, 299, 299, 'bilinear')
  return torch.clamp(y * 2 - 1, -1, 1)


@pytest.mark.parametrize('h,w', [(64, 128), (512, 1024), (1024, 2048)])
@pytest.mark.parametrize('flip', [False, True])
def test_preprocess_matches_the_unfused_chain(h, w, flip):
  rng = np.random.default_rng(h + flip)
  n = 2
  x = rng.uniform(0, 1, (n, h, w, 3)).astype(np.float32)
  rf = np.array([(int(rng.integers(-w // 2, w // 2)), int(flip)) for _ in range(n)], np.int32)
  xd = torch.from_numpy(x).to(DEV)
  got = iu.preprocess(xd, roll_flip=rf)
  want = _unfused(xd, rf)
  assert torch.equal(got, want)
  assert np.abs(got.cpu().numpy() - ref.preprocess_np(x, rf)).max() <= 1e-6
  gb = iu.preprocess(xd, roll_flip=rf, dtype=torch.bfloat16)
  assert torch.equal(gb, want.to(torch.bfloat16))
  # no augment: the plain crop + resize + renormalise
  assert torch.equal(iu.preprocess(xd), _unfused(xd, np.zeros((n, 2), np.int32)))


def _ulp_diff(a, b):
  return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(a.dtype)).astype(np.float64)


@pytest.mark.parametrize('size', [147, 71, 35, 17, 8])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pools_vs_torch(size, dtype):
  L = _lib.lib()
  rng = np.random.default_rng(size)
  n, c, ctot, c0 = 2, 24, 40, 12
  x = torch.from_numpy(rng.standard_normal((n, size, size, c)).astype(np.float32)).to(dtype)
  xd = x.to(DEV)
  code = _lib.dtype_code(xd)
  xc = x.float().permute(0, 3, 1, 2)
  # max 3x3 / 2 VALID, into a channel slice
  want = F.max_pool2d(xc, 3, 2).permute(0, 2, 3, 1)
  ho = want.shape[1]
  y = torch.full((n, ho, ho, ctot), 7.0, dtype=dtype, device=DEV)
  _lib.check(L.se3ds_inception_maxpool3s2(xd.data_ptr(), code, n, size, size, c, y.data_ptr(), ctot, c0,
                                          _lib.stream()), 'maxpool')
  yc = y.cpu().float()
  assert torch.equal(yc[..., c0:c0 + c], want)
  assert torch.all(yc[..., :c0] == 7) and torch.all(yc[..., c0 + c:] == 7)
  # average 3x3 / 1 SAME, padded taps excluded
  want = F.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, padding=1, count_include_pad=False).permute(0, 2, 3, 1)
  y = torch.full((n, size, size, ctot), 7.0, dtype=dtype, device=DEV)
  _lib.check(L.se3ds_inception_avgpool3s1(xd.data_ptr(), code, n, size, size, c, y.data_ptr(), ctot, c0,
                                          _lib.stream()), 'avgpool')
  yc = y.cpu()
  got = yc[..., c0:c0 + c]
  if dtype == torch.float32:
    assert _ulp_diff(got.numpy(), want.numpy()).max() <= 1
  else:
    # one bf16 ulp: neighbours in the bf16 bit pattern
    gi = got.view(torch.int16).int().numpy()
    wi = want.contiguous().view(torch.int16).int().numpy()
    assert np.abs(gi - wi).max() <= 1
  assert torch.all(yc[..., :c0].float() == 7) and torch.all(yc[..., c0 + c:].float() == 7)


def test_global_pool_and_softmax():
  L = _lib.lib()
  rng = np.random.default_rng(3)
  x = rng.standard_normal((3, 8, 8, 2048)).astype(np.float32)
  xd = torch.from_numpy(x).to(DEV)
  p = torch.empty((3, 2048), device=DEV)
  _lib.check(L.se3ds_global_avg_pool(xd.data_ptr(), _lib.F32, 3, 64, 2048, p.data_ptr(), _lib.stream()), 'gap')
  np.testing.assert_allclose(p.cpu().numpy(), x.astype(np.float64).mean((1, 2)), rtol=1e-5, atol=1e-6)
  z = (rng.standard_normal((5, 1000)) * 4).astype(np.float32)
  zd = torch.from_numpy(z).to(DEV)
  s = torch.empty((5, 1000), device=DEV)
  _lib.check(L.se3ds_softmax_rows(zd.data_ptr(), _lib.F32, 5, 1000, s.data_ptr(), _lib.stream()), 'softmax')
  e = np.exp(z.astype(np.float64) - z.max(1, keepdims=True))
  np.testing.assert_allclose(s.cpu().numpy(), e / e.sum(1, keepdims=True), rtol=1e-5, atol=1e-9)


def test_feature_moments_vs_numpy():
  rng = np.random.default_rng(4)
  x = (np.abs(rng.standard_normal((300, 2048))) * rng.uniform(0.1, 2, 2048)).astype(np.float32)
  xd = torch.from_numpy(x).to(DEV)
  a = iu.FeatureMoments().update(xd[:100]).update(xd[100:])
  n, s, g = a.state()
  x64 = x.astype(np.float64)
  assert n == 300
  assert np.abs(s - x64.sum(0)).max() <= 1e-12 * np.abs(x64.sum(0)).max()
  gram = x64.T @ x64
  assert np.abs(g - gram).max() <= 1e-12 * np.abs(gram).max()
  np.testing.assert_allclose(a.mean(), x64.mean(0), rtol=1e-12)
  cov = np.cov(x64, rowvar=False)
  assert np.abs(a.cov() - cov).max() <= 1e-9 * np.abs(cov).max()
  # bit-reproducible
  b = iu.FeatureMoments().update(xd[:100]).update(xd[100:])
  nb, sb, gb = b.state()
  assert s.tobytes() == sb.tobytes() and g.tobytes() == gb.tobytes()
  # merge of two halves == one pass over the same batches
  h1, h2 = iu.FeatureMoments().update(xd[:100]), iu.FeatureMoments().update(xd[100:])
  nm, sm, gm = h1.merge(h2).state()
  assert nm == 300
  np.testing.assert_allclose(sm, s, rtol=1e-13)
  np.testing.assert_allclose(gm, g, rtol=1e-13)
  # ragged dims (not a multiple of the 64 tile)
  y = rng.standard_normal((33, 100)).astype(np.float32)
  m = iu.FeatureMoments(dim=100).update(torch.from_numpy(y).to(DEV))
  _, sy, gy = m.state()
  np.testing.assert_allclose(gy, y.astype(np.float64).T @ y.astype(np.float64), rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(sy, y.astype(np.float64).sum(0), rtol=1e-12, atol=1e-12)


def _rel(a, b):
  return np.abs(a - b).max() / np.abs(b).max()


def _cos(a, b):
  a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
  return a @ b / np.linalg.norm(a) / np.linalg.norm(b)


def test_forward_vs_fp64_restatement(weights):
  rng = np.random.default_rng(5)
  x = rng.uniform(-1, 1, (4, 299, 299, 3)).astype(np.float32)
  rp, rq = ref.inception_v3(weights, x)
  assert rp.std() > 1e-3 and rq.std() > 1e-6   # the random network is not degenerate
  m = iu.InceptionV3(weights, device=DEV)
  p, q = m(torch.from_numpy(x).to(DEV))
  assert p.shape == (4, 2048) and q.shape == (4, 1000)
  assert _rel(p.cpu().numpy(), rp) <= 1e-4
  assert _rel(q.cpu().numpy(), rq) <= 1e-4
  mb = iu.InceptionV3(weights, device=DEV, dtype=torch.bfloat16)
  pb, qb = mb(torch.from_numpy(x).to(DEV))
  cos = _cos(pb.cpu().numpy(), rp)
  print(f'bf16 pools cosine vs fp64: {cos:.6f}')
  assert cos >= 0.999


def test_forward_in_chunks(weights):
  """More images than max_batch: the forward runs chunk by chunk and concatenates."""
  rng = np.random.default_rng(8)
  x = torch.from_numpy(rng.uniform(-1, 1, (5, 299, 299, 3)).astype(np.float32)).to(DEV)
  p, q = iu.InceptionV3(weights, device=DEV)(x)
  pc, qc = iu.InceptionV3(weights, device=DEV, max_batch=2)(x)
  assert pc.shape == (5, 2048) and qc.shape == (5, 1000)
  assert _rel(pc.cpu().numpy(), p.cpu().numpy()) <= 1e-6
  assert _rel(qc.cpu().numpy(), q.cpu().numpy()) <= 1e-6


def test_get_inception_from_panorama_frames(weights):
  """One batch of 384 x 1024 frames through the evaluator's gather and the network."""
  rng = np.random.default_rng(6)
  x = rng.uniform(0, 1, (2, 384, 1024, 3)).astype(np.float32)
  rf = np.array([(100, 1), (-37, 0)], np.int32)
  inp = ref.preprocess_np(x, rf)
  rp, rq = ref.inception_v3(weights, inp)
  m = iu.InceptionV3(weights, device=DEV)
  p, q = m(iu.preprocess(torch.from_numpy(x).to(DEV), roll_flip=rf))
  assert _rel(p.cpu().numpy(), rp) <= 1e-4 and _rel(q.cpu().numpy(), rq) <= 1e-4
  # get_inception: the reference's resize + renormalise on an already cropped frame
  crop = pano_utils.crop_pano(torch.from_numpy(x).to(DEV))
  p2, _ = iu.get_inception(crop, m)
  p3, _ = m(iu.preprocess(torch.from_numpy(x).to(DEV)))
  assert torch.equal(p2, p3)
  # re_normalize=False: resized (reference semantics), not renormalised
  scaled = crop * 2 - 1
  p4, _ = iu.get_inception(scaled, m, re_normalize=False)
  p5, _ = m(pano_utils.resize(scaled, 299, 299, 'bilinear'))
  assert torch.equal(p4, p5)


def test_eval_metric_end_to_end():
  from se3ds_amd.models import image_models
  from se3ds_amd.utils import eval_metric
  gin_lite.clear_config()
  size, t, n = 64, 3, 8
  G = image_models.ResNetGenerator(image_size=size, gen_dims=8, z_dim=4, resnet_version='50',
                                   device=DEV, seed=3, dtype=torch.float32)
  rng = np.random.default_rng(7)

  def batches():
    while True:
      image = rng.uniform(0, 1, (n, t, size, 2 * size, 3)).astype(np.float32)
      depth = rng.uniform(0.05, 0.95, (n, t, size, 2 * size, 1)).astype(np.float32)
      b = dict(image=image, depth=depth, position=(rng.standard_normal((n, t, 3)) * 0.3).astype(np.float32),
               depth_scale=np.full((n,), 20.0, np.float32))
      yield {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}

  inception = iu.inception_model(init='random', seed=12, device=DEV)
  em = eval_metric.EvalMetric(batches(), eval_num=16, batch_size=n, avg_num=2, eval_seq_len=t,
                              inception=inception, keep_pools=True)
  fid, fid_std, rmse = em.calculate_fid_score(G)
  assert sorted(fid) == sorted(fid_std) == sorted(rmse) == list(range(1, t))
  for i in range(1, t):
    assert np.isfinite(fid[i]) and np.isfinite(fid_std[i]) and np.isfinite(rmse[i]), i
    assert em.real_pools[i].shape == (16, 2048) and em.generated_pools[i].shape == (16, 2048)
    # the last repeat's FID from the device moments == the NumPy FID of the downloaded pools
    want = iu.calculate_fid(em.generated_pools[i].astype(np.float64), em.real_pools[i].astype(np.float64))
    got = em.fid_list[i][-1]
    assert abs(got - want) <= 1e-6 * abs(want), (i, got, want)
    # real vs real, from two independent accumulations of the same rows (another batch split)
    other = iu.FeatureMoments(device=DEV)
    rows = torch.from_numpy(em.real_pools[i]).to(DEV)
    for a, b in ((0, 5), (5, 11), (11, 16)):
      other.update(rows[a:b])
    assert other.count == 16
    assert abs(em._real[i].fid(other)) < 1e-3
