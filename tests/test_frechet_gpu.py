"""GPU tests of the device Frechet distance (csrc/frechet.hip): the binary64 MFMA GEMM bit for bit on
integer data, the moments -> statistics kernel against FeatureMoments.mean_cov(), the Newton-Schulz
root + trace against the reference's sqrtm formulation and the NumPy restatement (_frechet_ref), the
degenerate inputs, one production-size case and EvalMetric(frechet='device') end to end.

Bounds are relative to s = |mu1 - mu2|^2 + tr S1 + tr S2 (the distance itself can be 0): 1e-10 s for
full-rank covariances, 1e-6 s for rank-deficient ones; tests/test_frechet_cpu.py shows that the
algorithm in NumPy meets them on the same inputs."""
import warnings

import numpy as np
import pytest
import torch

import _frechet_ref as ref
from se3ds_amd import gin_lite
from se3ds_amd.utils import inception_utils as iu

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 512   # sentinel doubles on either side of C


def _dev(a):
  return torch.from_numpy(np.array(a, order='C')).to(DEV)   # a copy: the shared cases are read-only


def _gemm_guarded(a, b, alpha, diag):
  """f64_gemm into the middle of a larger allocation; checks that nothing around C was written."""
  n = a.shape[0]
  buf = torch.full((n * n + 2 * GUARD,), -12345.0, dtype=torch.float64, device=DEV)
  out = buf[GUARD:GUARD + n * n].view(n, n)
  iu.f64_gemm(_dev(a), _dev(b), alpha, diag, out=out)
  h = buf.cpu().numpy()
  assert (h[:GUARD] == -12345.0).all() and (h[GUARD + n * n:] == -12345.0).all(), 'wrote outside C'
  return h[GUARD:GUARD + n * n].reshape(n, n)


# ------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize('n', [16, 17, 64, 100, 130, 200])
def test_gemm_is_bit_exact_on_integer_matrices(n):
  """Entries in [-8, 8]: every product and partial sum is an integer below 2^53, so binary64 is exact
  whatever the order, and alpha in {1, -0.5, 2} keeps it exact."""
  rng = np.random.default_rng(n)
  a = rng.integers(-8, 9, (n, n))
  b = rng.integers(-8, 9, (n, n))
  prod = (a.astype(np.int64) @ b.astype(np.int64)).astype(np.float64)
  for alpha, diag in ((1.0, 0.0), (-0.5, 1.5), (2.0, -3.0)):
    got = _gemm_guarded(a.astype(np.float64), b.astype(np.float64), alpha, diag)
    want = alpha * prod + diag * np.eye(n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (n, alpha, diag, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize('n', [16, 17, 64, 100, 130, 200])
def test_gemm_operand_maps_with_identity_and_distinct_values(n):
  """A = I with B[i][j] = i n + j (asymmetric, every element distinct) gives C = B, and B = I gives
  C = A: a transposed or permuted fragment map moves a named row."""
  d = np.arange(n * n, dtype=np.float64).reshape(n, n)
  eye = np.eye(n)
  for name, a, b in (('A = I', eye, d), ('B = I', d, eye)):
    got = _gemm_guarded(a, b, 1.0, 0.0)
    rows = np.nonzero((got != d).any(axis=1))[0]
    assert rows.size == 0, (name, n, 'wrong rows', rows[:8], got[rows[0]][:8], d[rows[0]][:8])


# ------------------------------------------------------------------------------ moments -> statistics
@pytest.mark.parametrize('dim', [100, 2048])
@pytest.mark.parametrize('rows', [33, 300])
def test_mean_cov_device_matches_the_host_formula(dim, rows):
  fm = iu.FeatureMoments(dim=dim, device=DEV)
  x = _dev(ref.features(rows, dim, 7 * dim + rows))
  fm.update(x[:rows // 3]).update(x[rows // 3:])
  mean_h, cov_h = fm.mean_cov()
  mean_d, cov_d = fm.mean_cov_device()
  assert torch.equal(cov_d, cov_d.T), 'the device covariance is not exactly symmetric'
  mean_d, cov_d = mean_d.cpu().numpy(), cov_d.cpu().numpy()
  assert np.abs(mean_d - mean_h).max() <= 1e-12 * np.abs(mean_h).max()
  assert np.abs(cov_d - cov_h).max() <= 1e-12 * np.abs(cov_h).max()
  # the strictly lower 64 x 64 tiles of the Gram matrix were never written; the covariance has them
  assert not fm._gram[64:, :64].any()
  assert (cov_d[64:, :64] != 0).all()


def test_mean_cov_device_of_merged_accumulators_and_too_few_rows():
  x = _dev(ref.features(40, 100, 5))
  a, b = iu.FeatureMoments(dim=100, device=DEV), iu.FeatureMoments(dim=100, device=DEV)
  a.update(x[:1])
  with pytest.raises(ValueError, match='at least two rows'):
    a.mean_cov_device()
  a.update(x[1:25])
  root = a.sqrt_cov_device()
  assert a.sqrt_cov_device() is root            # cached
  b.update(x[25:])
  a.merge(b)
  assert a._root is None                        # dropped by merge()
  whole = iu.FeatureMoments(dim=100, device=DEV).update(x)
  mean_m, cov_m = a.mean_cov_device()
  mean_w, cov_w = whole.mean_cov_device()
  assert (mean_m - mean_w).abs().max() <= 1e-12 * mean_w.abs().max()
  assert (cov_m - cov_w).abs().max() <= 1e-12 * cov_w.abs().max()
  whole.sqrt_cov_device()
  whole.update(x[:3])
  assert whole._root is None                    # dropped by update()


# ------------------------------------------------------------------------------ root + trace
@pytest.mark.parametrize('dim,rows1,rows2', ref.FULL_RANK + ref.RANK_DEFICIENT)
def test_device_distance_matches_sqrtm(dim, rows1, rows2):
  c = ref.case(dim, rows1, rows2)
  full = (dim, rows1, rows2) in ref.FULL_RANK
  tol = ref.FULL_RANK_TOL if full else ref.RANK_DEFICIENT_TOL
  mu1, s1, mu2, s2 = (_dev(c[k]) for k in ('mu1', 's1', 'mu2', 's2'))
  r = iu.frechet_distance_device(mu1, s1, mu2, s2)
  err = abs(r.value - c['want']) / c['s']
  print(f'dim {dim} rows {rows1}/{rows2}: device {r.value!r} sqrtm {c["want"]!r} err/s {err:.3g} '
        f'iterations {r.iterations} (restatement {c["ns_iters"]})')
  assert r.converged
  assert err <= tol
  for k, k_ref in zip(r.iterations, c['ns_iters']):
    assert k <= 48 and abs(k - k_ref) <= 3, (r.iterations, c['ns_iters'])
  root = iu.sqrt_trace_device(s1)
  assert root.status == iu.SQRT_CONVERGED and root.iterations == r.iterations[0]
  if full:
    rr = root.root.cpu().numpy()
    resid = np.linalg.norm(rr @ rr - c['s1']) / np.linalg.norm(c['s1'])
    print(f'  |root root - S|_F / |S|_F = {resid:.3g}')
    assert resid <= 1e-8
  # a passed root gives the same bits as a computed one, and so does a second call
  r2 = iu.frechet_distance_device(mu1, s1, mu2, s2, root1=root.root)
  assert r2.value == r.value and r2.iterations == (0, r.iterations[1]) and r2.converged
  again = iu.sqrt_trace_device(s1)
  assert again.trace == root.trace and torch.equal(again.root, root.root)
  assert iu.frechet_distance_device(mu1, s1, mu2, s2) == r


# ------------------------------------------------------------------------------ degenerate inputs
def test_a_set_against_itself():
  c = ref.case(96, 40, 40)
  mu, s = _dev(c['mu1']), _dev(c['s1'])
  r = iu.frechet_distance_device(mu, s, mu, s)
  scale = ref.scale(c['mu1'], c['s1'], c['mu1'], c['s1'])
  print(f'self distance {r.value:.3g} at s = {scale:.4g}')
  assert r.converged and abs(r.value) <= 1e-6 * scale


def test_all_zero_covariances():
  c = ref.case(96, 40, 40)
  z = torch.zeros((96, 96), dtype=torch.float64, device=DEV)
  r = iu.frechet_distance_device(_dev(c['mu1']), z, _dev(c['mu2']), z)
  d = c['mu1'] - c['mu2']
  assert r.converged and r.iterations == (0, 0)
  assert abs(r.value - d.dot(d)) <= 1e-14 * d.dot(d)
  root = iu.sqrt_trace_device(z)
  assert root.trace == 0.0 and root.status == iu.SQRT_CONVERGED and not root.root.any()


def test_iteration_cap_is_reported_and_fid_falls_back_to_the_host():
  c = ref.case(96, 300, 300)
  r = iu.sqrt_trace_device(_dev(c['s1']), max_iters=3)
  assert r.status == iu.SQRT_CAP_REACHED and r.iterations == 3
  d = iu.frechet_distance_device(*(_dev(c[k]) for k in ('mu1', 's1', 'mu2', 's2')), max_iters=3)
  assert not d.converged and d.iterations == (3, 3)
  a = iu.FeatureMoments(dim=96, device=DEV).update(_dev(ref.features(300, 96, 1)))
  b = iu.FeatureMoments(dim=96, device=DEV).update(_dev(ref.features(300, 96, 2)))
  with pytest.warns(UserWarning, match='did not converge'):
    got = a.fid(b, method='device', max_iters=3)
  assert got == a.fid(b)
  with warnings.catch_warnings():
    warnings.simplefilter('error')
    dev = a.fid(b, method='device')
  mu1, s1 = a.mean_cov()
  mu2, s2 = b.mean_cov()
  assert abs(dev - a.fid(b)) <= 1e-10 * ref.scale(mu1, s1, mu2, s2)


# ------------------------------------------------------------------------------ production size
def test_production_size_against_the_host_path():
  """dim 2048, 500 rows each (rank deficient): FeatureMoments.fid on the device against the host's
  sqrtm of the same moments."""
  a = iu.FeatureMoments(device=DEV).update(_dev(ref.features(500, 2048, 31)))
  b = iu.FeatureMoments(device=DEV).update(_dev(ref.features(500, 2048, 32)))
  with warnings.catch_warnings():
    warnings.simplefilter('error')   # a fall-back to the host would warn
    got = a.fid(b, method='device')
  want = a.fid(b)
  mu1, s1 = a.mean_cov()
  mu2, s2 = b.mean_cov()
  s = ref.scale(mu1, s1, mu2, s2)
  print(f'dim 2048: device {got!r} host {want!r} err/s {abs(got - want) / s:.3g} '
        f'root iterations {a._root[3]}')
  assert abs(got - want) <= 1e-6 * s


# ------------------------------------------------------------------------------ end to end
def _eval_metric_fids(frechet):
  """The tiny random-weight set-up of test_inception_gpu.test_eval_metric_end_to_end (one repeat)."""
  from se3ds_amd.models import image_models
  from se3ds_amd.utils import eval_metric
  gin_lite.clear_config()
  torch.manual_seed(0)
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
  em = eval_metric.EvalMetric(batches(), eval_num=16, batch_size=n, avg_num=1, eval_seq_len=t,
                              inception=inception, keep_pools=True, frechet=frechet)
  with warnings.catch_warnings():
    warnings.simplefilter('error')   # a fall-back to the host would warn
    em.calculate_fid_score(G)
  return em


def test_eval_metric_with_the_device_frechet_distance():
  host = _eval_metric_fids('host')
  dev = _eval_metric_fids('device')
  assert sorted(dev.fid_list) == [1, 2]
  for i in dev.fid_list:
    assert np.array_equal(host.generated_pools[i], dev.generated_pools[i]), 'the runs differ before the FID'
    s = ref.scale(*ref.stats(host.real_pools[i]), *ref.stats(host.generated_pools[i]))
    got, want = dev.fid_list[i][0], host.fid_list[i][0]
    print(f'frame {i}: device {got!r} host {want!r} err/s {abs(got - want) / s:.3g}')
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * s
