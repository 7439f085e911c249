"""CPU tests of the device Frechet distance's algorithm and interface: the NumPy restatement of the
coupled Newton-Schulz iteration (_frechet_ref) against the reference's sqrtm formulation on the shapes
tests/test_frechet_gpu.py uses, why the stop rule exists, and the argument checks that need no GPU."""
import numpy as np
import pytest
import torch

import _frechet_ref as ref
from se3ds_amd import _lib
from se3ds_amd.utils import inception_utils as iu


@pytest.mark.parametrize('dim,rows1,rows2', ref.FULL_RANK + ref.RANK_DEFICIENT)
def test_restatement_meets_the_gpu_bounds_against_sqrtm(dim, rows1, rows2):
  """The algorithm alone (binary64 NumPy) is within the bound the GPU test asks of the kernels:
  1e-10 s full rank, 1e-6 s rank deficient, s = |mu1 - mu2|^2 + tr S1 + tr S2."""
  c = ref.case(dim, rows1, rows2)
  tol = ref.FULL_RANK_TOL if (dim, rows1, rows2) in ref.FULL_RANK else ref.RANK_DEFICIENT_TOL
  err = abs(c['ns'] - c['want']) / c['s']
  print(f'dim {dim} rows {rows1}/{rows2}: d {c["want"]:.6g} s {c["s"]:.6g} err/s {err:.3g} '
        f'iterations {c["ns_iters"]}')
  assert c['ns_converged']
  assert max(c['ns_iters']) <= 48
  assert err <= tol


def test_without_the_stop_rule_a_rank_deficient_root_overflows():
  """In the null space of a singular matrix Z grows 1.5 x per iteration: with tol = 0 and 80
  iterations the result is not finite (unless the trace happens to repeat bit for bit first, as it
  does for some covariances: the product R S2 R never does here).  The stop on the trace increment
  is part of the algorithm."""
  c = ref.case(96, 24, 300)
  tr, k, status, _ = ref.ns_sqrt_trace(c['s1'], max_iters=80, tol=0.0)
  assert status == ref.NONFINITE and not np.isfinite(tr) and k > 48, (tr, k, status)
  tr, k, status, _ = ref.ns_sqrt_trace(c['s1'])
  assert status == ref.CONVERGED and np.isfinite(tr) and k <= 48
  for shape in ref.RANK_DEFICIENT:
    c = ref.case(*shape)
    value, iters, ok = ref.frechet_ns(c['mu1'], c['s1'], c['mu2'], c['s2'], max_iters=80, tol=0.0)
    assert not ok and not np.isfinite(value), (shape, value, iters)


def test_restatement_degenerate_inputs():
  c = ref.case(96, 40, 40)
  v, _, ok = ref.frechet_ns(c['mu1'], c['s1'], c['mu1'], c['s1'])
  assert ok and abs(v) <= 1e-6 * ref.scale(c['mu1'], c['s1'], c['mu1'], c['s1'])
  z = np.zeros_like(c['s1'])
  v, iters, ok = ref.frechet_ns(c['mu1'], z, c['mu2'], z)
  d = c['mu1'] - c['mu2']
  assert ok and iters == (0, 0) and v == d.dot(d)


def test_device_entry_points_have_no_cpu_fallback():
  mu, sigma = torch.zeros(8, dtype=torch.float64), torch.eye(8, dtype=torch.float64)
  with pytest.raises(_lib.Se3dsHipError):
    iu.frechet_distance_device(mu, sigma, mu, sigma)
  with pytest.raises(_lib.Se3dsHipError):
    iu.sqrt_trace_device(sigma)
  with pytest.raises(_lib.Se3dsHipError):
    iu.f64_gemm(sigma, sigma)


class _NoDevice(iu.FeatureMoments):
  """A FeatureMoments without its device buffers: the argument check comes before any use of them."""

  def __init__(self):
    pass


def test_fid_rejects_an_unknown_method():
  with pytest.raises(ValueError, match='method'):
    _NoDevice().fid(_NoDevice(), method='gpu')
