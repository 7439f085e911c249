"""NumPy restatement of the device Frechet distance (csrc/frechet.hip, inception_utils.
frechet_distance_device) and the inputs its tests share.

  c = ||A||_F ;  Y0 = A / c ;  Z0 = I
  T = 1.5 I - 0.5 (Z Y) ;  Y <- Y T ;  Z <- T Z
  stop when |tr Y_k - tr Y_{k-1}| <= tol |tr Y_k|, at most max_iters iterations
  sqrt(A) = sqrt(c) Y ,  tr sqrt(A) = sqrt(c) tr Y
  d = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(R S2 R),  R = sqrt(S1)
"""
import functools

import numpy as np

CONVERGED, CAP_REACHED, NONFINITE = 0, 1, 2

# (dim, rows1, rows2) of the root + trace tests
FULL_RANK = [(96, 300, 300), (200, 1000, 1000)]
RANK_DEFICIENT = [(96, 40, 40), (96, 24, 300), (200, 64, 500)]
# bounds relative to s = |mu1 - mu2|^2 + tr S1 + tr S2
FULL_RANK_TOL, RANK_DEFICIENT_TOL = 1e-10, 1e-6


def features(rows, dim, seed):
  """(rows, dim) fp32: rectified Gaussian rows times a mixing matrix whose columns decay
  exponentially (correlated non-negative-ish features with a decaying spectrum, like pooled network
  features), rounded through fp32.  The mixing matrix is the identity plus a Gaussian coupling: a
  purely Gaussian one is itself ill conditioned (1e6 .. 1e8 at these sizes), which puts a full-rank
  covariance's condition number near 1e8 and the sqrtm reference's own error above the 1e-10 bound;
  with this one a full-rank covariance has a condition number of about 2e3."""
  rng = np.random.default_rng(seed)
  mix = np.eye(dim) + 0.5 * rng.standard_normal((dim, dim)) / np.sqrt(dim)
  scale = np.exp(-3.0 * np.arange(dim) / dim)
  x = np.maximum(rng.standard_normal((rows, dim)), 0.0) @ (mix * scale[None, :])
  return x.astype(np.float32)


def stats(x):
  x = x.astype(np.float64)
  return np.mean(x, axis=0), np.cov(x, rowvar=False)


def ns_sqrt_trace(a, max_iters=48, tol=1e-10):
  """(tr sqrt(a), iterations, status, sqrt(a)) by the coupled Newton-Schulz iteration."""
  n = a.shape[0]
  c = np.sqrt(np.sum(a * a))
  if not np.isfinite(c):
    return np.trace(a), 0, NONFINITE, a
  if c == 0.0:
    return 0.0, 0, CONVERGED, np.zeros_like(a)
  y, z = a / c, np.eye(n)
  prev, k, status = np.trace(y), 0, CAP_REACHED
  with np.errstate(all='ignore'):
    for k in range(1, max_iters + 1):
      t = 1.5 * np.eye(n) - 0.5 * (z @ y)
      y, z = y @ t, t @ z
      tr = np.trace(y)
      delta, prev = abs(tr - prev), tr
      if not np.isfinite(tr):
        status = NONFINITE
        break
      if delta <= tol * abs(tr):
        status = CONVERGED
        break
  return np.sqrt(c) * prev, k, status, np.sqrt(c) * y


def scale(mu1, s1, mu2, s2):
  d = mu1 - mu2
  return d.dot(d) + np.trace(s1) + np.trace(s2)


def frechet_ns(mu1, s1, mu2, s2, max_iters=48, tol=1e-10):
  """(value, (k1, k2), converged) of the restated device algorithm."""
  _, k1, st1, r = ns_sqrt_trace(s1, max_iters, tol)
  tr, k2, st2, _ = ns_sqrt_trace((r @ s2) @ r, max_iters, tol)
  value = scale(mu1, s1, mu2, s2) - 2 * tr
  return value, (k1, k2), st1 == CONVERGED and st2 == CONVERGED and bool(np.isfinite(value))


@functools.lru_cache(maxsize=None)
def case(dim, rows1, rows2):
  """The statistics of one test case, the reference's value and the restatement's, computed once."""
  from se3ds_amd.utils import inception_utils as iu
  mu1, s1 = stats(features(rows1, dim, 1000 + dim + rows1))
  mu2, s2 = stats(features(rows2, dim, 2000 + dim + rows2))
  want = float(iu._calculate_frechet_distance(mu1, s1, mu2, s2))
  ns, iters, converged = frechet_ns(mu1, s1, mu2, s2)
  out = dict(mu1=mu1, s1=s1, mu2=mu2, s2=s2, want=want, ns=ns, ns_iters=iters,
             ns_converged=converged, s=float(scale(mu1, s1, mu2, s2)))
  for v in out.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return out
