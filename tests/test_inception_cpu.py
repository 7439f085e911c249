"""CPU tests of the Inception-v3 evaluator (utils/inception_utils.py): the architecture's parameter
counts without weights, the Frechet distance and Inception Score against closed forms, and the two
weight loaders."""
import os
import warnings

import numpy as np
import pytest

from se3ds_amd.utils import inception_utils as iu
from se3ds_amd.utils import tf_bundle
from se3ds_amd.utils.tf_checkpoint_keys import SUFFIX


def test_architecture_matches_keras_parameter_counts():
  """Keras InceptionV3(include_top=True): 23,851,784 parameters, 34,432 non-trainable (the BN moving
  statistics), in 94 Conv2D + 94 BatchNormalization + 1 Dense layers."""
  w = iu.random_weights(0)
  m = iu.InceptionV3(w, device='cpu')
  assert m.count_params() == (23851784, 34432)
  assert len(iu.conv_specs()) == 94
  assert sum(k.endswith('/kernel') and k.startswith('conv2d') for k in w) == 94
  assert sum(k.endswith('/beta') for k in w) == 94
  assert w['predictions/kernel'].shape == (2048, 1000)
  assert all(c % 4 == 0 for _, c, *_ in iu.conv_specs())
  # deterministic
  w2 = iu.random_weights(0)
  assert all(np.array_equal(w[k], w2[k]) for k in w)


def test_frechet_distance_closed_form_on_diagonal_gaussians():
  rng = np.random.default_rng(1)
  d = 64
  mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
  s1, s2 = rng.uniform(0.1, 2.0, d), rng.uniform(0.1, 2.0, d)
  got = iu._calculate_frechet_distance(mu1, np.diag(s1), mu2, np.diag(s2))
  want = np.sum((mu1 - mu2) ** 2) + np.sum(s1 + s2 - 2 * np.sqrt(s1 * s2))
  assert abs(got - want) <= 1e-9 * abs(want)


def test_fid_of_identical_pools_is_zero():
  pool = np.random.default_rng(2).standard_normal((200, 16))
  assert abs(iu.calculate_fid(pool, pool)) < 1e-6


def test_fid_shape_mismatch():
  with pytest.raises(iu.ShapeNotMatchError):
    iu._calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(3))
  with pytest.raises(iu.ShapeNotMatchError):
    iu._calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(3), np.eye(4))


def test_singular_product_warns_and_retries():
  """A nilpotent product has no square root (sqrtm -> nan): eps = 1e-6 goes onto both diagonals,
  sqrt((N + eps I)(1 + eps) I) has trace ~ 2 sqrt(eps)."""
  nil = np.array([[0.0, 1.0], [0.0, 0.0]])
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    fid = iu._calculate_frechet_distance(np.zeros(2), nil, np.ones(2), np.eye(2))
  assert any('singular product' in str(r.message) for r in rec)
  assert np.isfinite(fid) and abs(fid - (4 - 4e-3)) < 1e-5


def test_inception_score_closed_forms():
  u = np.full((100, 10), 0.1)
  m, s = iu.calculate_inception_score(u, num_splits=1)
  assert abs(m - 1.0) < 1e-12 and s == 0
  k = 7
  p = np.full((k * 10, 1000), 1e-30)
  p[np.arange(k * 10), np.arange(k * 10) % k] = 1.0
  m, _ = iu.calculate_inception_score(p, num_splits=1)
  assert abs(m - k) < 1e-6


def test_checkpoint_path_none_is_an_error():
  with pytest.raises(ValueError, match='checkpoint_path'):
    iu.inception_model()
  with pytest.raises(ValueError):
    iu.inception_model(version='V1', init='random')


def test_npz_and_bundle_load_bit_identically(tmp_path):
  w = iu.random_weights(3)
  npz = os.path.join(tmp_path, 'w.npz')
  np.savez(npz, **w)
  ckdir = os.path.join(tmp_path, 'ckpt')
  os.makedirs(ckdir)
  keys = iu.bundle_keys()
  assert len(set(keys.values())) == len(keys) == 94 * 4 + 2
  tf_bundle.write_bundle(os.path.join(ckdir, 'ckpt-1'), {keys[k]: v for k, v in w.items()})
  with open(os.path.join(ckdir, 'checkpoint'), 'w') as f:
    f.write('model_checkpoint_path: "ckpt-1"\nall_model_checkpoint_paths: "ckpt-1"\n')
  a, b = iu.load_weights(npz), iu.load_weights(ckdir)
  assert sorted(a) == sorted(b) == sorted(w)
  for k in w:
    assert a[k].tobytes() == w[k].tobytes() and b[k].tobytes() == w[k].tobytes(), k
  fa, fb = iu.fold_batch_norm(a), iu.fold_batch_norm(b)
  assert all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(fa, fb))
  m = iu.inception_model(checkpoint_path=ckdir, device='cpu')
  assert m.count_params() == (23851784, 34432)


def test_wrong_shape_is_refused(tmp_path):
  w = iu.random_weights(4)
  w['conv2d_5/kernel'] = w['conv2d_5/kernel'][..., :-4]
  npz = os.path.join(tmp_path, 'bad.npz')
  np.savez(npz, **w)
  with pytest.raises(ValueError, match='conv2d_5/kernel'):
    iu.load_weights(npz)
  del w['conv2d_5/kernel']
  np.savez(npz, **w)
  with pytest.raises(ValueError, match='missing'):
    iu.load_weights(npz)


def test_batch_norm_folding():
  w = iu.random_weights(5)
  k, b = iu.fold_batch_norm(w)[7]
  r = 1 / np.sqrt(w['batch_normalization_7/moving_variance'].astype(np.float64) + 1e-3)
  np.testing.assert_allclose(k, w['conv2d_7/kernel'] * r, rtol=1e-6)
  np.testing.assert_allclose(b, w['batch_normalization_7/beta'] - w['batch_normalization_7/moving_mean'] * r,
                             rtol=1e-6, atol=1e-7)


def test_restatement_preprocess_is_the_reference_chain():
  """The NumPy statement used by the GPU tests: roll, flip, crop, resize to the same size = copy."""
  import _inception_ref as ref
  rng = np.random.default_rng(6)
  x = rng.uniform(0, 1, (1, 16, 12, 3)).astype(np.float32)
  y = ref.preprocess_np(x, [(3, 1)], out=12)   # crop 2 + 2 rows -> 12 x 12: an identity resize
  want = np.roll(x[0], 3, axis=1)[:, ::-1][2:14] * 2 - 1
  np.testing.assert_allclose(y[0], want, atol=1e-6)


def test_checkpoint_keys_follow_keras_layers_order():
  """layer_with_weights-<k> counts the weighted layers in model.layers order (depth to the output,
  deepest first; ties by the depth-first index from the output), not in creation order.  Indices
  derived by hand from that rule: the stem chain is k = 0..9 in creation order; after the stem's
  second max pool the deepest layer is mixed0's 3x3dbl 1x1 (conv2d_8: 9 layers to the concatenation),
  then conv2d_6 / conv2d_9 tie at 6 (conv2d_6's branch is listed first in the concatenation)."""
  order = iu.keras_layer_order()
  assert len(order) == 313   # Keras: len(InceptionV3(include_top=True).layers)
  assert order[0] == 'input' and order[-2:] == ['avg_pool', 'predictions']
  keys = iu.bundle_keys()

  def k(name):
    return int(keys[name].split('/')[1].split('-')[1])

  for i in range(5):
    assert k(iu._name('conv2d', i) + '/kernel') == 2 * i
    assert k(iu._name('batch_normalization', i) + '/beta') == 2 * i + 1
  assert k('conv2d_8/kernel') == 10 and k('batch_normalization_8/moving_mean') == 11
  assert k('conv2d_6/kernel') == 12 and k('conv2d_9/kernel') == 13
  assert k('batch_normalization_6/beta') == 14 and k('batch_normalization_9/beta') == 15
  assert [k(f'conv2d_{i}/kernel') for i in (5, 7, 10, 11)] == [16, 17, 18, 19]
  assert k('predictions/kernel') == k('predictions/bias') == 188
  assert keys['conv2d_8/kernel'] == 'inception_v3/layer_with_weights-10/kernel' + SUFFIX
  # every variable of a layer shares its index; the indices are 0..188 without gaps
  assert sorted({k(n) for n in keys}) == list(range(189))
