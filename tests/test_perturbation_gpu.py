"""Device half of the VLN perturbation augmentation on an MI355X: `se3ds_collision_count`
(csrc/perturb.hip) through se3ds_amd/inference/perturbation_utils.py against the NumPy restatement
of the reference function (tests/_perturbation_ref.py) -- counts, areas and proportions are
integers or one exact binary64 division, so every comparison is bit-exact -- and the augmentation
loop with its batched rendering (SE3DSModel.predict_views)."""
import math
import types

import numpy as np
import pytest
import torch

import _perturbation_ref as ref
from se3ds_amd import _lib
from se3ds_amd import gin_lite
from se3ds_amd.inference import perturbation_utils as pu

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def _all_offsets():
  return np.concatenate([ref.seeded_offsets(), ref.special_offsets()])


def _depth(shape, seed):
  """Depths of 0 ... 3 m against thresholds of 0.1 ... 2.3 m, with a few NaN, 0 and 1."""
  rng = np.random.default_rng(seed)
  d = rng.uniform(0, 0.15, shape).astype(F32)
  poison = rng.uniform(0, 1, shape)
  d[poison < 0.02] = 0
  d[poison > 0.98] = 1
  d[(poison > 0.5) & (poison < 0.51)] = np.nan
  return d


def _expect(offsets, depth_np, index=None, padding=0.10):
  count, area, prop = [], [], []
  for c, off in enumerate(offsets):
    img = depth_np if depth_np.ndim == 2 else depth_np[0 if index is None else index[c]]
    p, n, a = ref.get_proportion_invalid_for_depth(off, img, padding)
    count.append(n)
    area.append(a)
    prop.append(p)
  return np.array(count, np.int32), np.array(area, np.int32), np.array(prop, np.float64)


def _check(res, want):
  count, area, prop = want
  assert res.count.dtype == torch.int32 and res.area.dtype == torch.int32
  assert res.proportion.dtype == torch.float64
  np.testing.assert_array_equal(res.count.cpu().numpy(), count)
  np.testing.assert_array_equal(res.area.cpu().numpy(), area)
  got = res.proportion.cpu().numpy()
  assert np.array_equal(np.isnan(got), np.isnan(prop))
  assert np.array_equal(got[~np.isnan(prop)], prop[~np.isnan(prop)])   # bit-exact binary64


# 64x128 the reference's shape; 6x12 thresholds 2 and 1; 37x75 odd width (no row segment 16-byte
# aligned); 100x200 windows clipped at all four borders and at the seam; 2x24 empty windows
@pytest.mark.parametrize('shape', [(64, 128), (6, 12), (37, 75), (100, 200), (2, 24)])
def test_counts_bit_exact(shape):
  offs = _all_offsets()
  depth = _depth(shape, seed=shape[0])
  res = pu.get_proportion_invalid_batch(offs, torch.from_numpy(depth).to(DEV))
  want = _expect(offs, depth)
  _check(res, want)
  if shape == (2, 24):
    assert np.all(want[1] == 0) and np.all(res.count.cpu().numpy() == 0)
    assert np.all(np.isnan(res.proportion.cpu().numpy()))
  else:
    assert want[0].max() > 0 and np.any(want[0] < want[1])   # the case can tell hits from misses
  if shape == (100, 200):
    win, _ = pu.collision_windows(offs, *shape)
    assert (win[:, 0] == 0).any() and (win[:, 1] == 100).any()
    assert (win[:, 2] == 0).any() and (win[:, 3] == 200).any()


def test_counts_bit_exact_512x1024_k64():
  """The window (up to 340 rows x 170 columns) is wider than a wave's 64 lanes and has more rows
  than one workgroup's block."""
  offs = _all_offsets()[:64]
  depth = _depth((512, 1024), seed=512)
  res = pu.get_proportion_invalid_batch(offs, torch.from_numpy(depth).to(DEV))
  assert res.count.shape == (64,)
  want = _expect(offs, depth)
  assert want[1].max() == 340 * 170
  _check(res, want)


def test_counts_several_images_shuffled_index():
  offs = _all_offsets()
  depth = _depth((3, 37, 75), seed=3)
  index = np.random.default_rng(4).permutation(np.arange(len(offs)) % 3).astype(np.int32)
  res = pu.get_proportion_invalid_batch(offs, torch.from_numpy(depth).to(DEV), image_index=index)
  _check(res, _expect(offs, depth, index))
  # the images differ: the index matters
  assert not np.array_equal(_expect(offs, depth, index)[0], _expect(offs, depth, np.zeros_like(index))[0])
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    pu.get_proportion_invalid_batch(offs[:2], torch.from_numpy(depth).to(DEV), image_index=[0, 3])


def test_counts_single_candidate():
  off = ref.seeded_offsets()[5:6]
  depth = _depth((64, 128), seed=1)
  _check(pu.get_proportion_invalid_batch(off, torch.from_numpy(depth).to(DEV)), _expect(off, depth))


def test_threshold_edge_strict_fp32_compare_and_nan():
  """Offset [0, 1, 0] with padding 0.25: the threshold is exactly 1.25 = 0.0625 * 20.  Of the
  depths {just below 0.0625, 0.0625, just above, NaN} only the first is closer."""
  below, above = np.nextafter(F32(0.0625), F32(0)), np.nextafter(F32(0.0625), F32(1))
  values = np.array([below, F32(0.0625), above, F32(np.nan)], F32)
  assert F32(below * F32(20)) < F32(1.25) and F32(above * F32(20)) > F32(1.25)
  pick = np.random.default_rng(9).integers(0, 4, (64, 128))
  depth = values[pick]
  off = np.array([[0, 1, 0]], F32)
  win, dist = pu.collision_windows(off, 64, 128)
  assert F32(dist[0] + F32(0.25)) == F32(1.25)
  r0, r1, c0, c1 = (int(v) for v in win[0])
  res = pu.get_proportion_invalid_batch(off, torch.from_numpy(depth).to(DEV), distance_padding=0.25)
  n_first = int((pick[r0:r1, c0:c1] == 0).sum())
  assert 0 < n_first < (r1 - r0) * (c1 - c0)
  assert int(res.count.cpu()[0]) == n_first
  _check(res, _expect(off, depth, padding=0.25))


def test_count_is_overwritten_and_inputs_untouched():
  """The C entry point on buffers of the test's own: count holds garbage before the call."""
  offs = _all_offsets()
  depth_np = _depth((37, 75), seed=8)
  depth = torch.from_numpy(depth_np).to(DEV)
  before = depth.clone()
  win, dist = pu.collision_windows(offs, 37, 75)
  k = len(offs)
  d_win = torch.from_numpy(win).to(DEV)
  d_thr = torch.from_numpy(dist + F32(0.1)).to(DEV)
  count = torch.full((k,), 0x7f0f0f0f, dtype=torch.int32, device=DEV)
  want = _expect(offs, depth_np)[0]
  for _ in range(2):   # the second call starts from the first one's result, not from zero
    _lib.check(_lib.lib().se3ds_collision_count(
        depth.data_ptr(), 1, 37, 75, d_win.data_ptr(), None, d_thr.data_ptr(), 20.0, k,
        count.data_ptr(), _lib.stream()), 'se3ds_collision_count')
    np.testing.assert_array_equal(count.cpu().numpy(), want)
  assert torch.equal(depth.view(torch.int32), before.view(torch.int32))
  np.testing.assert_array_equal(d_win.cpu().numpy(), win)


def test_single_equals_batch_and_reference_known_answers():
  offs = _all_offsets()[40:56]
  depth_np = _depth((64, 128), seed=2)
  depth = torch.from_numpy(depth_np).to(DEV)
  batch = pu.get_proportion_invalid_batch(offs, depth).proportion.cpu().numpy()
  for c, off in enumerate(offs):
    p = pu.get_proportion_invalid_for_depth(off, depth)
    assert isinstance(p, float) and p == batch[c] == ref.get_proportion_invalid_for_depth(off, depth_np)[0]
  assert math.isnan(pu.get_proportion_invalid_for_depth(offs[0], torch.zeros((2, 24), device=DEV)))
  # inference/perturbation_utils_test.py's five expectations on the device path
  h, w = 64, 128
  dev = lambda a: torch.from_numpy(np.asarray(a, F32)).to(DEV)
  f = pu.get_proportion_invalid_for_depth
  assert f(torch.tensor([0.0, 0.5, 0.0]), dev(np.full((h, w), 0.5 / 20.0))) == 1.0
  assert f(torch.tensor([0.0, 0.3, 0.0]), dev(np.full((h, w), 0.5 / 20.0))) == 0.0
  def patch(r0, r1, c0, c1):
    d = np.full((h, w), 1.0, F32)
    d[r0:r1, c0:c1] = 0.0
    return dev(d)
  assert f([0.0, 0.5, 0.0], patch(22, 42, 54, 74)) > 0.0
  assert f([0.0, 0.5, 0.0], patch(0, 10, 0, 10)) == 0.0
  assert f([0.5, 0.5, 0.0], patch(38, 58, 86, 106)) > 0.0
  assert f([0.5, 0.5, 0.0], patch(0, 10, 0, 10)) == 0.0


# ------------------------------------------------------------------------------ the loop
SIZE = 128


@pytest.fixture(scope='module')
def scene():
  """get_test_config() at image_height 128 with one random panorama in the memory (the set-up of
  test_nets_gpu.py's SE3DSModel test) and inference state as test_configs_gpu.py's cfg2 gives it."""
  from se3ds_amd.models import model_config, models
  from tests.test_configs_gpu import _randomise_inference_state
  gin_lite.clear_config()
  g = torch.Generator().manual_seed(3)
  rgb = torch.randint(0, 255, (1, SIZE, SIZE * 2, 3), generator=g, dtype=torch.int32).to(torch.uint8)
  seg = torch.randint(0, 42, (1, SIZE, SIZE * 2, 1), generator=g, dtype=torch.int32).to(torch.uint8)
  depth = torch.rand((1, SIZE, SIZE * 2), generator=g)
  pos = torch.randn((1, 3), generator=g)
  config = model_config.get_test_config()
  config.image_height = SIZE
  model = models.SE3DSModel(config, device=DEV)
  _randomise_inference_state(model.model)
  model.add_to_memory(rgb.to(DEV), seg.to(DEV), depth.to(DEV), pos.to(DEV), mask_blurred=False)
  return types.SimpleNamespace(model=model, config=config, rgb=rgb, seg=seg, depth=depth, pos=pos)


def _screen_depth(kind):
  d = np.full((SIZE, 2 * SIZE), 0.9, F32)       # 18 m: (almost) every candidate passes
  if kind == 'wall':
    d[:, :SIZE] = 0.02                         # 0.4 m on one half of the headings: those fail
  return d


@pytest.mark.parametrize('kind', ['open', 'wall'])
def test_augment_equals_the_notebook_loop(scene, kind):
  model, start = scene.model, scene.pos.to(DEV)
  depth_np = _screen_depth(kind)
  depth = torch.from_numpy(depth_np).to(DEV)
  memory = model.get_memory_state()
  got = pu.perturbation_augment(model, num_samples=3, start_pos=start, depth=depth[None], seed=1,
                                views_per_forward=1)
  # notebook cell 13 written out: the same draws, the single-candidate function, model(pos)
  rng = np.random.default_rng(1)
  images, offsets, props, drawn, rejected = [], [], [], 0, 0
  while len(images) < 3:
    if drawn % 64 == 0:
      cand = pu.draw_candidates(rng, 64, 1.5, 0.1)
    noise = cand[drawn % 64]
    drawn += 1
    p = pu.get_proportion_invalid_for_depth(noise, depth, distance_padding=0.1)
    assert p == ref.get_proportion_invalid_for_depth(noise, depth_np, 0.1)[0]
    if p < 0.02:
      curr_pos = start + torch.from_numpy(noise[None]).to(DEV)
      outputs = model(curr_pos, add_preds_to_memory=False)
      images.append(outputs.pred_rgb[0])
      offsets.append(noise)
      props.append(p)
    else:
      rejected += 1
  assert rejected > 0 if kind == 'wall' else rejected == 0
  assert got.num_drawn == drawn
  np.testing.assert_array_equal(got.offsets, np.stack(offsets))
  np.testing.assert_array_equal(got.proportion_invalid, np.array(props, np.float64))
  assert got.images.dtype == torch.uint8 and tuple(got.images.shape) == (3, SIZE, 2 * SIZE, 3)
  assert torch.equal(got.images, torch.stack(images))
  assert torch.equal(got.positions, start + torch.from_numpy(np.stack(offsets)).to(DEV))
  after = model.get_memory_state()
  assert all(torch.equal(a, b) for a, b in zip(memory, after))   # nothing joined the memory


def test_augment_raises_when_nothing_passes(scene):
  depth = torch.zeros((SIZE, 2 * SIZE), device=DEV)   # everything collides: proportion 1.0
  with pytest.raises(RuntimeError, match='after 2 rounds'):
    pu.perturbation_augment(scene.model, num_samples=1, start_pos=scene.pos.to(DEV), depth=depth,
                            candidates_per_round=8, max_rounds=2)


def test_predict_views_three_views(scene):
  """views_per_forward = 3: the projections are the batch-1 warp's, bit for bit; the generator's
  outputs are held against the CPU oracle per view with the tolerance of test_configs_gpu.py's
  cfg2 SE3DSModel comparison (_check_frame), because the conv route may depend on the batch."""
  from oracle import model_np
  from tests.test_configs_gpu import _check_frame, _cpu_params
  model, start = scene.model, scene.pos.to(DEV)
  depth = torch.from_numpy(_screen_depth('open')).to(DEV)
  got = pu.perturbation_augment(model, num_samples=3, start_pos=start, depth=depth, seed=1,
                                views_per_forward=3)
  out = model.predict_views(got.positions)
  assert torch.equal(got.images, out.pred_rgb) and tuple(got.images.shape) == (3, SIZE, 2 * SIZE, 3)
  cfg = scene.config
  oracle = model_np.SE3DSModelOracle(_cpu_params(model.model), SIZE, cfg.gen_dims, cfg.resnet_version,
                                     depth_scale=cfg.depth_scale, z_dim=cfg.z_dim)
  oracle.add_to_memory(scene.rgb.numpy(), scene.seg.numpy(), scene.depth.numpy(), scene.pos.numpy(),
                       mask_blurred=False)
  positions = got.positions.cpu().numpy()
  for v in range(3):
    single = model(got.positions[v:v + 1], add_preds_to_memory=False)
    for name in ('proj_rgb', 'proj_depth', 'proj_mask', 'proj_semantic'):
      assert torch.equal(getattr(out, name)[v:v + 1], getattr(single, name)), (v, name)
    view = types.SimpleNamespace(**{k: getattr(out, k)[v:v + 1] for k in (
        'proj_semantic', 'proj_rgb', 'proj_depth', 'proj_mask', 'pred_depth', 'pred_rgb',
        'pred_semantic')})
    e = _check_frame(view, oracle(positions[v:v + 1]), f'view {v}')
    print(f'predict_views view {v}: pred_depth err vs oracle {e:.2e}')
  with pytest.raises(ValueError):
    model.predict_views(got.positions[0])
