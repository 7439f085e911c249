"""Checkpoints written from the training loop on an MI355X: GANManager.save_checkpoint_async (device
CRC-32, snapshot, writer thread) against state_dict() / save_checkpoint, and train(checkpoints=...,
resume=..., max_to_keep=...).  Every comparison is bit-exact; nothing asserts a time."""
import os
import threading

import numpy as np
import pytest
import torch

from se3ds_amd import gin_lite
from se3ds_amd.models import image_models

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE = 64


def _make_gan(model_dir, **kw):
  """The tiny GAN of tests/test_gan_test_loop_gpu.py: 64 x 128, gen_dims = 8."""
  from se3ds_amd.trainers import gan_manager, se3ds_trainer
  gin_lite.clear_config()
  gin_lite.parse_config('''
image_models.ResNetGenerator.gen_dims = 8
image_models.ResNetGenerator.z_dim = 4
image_models.ResNetGenerator.resnet_version = "50"
image_models.SNMultiScaleDiscriminator.dis_dims = 4
image_models.SNMultiScaleDiscriminator.n_dis = 2
image_models.SNMultiScaleDiscriminator.n_layers = 3
''')
  gan = se3ds_trainer.GAN(
      strategy=gan_manager.OneDeviceStrategy(DEV), model_dir=model_dir, lambda_gan=1.0,
      lambda_kld=10.0, lambda_wc=10.0, lambda_depth=100.0, mask_blurred=True, predict_depth=True,
      image_size=SIZE, beta1=0.5, g_lr=1e-4, d_lr=4e-4, d_step_per_g_step=1, num_batched_steps=1,
      generator_fn=image_models.ResNetGenerator,
      discriminator_fn=image_models.SNMultiScaleDiscriminator, seed=0, compute_dtype=torch.float32, **kw)
  gan._create_obj()
  return gan


def _synth_batch(n, h, seed):
  """The constant synthetic batch of tests/test_nets_gpu.py."""
  g = torch.Generator().manual_seed(seed)
  w = 2 * h
  image = torch.rand((n, h, w, 3), generator=g)
  depth = torch.rand((n, h, w, 1), generator=g)
  poison = torch.rand((n, h, w, 1), generator=g)
  depth = torch.where(poison < 0.02, torch.zeros_like(depth), depth)
  depth = torch.where(poison > 0.99, torch.ones_like(depth), depth)
  pm = (torch.rand((n, h, w, 1), generator=g) < 0.5).float()
  pm[:, h // 3:h // 3 + max(1, h // 8)] = 0
  bm = torch.zeros((n, h, w, 1))
  bm[:, :h // 8] = 1
  bm[:, -(h // 8):] = 1
  batch = dict(image=image, depth=depth, proj_mask=pm, proj_image=image * pm, proj_depth=depth * pm,
               blurred_mask=bm)
  return {k: v.to(DEV) for k, v in batch.items()}


@pytest.fixture(scope='module')
def batch():
  return _synth_batch(2, SIZE, seed=83)


def _forever(batch):
  while True:
    yield batch


def _two_steps(gan, batch):
  for _ in range(2):
    gan.train_g_d(batch)
    gan.global_step += 1
  torch.cuda.synchronize()


def _assert_file_is(path, state):
  with np.load(path) as f:
    assert sorted(f.files) == sorted(state)
    for k, want in state.items():
      got = f[k]   # np.load checks the member's CRC-32: the device checksum, independently
      assert got.dtype == want.dtype and got.shape == want.shape, k
      assert got.tobytes() == want.tobytes(), k
  assert not os.path.exists(path + '.tmp')


def _arenas(gan):
  return [gan.generator.store.theta, gan.generator.store.state, gan.discriminator.store.theta,
          gan.discriminator.store.state, gan.ema_generator.store.theta, gan.ema_generator.store.state,
          gan.g_optimizer.m, gan.g_optimizer.v, gan.d_optimizer.m, gan.d_optimizer.v]


def _assert_same_state(a, b):
  for x, y in zip(_arenas(a), _arenas(b)):
    assert torch.equal(x, y)
  assert (a.global_step, a.g_optimizer.iterations, a.d_optimizer.iterations) == (
      b.global_step, b.g_optimizer.iterations, b.d_optimizer.iterations)


def test_same_contents_as_the_synchronous_save(tmp_path, batch):
  gan = _make_gan(str(tmp_path))
  _two_steps(gan, batch)
  state = gan.state_dict()
  largest = max(v.nbytes for v in state.values())
  total = sum(v.nbytes for v in state.values())
  # slabs: the default (one slab holds everything), several slabs with a member that spans two,
  # and slabs smaller than most members
  for staging in (2 * (256 << 20), 2 * (largest // 2 // 16 * 16 + 16), 2 * 4096):
    assert staging == 2 * (256 << 20) or total > 3 * (staging // 2)
    for snapshot in ('device', 'direct'):
      path = str(tmp_path / f'{snapshot}-{staging}.npz')
      handle = gan.save_checkpoint_async(path, snapshot=snapshot, staging_bytes=staging)
      assert handle.wait() == path and handle.done
      _assert_file_is(path, state)
  ref = str(tmp_path / 'sync.npz')
  gan.save_checkpoint(ref)
  with np.load(ref) as f:
    assert sorted(f.files) == sorted(state)
  with pytest.raises(ValueError):
    gan.save_checkpoint_async(ref, snapshot='host')


def test_the_file_is_the_state_at_the_save_whatever_runs_next(tmp_path, batch):
  gan = _make_gan(str(tmp_path))
  _two_steps(gan, batch)
  state = gan.state_dict()
  gate, calls = threading.Event(), []

  def hook():
    calls.append(threading.current_thread().name)
    assert gate.wait(60)

  path = str(tmp_path / 'held.npz')
  # a second save is requested while this one is in flight, below: it first waits for it
  handle = gan.save_checkpoint_async(path, snapshot='device', staging_bytes=2 * 65536, writer_hook=hook)
  _two_steps(gan, batch)                     # the trainer runs on while the writer is held
  assert not handle.done and not os.path.exists(path)
  later = gan.state_dict()
  assert any(later[k].tobytes() != state[k].tobytes() for k in state)
  gate.set()
  second = str(tmp_path / 'second.npz')
  handle2 = gan.save_checkpoint_async(second, snapshot='device', staging_bytes=2 * 65536)
  assert handle.done and os.path.exists(path)
  handle2.wait()
  _assert_file_is(path, state)
  _assert_file_is(second, later)
  assert len(calls) > 2 and set(calls) == {calls[0]} and calls[0] != threading.main_thread().name


def test_restore_parity(tmp_path, batch):
  a = _make_gan(str(tmp_path))
  _two_steps(a, batch)
  path = str(tmp_path / 'ckpt.npz')
  a.save_checkpoint_async(path, staging_bytes=2 * 65536).wait()
  a.train_g_d(batch)
  b = _make_gan(str(tmp_path))
  assert b.restore_checkpoint(path) == []
  assert b.global_step == 2 and b.g_optimizer.iterations == 2
  b.train_g_d(batch)
  for x, y in ((a.generator.store.theta, b.generator.store.theta),
               (a.generator.store.state, b.generator.store.state),
               (a.discriminator.store.theta, b.discriminator.store.theta),
               (a.ema_generator.store.theta, b.ema_generator.store.theta),
               (a.g_optimizer.m, b.g_optimizer.m), (a.d_optimizer.v, b.d_optimizer.v)):
    assert torch.equal(x, y)


@pytest.mark.parametrize('mode', ['async', 'sync'])
def test_train_writes_the_schedule_of_the_reference(tmp_path, batch, mode):
  model_dir = str(tmp_path)
  gan = _make_gan(model_dir, save_every_steps=2)
  seen = []
  prune = gan._prune_checkpoints

  def spy(max_to_keep):   # the files in place each time one has just been added
    seen.append(sorted(n for n in os.listdir(model_dir)))
    prune(max_to_keep)
  gan._prune_checkpoints = spy
  gan.train(_forever(batch), num_train_steps=7, checkpoints=mode, max_to_keep=2, staging_bytes=2 * 65536)
  # step > 1 and step % 2 < 1 for step in 0 .. 6, then num_train_steps; two are kept
  assert seen == [['ckpt-2.npz'], ['ckpt-2.npz', 'ckpt-4.npz'], ['ckpt-2.npz', 'ckpt-4.npz', 'ckpt-6.npz'],
                  ['ckpt-4.npz', 'ckpt-6.npz', 'ckpt-7.npz']]
  assert sorted(os.listdir(model_dir)) == ['ckpt-6.npz', 'ckpt-7.npz']     # the newest two, no .tmp
  assert gan._unevaluated_checkpoints() == [os.path.join(model_dir, n) for n in ('ckpt-6.npz', 'ckpt-7.npz')]
  with np.load(os.path.join(model_dir, 'ckpt-6.npz')) as f:
    assert int(f['global_step']) == 6 and int(f['g_optimizer/iter']) == 7   # saved before the increment
  with np.load(os.path.join(model_dir, 'ckpt-7.npz')) as f:
    assert int(f['global_step']) == 7 and int(f['g_optimizer/iter']) == 7
  assert gan.global_step == 7


def test_train_resumes_from_the_highest_step(tmp_path, batch):
  model_dir = str(tmp_path)
  a = _make_gan(model_dir, save_every_steps=2)
  a.train(_forever(batch), num_train_steps=5, checkpoints='async', staging_bytes=2 * 65536)
  assert sorted(os.listdir(model_dir)) == ['ckpt-2.npz', 'ckpt-4.npz', 'ckpt-5.npz']
  os.remove(os.path.join(model_dir, 'ckpt-5.npz'))
  latest = os.path.join(model_dir, 'ckpt-4.npz')
  # ckpt-4 holds global_step 4 and five optimiser iterations: the resumed loop runs steps 4, 5, 6
  b = _make_gan(model_dir, save_every_steps=2)
  b.train(_forever(batch), num_train_steps=7, resume=True)
  assert b.restored_from == latest and b.global_step == 7
  assert sorted(os.listdir(model_dir)) == ['ckpt-2.npz', 'ckpt-4.npz']     # checkpoints=None writes nothing
  c = _make_gan(model_dir, save_every_steps=2)
  c.restore_checkpoint(latest)
  assert c.global_step == 4 and c.g_optimizer.iterations == 5
  c.train_ds = _forever(batch)
  for _ in range(3):
    c.train_cluster(1)
    c.global_step += 1
  _assert_same_state(b, c)
  # nothing to resume from: starts from initialisation; and today's behaviour writes nothing
  empty = str(tmp_path / 'empty')
  os.mkdir(empty)
  d = _make_gan(empty, save_every_steps=2)
  d.train(_forever(batch), num_train_steps=1, resume=True)
  assert d.restored_from is None
  d.train(_forever(batch), num_train_steps=4)
  assert os.listdir(empty) == []


def test_a_writer_failure_surfaces(tmp_path, batch):
  gan = _make_gan(str(tmp_path / 'missing' / 'dir'), save_every_steps=2)   # nothing can be written there
  _two_steps(gan, batch)
  handle = gan.save_checkpoint_async(str(tmp_path / 'missing' / 'x.npz'))
  with pytest.raises(OSError):
    handle.wait()
  assert handle.done
  with pytest.raises(OSError):               # the next save raises the failure of the last one too
    gan.save_checkpoint_async(str(tmp_path / 'ok.npz'))
  gan.save_checkpoint_async(str(tmp_path / 'ok.npz')).wait()
  assert sorted(os.listdir(str(tmp_path))) == ['ok.npz']
  with pytest.raises(OSError):
    gan.train(_forever(batch), num_train_steps=6, checkpoints='async')
  gan.wait_for_checkpoint()                  # the failure was raised once; nothing is in flight
