"""GANManager.test on the GPU: parsed trajectory examples -> R2RVideoDataset -> roll-out PNGs ->
EvalMetric -> scores_<split>.csv, for the unit-test pass and for saved checkpoints."""
import csv
import os

import numpy as np
import pytest
import torch

import _video_input_ref as ref
from se3ds_amd import gin_lite
from se3ds_amd.models import image_models
from se3ds_amd.utils import inception_utils as iu

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE, T, BATCH, SEQ = 64, 3, 2, 3
SPLIT = 'val_seen'


def _make_gan(model_dir):
  from se3ds_amd.trainers import gan_manager, se3ds_trainer
  gin_lite.clear_config()
  gin_lite.parse_config(f'''
image_models.ResNetGenerator.gen_dims = 8
image_models.ResNetGenerator.z_dim = 4
image_models.ResNetGenerator.resnet_version = "50"
image_models.SNMultiScaleDiscriminator.dis_dims = 4
image_models.SNMultiScaleDiscriminator.n_dis = 2
image_models.SNMultiScaleDiscriminator.n_layers = 3
R2RVideoDataset.image_size = {SIZE}
R2RVideoDataset.preprocessed_image_height = {2 * SIZE}
R2RVideoDataset.video_length = {T}
''')
  return se3ds_trainer.GAN(
      strategy=gan_manager.OneDeviceStrategy(DEV), model_dir=model_dir, lambda_gan=1.0,
      lambda_kld=10.0, lambda_wc=10.0, lambda_depth=100.0, mask_blurred=True, predict_depth=True,
      image_size=SIZE, beta1=0.5, g_lr=1e-4, d_lr=4e-4, d_step_per_g_step=1, num_batched_steps=1,
      generator_fn=image_models.ResNetGenerator,
      discriminator_fn=image_models.SNMultiScaleDiscriminator, seed=0, test_batch_size=BATCH,
      eval_size=None, test_split=SPLIT, eval_seq_len=SEQ, compute_dtype=torch.float32)


def _columns():
  return ['checkpoint_path', 'step'] + sorted(
      f'{SPLIT}/eval_image/{k}@{i}' for k in ('fid', 'ema_fid', 'rmse', 'ema_rmse')
      for i in range(1, SEQ))


def _read(model_dir):
  with open(os.path.join(model_dir, f'scores_{SPLIT}.csv'), newline='') as f:
    reader = csv.DictReader(f)
    return reader.fieldnames, list(reader)


def _check_values(row):
  for k in _columns()[2:]:
    assert np.isfinite(float(row[k])), (k, row[k])
    assert row[k] == '{:.3f}'.format(float(row[k])), (k, row[k])


def _check_images(model_dir, step):
  for frame in range(SEQ):
    for example in range(BATCH):
      for suffix, channels in (('rgb', 3), ('depth', 1)):
        path = os.path.join(model_dir, 'images', SPLIT, str(step), str(frame),
                            f'{example}_{suffix}.png')
        assert os.path.isfile(path), path
        with open(path, 'rb') as f:
          px = ref.decode_png(f.read())
        assert px.shape == (SIZE, 2 * SIZE, channels) and px.dtype == np.uint8


def test_gan_manager_test_loop(tmp_path):
  """G7."""
  model_dir = str(tmp_path)
  examples = ref.synth_examples(2 * BATCH, T, 2 * SIZE, seed=31)
  inception = iu.inception_model(init='random', seed=12, device=DEV)
  try:
    gan = _make_gan(model_dir)
    rows = gan.test(eval_examples=examples, unit_test=True, inception=inception)
    assert gan.eval_num == 2 * BATCH and gan.global_batch_size == BATCH
    header, on_disk = _read(model_dir)
    assert header == _columns()
    assert len(rows) == len(on_disk) == 1 and dict(on_disk[0]) == rows[0]
    assert on_disk[0]['checkpoint_path'] == 'test-1' and on_disk[0]['step'] == '1'
    _check_values(on_disk[0])
    _check_images(model_dir, 1)

    # two saved checkpoints, written out of order: evaluated in step order, appended to the file
    gan.global_step = 40
    gan.save_checkpoint(os.path.join(model_dir, 'ckpt-40.npz'))
    gan.global_step = 20
    gan.save_checkpoint(os.path.join(model_dir, 'ckpt-20.npz'))
    rows = gan.test(eval_examples=examples, inception=inception)
    header, on_disk = _read(model_dir)
    assert header == _columns()
    assert [r['checkpoint_path'] for r in on_disk] == [
        'test-1', os.path.join(model_dir, 'ckpt-20.npz'), os.path.join(model_dir, 'ckpt-40.npz')]
    assert [r['step'] for r in on_disk] == ['1', '20', '40']
    assert [dict(r) for r in on_disk[1:]] == rows
    assert gan.global_step == 40   # restored from the last file
    for r in on_disk[1:]:
      _check_values(r)
    _check_images(model_dir, 20)
    _check_images(model_dir, 40)

    # nothing new: no row is added
    assert gan.test(eval_examples=examples, inception=inception) == []
    assert len(_read(model_dir)[1]) == 3

    # an explicit list is evaluated whether or not it has a row already
    rows = gan.test(eval_examples=examples, checkpoints=[os.path.join(model_dir, 'ckpt-20.npz')],
                    inception=inception)
    assert len(rows) == 1 and rows[0]['step'] == '20' and len(_read(model_dir)[1]) == 4

    with pytest.raises(ValueError):
      gan.test(inception=inception)
  finally:
    gin_lite.clear_config()


def test_gan_manager_test_needs_one_replica(tmp_path):
  gan = _make_gan(str(tmp_path))
  gin_lite.clear_config()

  class TwoReplicas:
    num_replicas_in_sync = 2
    group = None
    device = DEV
  gan.strategy = TwoReplicas()
  with pytest.raises(NotImplementedError):
    gan.test(eval_examples=ref.synth_examples(2, T, 2 * SIZE, seed=1), unit_test=True)
