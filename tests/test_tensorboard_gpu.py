"""TensorBoard summaries from the training and the evaluation loop on the GPU: GANManager.train /
test with a utils/logger.UniversalLogger -> event file -> scalars and the nine image grids, PNG-encoded
on the device; the roll-out PNGs of test() under png_encoder='device'; no logger, no file."""
import os

import numpy as np
import pytest
import torch

import _video_input_ref as ref
from se3ds_amd import gin_lite
from se3ds_amd.models import image_models
from se3ds_amd.utils import image_grid, inception_utils as iu, logger as logger_lib, png, tf_events

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE, T, BATCH, SEQ = 64, 3, 2, 3
SPLIT = 'val_seen'
FAMILIES = ['_raw_generated', '_ema_generated', '_pred_depth', '_ema_pred_depth', '_real_img',
            '_real_depth', '_projected', '_blur_bbox', '_proj_mask']


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


def _train_batch(n, h, seed):
  """A single-frame training batch: the keys GAN.train_g_d reads."""
  g = torch.Generator().manual_seed(seed)
  w = 2 * h
  image = torch.rand((n, h, w, 3), generator=g)
  depth = torch.rand((n, h, w, 1), generator=g)
  pm = (torch.rand((n, h, w, 1), generator=g) < 0.5).float()
  bm = torch.zeros((n, h, w, 1))
  bm[:, :h // 8] = 1
  bm[:, -(h // 8):] = 1
  batch = dict(image=image, depth=depth, proj_mask=pm, proj_image=image * pm, proj_depth=depth * pm,
               blurred_mask=bm)
  return {k: v.to(DEV) for k, v in batch.items()}


def _display_batch(examples):
  from se3ds_amd.datasets import indoor_datasets
  return next(indoor_datasets.R2RVideoDataset().input_fn(examples, BATCH, seed=0, device=DEV))


def _record_rollouts(gan):
  """Wraps gan._get_image_grid so that the roll-outs it returns can be looked at afterwards."""
  seen, inner = [], gan._get_image_grid

  def wrapped(inputs, modes=('normal', 'ema')):
    out = inner(inputs, modes=modes)
    seen.append((inputs, out))
    return out
  gan._get_image_grid = wrapped
  return seen


def _expected_sheets(gan, inputs, rollouts, prefix):
  """The nine families restated from the reference (trainers/gan_manager.py:558-598), each through
  get_grid_image on its own."""
  normal, ema = rollouts['normal'], rollouts['ema']
  cat = lambda xs: torch.cat([x.float() for x in xs], dim=0)
  sources = {
      '_raw_generated': cat(normal.generated), '_ema_generated': cat(ema.generated),
      '_pred_depth': cat(normal.pred_depth), '_ema_pred_depth': cat(ema.pred_depth),
      '_real_img': cat([inputs['image'][:, k] for k in range(SEQ)]),
      '_real_depth': cat([inputs['depth'][:, k] for k in range(SEQ)]),
      '_projected': cat(normal.projected), '_blur_bbox': torch.zeros_like(cat(normal.pred_depth)),
      '_proj_mask': cat(normal.proj_mask)}
  return {prefix + k: image_grid.get_grid_image(v, gan.show_num, None, out_c=3) for k, v in sources.items()}


def _check_grids(events, step, sheets):
  images = {tag: v for _, s, values in events for tag, v in values.items()
            if isinstance(v, tuple) and s == step}
  assert sorted(images) == sorted(sheets)
  decoded = png.decode_png_batch({tag: [data] for tag, (_, _, data) in images.items()}, DEV)
  for tag, sheet in sheets.items():
    h, w, _ = images[tag]
    assert tuple(sheet.shape) == (1, 2 * SIZE, 3 * 2 * SIZE, 3) == (1, h, w, 3)   # 6 frames: 2 x 3
    assert torch.equal(decoded[tag], sheet), tag
  assert float(sheets[[t for t in sheets if t.endswith('_real_img')][0]].float().std()) > 1.0


def _event_files(root):
  return [os.path.join(d, f) for d, _, files in os.walk(root) for f in files if 'tfevents' in f]


@pytest.fixture(scope='module')
def examples():
  return ref.synth_examples(2 * BATCH, T, 2 * SIZE, seed=31)


@pytest.fixture(scope='module')
def inception():
  return iu.inception_model(init='random', seed=12, device=DEV)


def test_train_writes_scalars_and_grids(tmp_path, examples):
  try:
    gan = _make_gan(str(tmp_path))
    gan._create_obj()
    display = _display_batch(examples)
    seen = _record_rollouts(gan)
    gan.log_every_steps, gan.save_every_steps, gan.global_step = 2, 2, 2
    lines = []
    log = logger_lib.UniversalLogger(os.path.join(str(tmp_path), 'logs'), step=2, logging_fn=lines.append)
    gan.train(train_ds=[_train_batch(BATCH, SIZE, 5)], num_train_steps=3, logger=log,
              display_batch=display)
    log.close()
    assert gan.global_step == 3 and len(seen) == 1
    files = _event_files(str(tmp_path))
    assert files == [log.summary_writer.path]
    events = list(tf_events.read_events(files[0]))
    scalars = {tag: (s, v) for _, s, values in events for tag, v in values.items() if not isinstance(v, tuple)}
    # the trainer's metric names, as the reference has them: gen/gen_loss, dis/disc_loss, ...
    assert set(scalars) == set(gan.metrics) and {'gen/gen_loss', 'dis/disc_loss'} <= set(scalars)
    for tag, (step, value) in scalars.items():
      assert step == 2 and np.isfinite(value), tag
    assert len(lines) == 1 and lines[0].startswith('[2] ') and 'gen_loss = ' in lines[0]
    sheets = _expected_sheets(gan, *seen[0], 'train')
    assert sorted(sheets) == sorted('train' + f for f in FAMILIES)
    _check_grids(events, 2, sheets)
  finally:
    gin_lite.clear_config()


def test_test_loop_writes_scalars_grids_and_device_pngs(tmp_path, examples, inception):
  try:
    model_dir = str(tmp_path)
    gan = _make_gan(model_dir)
    seen = _record_rollouts(gan)
    log = logger_lib.UniversalLogger(os.path.join(model_dir, 'logs'), step=0, logging_fn=lambda s: None)
    rows = gan.test(eval_examples=examples, unit_test=True, inception=inception, logger=log)
    log.close()
    assert len(rows) == 1 and len(seen) == 1
    events = list(tf_events.read_events(log.summary_writer.path))
    scalars = {tag: (s, v) for _, s, values in events for tag, v in values.items() if not isinstance(v, tuple)}
    keys = [k for k in rows[0] if k not in ('checkpoint_path', 'step')]
    assert sorted(scalars) == sorted(keys) and len(keys) == 4 * (SEQ - 1)
    for k in keys:
      assert scalars[k] == (1, np.float32(float(rows[0][k]))), k
    _check_grids(events, 1, _expected_sheets(gan, *seen[0], SPLIT))

    # the roll-out PNGs: the device encoder's files hold the pixels of the host encoder's
    rollout = seen[0][1]['ema']
    assert gan.png_encoder == 'host'
    gan._save_rollout_images(rollout, 7)
    gan.png_encoder = 'device'
    gan._save_rollout_images(rollout, 8)
    root = os.path.join(model_dir, 'images', SPLIT)
    names = sorted(os.path.join(str(f), f'{e}_{s}.png') for f in range(SEQ) for e in range(BATCH)
                   for s in ('rgb', 'depth'))
    for name in names:
      host = open(os.path.join(root, '7', name), 'rb').read()
      device = open(os.path.join(root, '8', name), 'rb').read()
      assert host != device   # filter 0 + zlib level 6 against adaptive filters + runs
      both = png.decode_png_batch({'host': [host], 'device': [device]}, DEV)
      shape = (1, SIZE, 2 * SIZE, 3) if name.endswith('rgb.png') else (1, SIZE, 2 * SIZE)
      assert tuple(both['host'].shape) == shape and torch.equal(both['host'], both['device']), name
    gan.png_encoder = 'gpu'
    with pytest.raises(ValueError, match='png_encoder'):
      gan._save_rollout_images(rollout, 9)
  finally:
    gin_lite.clear_config()


def test_no_logger_no_event_file(tmp_path, examples, inception):
  try:
    gan = _make_gan(str(tmp_path))
    gan._create_obj()
    gan.log_every_steps, gan.save_every_steps, gan.global_step = 2, 2, 2
    gan.train(train_ds=[_train_batch(BATCH, SIZE, 5)], num_train_steps=3,
              display_batch=_display_batch(examples))
    gan.test(eval_examples=examples, unit_test=True, inception=inception)
    assert os.path.isfile(os.path.join(str(tmp_path), f'scores_{SPLIT}.csv'))
    assert _event_files(str(tmp_path)) == []
  finally:
    gin_lite.clear_config()
