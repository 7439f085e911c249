"""R2RVideoDataset: the evaluation side of the input pipeline.  CPU cases: gin wiring, the batching of
input_fn, the host draws, the NumPy restatement itself (tests/_video_input_ref.py) and the PNG writer.
GPU cases: se3ds_video_transform bit for bit against the restatement and against the op-by-op chain of
pano_utils.resize, buffer sharing, argument checks, the shipped size, and input_fn -> EvalMetric."""
import os
import zlib

import numpy as np
import pytest
import torch

import _video_input_ref as ref
from se3ds_amd import gin_lite
from se3ds_amd.datasets import indoor_datasets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
F32 = np.float32
OUT_KEYS = ('image', 'original_image', 'segmentation', 'pathdreamer_segmentation', 'depth',
            'pathdreamer_depth', 'position', 'position_xyz1', 'mask', 'depth_scale', 'dataset_type',
            'id')


# ----------------------------------------------------------------------------------------- CPU
def test_video_dataset_is_gin_configurable():
  """C1: the three R2RVideoDataset lines of the shipped low-resolution config reach the constructor."""
  gin_lite.clear_config()
  with open(os.path.join(ROOT, 'configs', 'lowres', 'lowres.gin')) as f:
    lines = [l for l in f.read().splitlines() if l.startswith('R2RVideoDataset.')]
  assert len(lines) == 3
  gin_lite.parse_config('\n'.join(lines))
  try:
    ds = indoor_datasets.R2RVideoDataset()
  finally:
    gin_lite.clear_config()
  assert ds.image_size == 128 and ds.preprocessed_image_height == 1024 and ds.data_dir == 'data/val/'
  assert ds.horizontal_mask_ratio == 0.0 and ds.video_length == 8 and ds.return_filename is False
  assert ds.num_examples == {'train': 4675, 'val_unseen': 783, 'val_seen': 340}
  assert ds.get_file_patterns('val_seen') == 'data/val/val_seen*.tfrecord'
  assert ds.get_file_patterns(file_pattern='x/*.tfrecord') == 'x/*.tfrecord'
  with pytest.raises(ValueError):
    ds.get_file_patterns('test')


def test_input_fn_batches_across_the_epoch_boundary():
  """C2: repeat comes before batch -- 3 examples in batches of 2 give (0,1), (2,0), (1,2), ...; one
  epoch gives one batch and drops the tail."""
  examples = [dict(id=np.int64(i), image=np.full((2, 3), i, F32)) for i in range(3)]
  it = indoor_datasets.R2RVideoDataset.batch_examples(examples, 2, num_epochs=None)
  got = [next(it) for _ in range(3)]
  assert [b['id'].tolist() for b in got] == [[0, 1], [2, 0], [1, 2]]
  assert got[1]['image'].shape == (2, 2, 3) and got[1]['image'].dtype == F32
  assert got[1]['image'][:, 0, 0].tolist() == [2.0, 0.0]
  one = list(indoor_datasets.R2RVideoDataset.batch_examples(examples, 2, num_epochs=1))
  assert [b['id'].tolist() for b in one] == [[0, 1]]
  # a callable is asked for a fresh iterator every epoch
  calls = []

  def fresh():
    calls.append(1)
    return iter(examples)
  two = list(indoor_datasets.R2RVideoDataset.batch_examples(fresh, 2, num_epochs=2))
  assert [b['id'].tolist() for b in two] == [[0, 1], [2, 0], [1, 2]] and len(calls) == 2
  with pytest.raises(ValueError):
    next(indoor_datasets.R2RVideoDataset.batch_examples([], 2))


def test_draw_params():
  """C3: no draw without a mask ratio; with one, the band of the reference (:753-757)."""
  rng = np.random.default_rng(5)
  before = rng.bit_generator.state
  assert indoor_datasets.R2RVideoDataset(image_size=64).draw_params(rng) == dict(hmask=None)
  assert rng.bit_generator.state == before
  ds = indoor_datasets.R2RVideoDataset(image_size=64, horizontal_mask_ratio=0.25)
  modes = set()
  for _ in range(500):
    mode, start, end = ds.draw_params(rng)['hmask']
    assert 0 <= start < 128 and 0 <= end < 128
    assert (mode == 2) == (start > end) and mode in (1, 2)
    modes.add(mode)
    # kept width 128 * 0.75: start + 96 < 256 rounds once in fp32 (half an ulp of [128, 256)), the
    # fp32 mod of that sum by 128 is exact
    assert abs((end - start) % 128 - 96) <= np.spacing(F32(128)) / 2
  assert modes == {1, 2}


def test_restatement_identity_and_no_clip():
  """C4: identity size returns the inputs, values outside [0, 1] included."""
  ex = ref.synth_examples(2, 2, 8, seed=1, lo=-0.2, hi=1.2)
  raw = {k: np.stack([e[k] for e in ex]) for k in ex[0]}
  assert raw['image'].min() < 0 and raw['image'].max() > 1
  out = ref.video_transform(raw, [dict(hmask=None)] * 2, 8)
  np.testing.assert_array_equal(out['original_image'], raw['image'])
  assert out['image'] is out['original_image']
  for k in ref.PLANES:
    np.testing.assert_array_equal(out[k], raw[k][..., None])
    assert out[k].dtype == raw[k].dtype
  np.testing.assert_array_equal(out['position'], raw['position'][..., :3])
  np.testing.assert_array_equal(out['position_xyz1'], raw['position'])


def test_restatement_exact_2x():
  """C4: an exact 2x reduction is, per 2x2 block, top + (bot - top) * 0.5 with top / bot the fp32
  lerps of the row pairs at 0.5; the nearest planes take the block's lower-right sample."""
  ex = ref.synth_examples(1, 2, 8, seed=2, lo=-0.2, hi=1.2)
  raw = {k: np.stack([e[k] for e in ex]) for k in ex[0]}
  out = ref.video_transform(raw, [dict(hmask=None)], 4)
  x = raw['image']
  half = F32(0.5)
  tl, tr = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2]
  bl, br = x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
  top = (tl + (tr - tl) * half).astype(F32)
  bot = (bl + (br - bl) * half).astype(F32)
  np.testing.assert_array_equal(out['original_image'], (top + (bot - top) * half).astype(F32))
  for k in ref.PLANES:
    np.testing.assert_array_equal(out[k][..., 0], raw[k][:, :, 1::2, 1::2])


def test_restatement_band_masks():
  """C4: wrapped and unwrapped bands zero exactly the complement columns."""
  ex = ref.synth_examples(3, 1, 8, seed=3, lo=0.1, hi=1.0)
  raw = {k: np.stack([e[k] for e in ex]) for k in ex[0]}
  params = [dict(hmask=None), dict(hmask=(1, 2.5, 9.0)), dict(hmask=(2, 12.0, 3.5))]
  out = ref.video_transform(raw, params, 8)
  keep = [set(range(16)), set(range(3, 9)), set(range(13, 16)) | set(range(0, 4))]
  for b in range(3):
    for x in range(16):
      col = out['image'][b, :, :, x]
      if x in keep[b]:
        np.testing.assert_array_equal(col, out['original_image'][b, :, :, x])
        assert (col != 0).all()
      else:
        assert (col == 0).all()
  # open interval: an integer bound is itself masked
  np.testing.assert_array_equal(ref.band_mask(8, (1, 2.0, 5.0)), [0, 0, 0, 1, 1, 0, 0, 0])


def test_png_helper_round_trips():
  """C5: decode the writer's bytes with zlib by hand."""
  from se3ds_amd.trainers import gan_manager
  rng = np.random.default_rng(4)
  for shape in ((5, 7, 3), (4, 6, 1), (1, 1, 3)):
    px = rng.integers(0, 256, shape).astype(np.uint8)
    data = gan_manager._encode_png(px)
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR'
    np.testing.assert_array_equal(ref.decode_png(data), px)
  # the IDAT payload is a plain zlib stream of filter-0 rows
  px = rng.integers(0, 256, (2, 3, 1)).astype(np.uint8)
  data = gan_manager._encode_png(px)
  at = data.index(b'IDAT')
  length = int.from_bytes(data[at - 4:at], 'big')
  rows = zlib.decompress(data[at + 4:at + 4 + length])
  assert rows == b'\x00' + px[0].tobytes() + b'\x00' + px[1].tobytes()
  with pytest.raises(ValueError):
    gan_manager._encode_png(np.zeros((2, 2, 2), np.uint8))
  # float -> uint8 as tf.image.convert_image_dtype does: x * 255.5, saturated, truncated
  x = torch.tensor([-0.1, 0.0, 0.5, 0.999, 1.0, 1.3])
  assert gan_manager._to_uint8(x).tolist() == [0, 0, 127, 255, 255, 255]


def test_checkpoint_bookkeeping(tmp_path, monkeypatch):
  """The host side of GANManager.test: which checkpoints still lack a row (whether model_dir is
  given relative or absolute), the step of a checkpoint name, and a score file of other columns."""
  import csv
  from se3ds_amd.trainers import se3ds_trainer

  class Strategy:
    num_replicas_in_sync = 1
    group = None
    device = 'cpu'
  gin_lite.clear_config()
  (tmp_path / 'run').mkdir()
  monkeypatch.chdir(tmp_path)
  for name in ('ckpt-30.npz', 'ckpt-4.npz', 'ckpt-200.npz', 'ckpt-x.npz', 'other-7.npz'):
    (tmp_path / 'run' / name).write_bytes(b'')
  make = lambda model_dir: se3ds_trainer.GAN(1.0, 1.0, 1.0, 1.0, strategy=Strategy(),
                                             model_dir=model_dir, seed=0, eval_seq_len=2)
  rel, absolute = make('run'), make(str(tmp_path / 'run'))
  assert rel._unevaluated_checkpoints() == [os.path.join('run', f'ckpt-{s}.npz') for s in (4, 30, 200)]
  result = {'val_seen/eval_image/fid@1': 1.0}
  row = rel._add_eval_result(os.path.join('run', 'ckpt-30.npz'), 30, result)
  assert row == {'checkpoint_path': os.path.join('run', 'ckpt-30.npz'), 'step': '30',
                 'val_seen/eval_image/fid@1': '1.000'}
  # the row was written under the relative name; the absolute spelling of the directory sees it
  assert absolute._unevaluated_checkpoints() == [str(tmp_path / 'run' / f'ckpt-{s}.npz') for s in (4, 200)]
  assert rel._unevaluated_checkpoints() == [os.path.join('run', f'ckpt-{s}.npz') for s in (4, 200)]
  # another set of columns (e.g. another eval_seq_len) is an error, not a silently ragged file
  with pytest.raises(ValueError, match='columns'):
    rel._add_eval_result(os.path.join('run', 'ckpt-4.npz'), 4, {'val_seen/eval_image/fid@2': 1.0})
  with open(tmp_path / 'run' / 'scores_val_seen.csv', newline='') as f:
    assert len(list(csv.DictReader(f))) == 1
  step = se3ds_trainer.GAN._checkpoint_step
  assert step('test-1') == 1 and step('a/b/ckpt-2000.npz') == 2000 and step('ema-run-12') == 12
  for bad in ('final.npz', 'ckpt-.npz', 'ckpt-12.npy', 'ckpt'):
    with pytest.raises(ValueError, match='step'):
      step(bad)
  # a bad name is refused before the dataset or the evaluator are built
  with pytest.raises(ValueError, match='step'):
    rel.test(eval_examples=[{}], checkpoints=['final.npz'])


# ----------------------------------------------------------------------------------------- GPU
def _raw(n, t, h0, seed, pathdreamer=True):
  ex = ref.synth_examples(n, t, h0, seed, pathdreamer=pathdreamer, lo=-0.2, hi=1.2)
  return {k: np.stack([e[k] for e in ex]) for k in ex[0]}


def _upload(raw):
  return {k: torch.from_numpy(v).to(DEV) for k, v in raw.items()}


def _band_params(size):
  """mode 0, a wrapped band and an unwrapped band on the output grid of width 2 * size."""
  w = 2 * size
  return [dict(hmask=None), dict(hmask=(2, 0.7 * w + 0.25, 0.2 * w)),
          dict(hmask=(1, 0.125 * w, 0.8 * w + 0.5))]


def _assert_same(got, want, keys):
  assert sorted(got) == sorted(keys)
  for k in keys:
    g = got[k].cpu().numpy()
    assert g.dtype == want[k].dtype, (k, g.dtype, want[k].dtype)
    assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
    np.testing.assert_array_equal(g, want[k], err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize('pathdreamer', [True, False])
@pytest.mark.parametrize('h0,size', [(64, 32), (128, 128), (96, 64), (64, 8)])
def test_device_transform_matches_restatement(h0, size, pathdreamer):
  """G1: 2x, identity, 1.5x and 8x, with and without the pathdreamer planes, bit for bit."""
  n, t = 3, 4
  raw = _raw(n, t, h0, seed=h0 + size, pathdreamer=pathdreamer)
  ds = indoor_datasets.R2RVideoDataset(image_size=size, horizontal_mask_ratio=0.25)
  keys = [k for k in OUT_KEYS if pathdreamer or not k.startswith('pathdreamer_')]
  for params in (_band_params(size), [dict(hmask=None)] * n):
    got = ds.device_transform(_upload(raw), params)
    want = ref.video_transform(raw, params, size)
    _assert_same(got, want, keys)
    assert got['image'].shape == (n, t, size, 2 * size, 3)
    assert got['segmentation'].shape == (n, t, size, 2 * size, 1)
    assert got['position'].shape == (n, t, 3) and got['position'].is_contiguous()


def _op_by_op(rawd, params, size):
  """The same outputs from the operators that were there before: pano_utils.resize per field and a
  torch multiply for the mask."""
  from se3ds_amd.utils import pano_utils
  n, t, h0, w0, _ = rawd['image'].shape
  h, w = size, 2 * size
  out = {}
  out['original_image'] = pano_utils.resize(rawd['image'].reshape(n * t, h0, w0, 3), h, w,
                                            'bilinear').reshape(n, t, h, w, 3)
  mask = torch.from_numpy(np.stack([ref.band_mask(w, p.get('hmask')) for p in params])).to(DEV)
  out['image'] = out['original_image'] * mask[:, None, None, :, None]
  for k in ref.PLANES:
    out[k] = pano_utils.resize(rawd[k][..., None].contiguous().reshape(n * t, h0, w0, 1), h, w,
                               'nearest').reshape(n, t, h, w, 1)
  return out


@pytest.mark.gpu
@pytest.mark.parametrize('h0,size', [(64, 32), (128, 128), (96, 64), (64, 8)])
def test_device_transform_matches_op_by_op_chain(h0, size):
  """G2: ties the new kernel to se3ds_resize."""
  raw = _raw(3, 4, h0, seed=7 * h0 + size)
  rawd = _upload(raw)
  params = _band_params(size)
  got = indoor_datasets.R2RVideoDataset(image_size=size).device_transform(rawd, params)
  want = _op_by_op(rawd, params, size)
  for k in want:
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    assert torch.equal(got[k], want[k]), k


@pytest.mark.gpu
def test_image_shares_the_buffer_without_a_mask():
  """G3: ratio 0 -> one buffer under both keys; ratio > 0 -> two, and original_image is what the
  unmasked run returns as image."""
  raw = _upload(_raw(2, 3, 32, seed=11))
  rng = np.random.default_rng(0)
  plain = indoor_datasets.R2RVideoDataset(image_size=16).transform(raw, rng)
  assert plain['image'].data_ptr() == plain['original_image'].data_ptr()
  masked = indoor_datasets.R2RVideoDataset(image_size=16, horizontal_mask_ratio=0.5).transform(raw, rng)
  assert masked['image'].data_ptr() != masked['original_image'].data_ptr()
  assert torch.equal(masked['original_image'], plain['image'])
  assert not torch.equal(masked['image'], plain['image'])
  zero_cols = (masked['image'] == 0).all(dim=4).all(dim=2).all(dim=1)   # (N, w)
  assert (zero_cols.sum(dim=1) >= 15).all() and (zero_cols.sum(dim=1) <= 17).all()


@pytest.mark.gpu
def test_device_transform_rejects_bad_arguments():
  """G4."""
  ds = indoor_datasets.R2RVideoDataset(image_size=8)
  raw = _upload(_raw(2, 3, 16, seed=12))
  params = [dict(hmask=None)] * 2
  ds.device_transform(raw, params)
  with pytest.raises(ValueError, match='segmentation'):
    ds.device_transform(dict(raw, segmentation=raw['segmentation'].to(torch.int32)), params)
  with pytest.raises(ValueError, match='image'):
    ds.device_transform(dict(raw, image=raw['image'].to(torch.float64)), params)
  with pytest.raises(ValueError, match='parameter rows'):
    ds.device_transform(raw, params[:1])
  with pytest.raises(ValueError, match='depth'):
    ds.device_transform(dict(raw, depth=raw['depth'][:, :2].contiguous()), params)
  with pytest.raises(ValueError, match='position'):
    ds.device_transform(dict(raw, position=raw['position'][:, :2].contiguous()), params)
  with pytest.raises(ValueError, match='hmask mode'):
    ds.device_transform(raw, [dict(hmask=None), dict(hmask=(3, 1.0, 2.0))])


def test_video_transform_abi_rejects_bad_shapes():
  """Non-positive sizes, a pathdreamer input without its output and a masked output without band rows
  are SE3DS_E_BADSHAPE before anything is launched (no device needed: the pointers are never read)."""
  import ctypes
  from se3ds_amd import _lib
  L = _lib.lib()
  buf = ctypes.create_string_buffer(256)
  p = ctypes.addressof(buf)
  args = lambda **kw: [p, p, kw.get('pd', None), p, None, None, None, kw.get('n', 1), kw.get('t', 1),
                       2, 2, kw.get('h', 1), 1, p, kw.get('masked', None), p, None, p, None, None]
  assert L.se3ds_video_transform(*args(n=0)) == -1
  assert L.se3ds_video_transform(*args(t=0)) == -1
  assert L.se3ds_video_transform(*args(h=-3)) == -1
  assert L.se3ds_video_transform(*args(pd=p)) == -1
  assert L.se3ds_video_transform(*args(masked=p)) == -1


@pytest.mark.gpu
def test_shipped_size_against_restatement():
  """G5: N = 1, T = 8, 1024x2048 -> 512x1024 (the 201 MB input needs 64-bit element offsets)."""
  rng = np.random.default_rng(13)
  t, h0, size = 8, 1024, 512
  raw = dict(
      image=rng.random((1, t, h0, 2 * h0, 3), dtype=F32),
      segmentation=rng.integers(0, 42, (1, t, h0, 2 * h0), dtype=np.uint8),
      depth=rng.random((1, t, h0, 2 * h0), dtype=F32),
      position=rng.random((1, t, 4), dtype=F32))
  params = [dict(hmask=(2, 900.5, 130.0))]
  got = indoor_datasets.R2RVideoDataset(image_size=size).device_transform(_upload(raw), params)
  want = ref.video_transform(raw, params, size)
  _assert_same(got, want, ['image', 'original_image', 'segmentation', 'depth', 'position',
                           'position_xyz1'])


def _eval_run(mask_ratio):
  from se3ds_amd.models import image_models
  from se3ds_amd.utils import eval_metric
  from se3ds_amd.utils import inception_utils as iu
  gin_lite.clear_config()
  size, t, n = 64, 3, 4
  G = image_models.ResNetGenerator(image_size=size, gen_dims=8, z_dim=4, resnet_version='50',
                                   device=DEV, seed=3, dtype=torch.float32)
  examples = ref.synth_examples(6, t, 2 * size, seed=21)
  ds = indoor_datasets.R2RVideoDataset(image_size=size, video_length=t,
                                       horizontal_mask_ratio=mask_ratio)
  inception = iu.inception_model(init='random', seed=12, device=DEV)
  em = eval_metric.EvalMetric(ds.input_fn(examples, n, seed=5, device=DEV), eval_num=8,
                              batch_size=n, avg_num=1, eval_seq_len=t, inception=inception, seed=9,
                              keep_pools=True)
  fid, _, rmse = em.calculate_fid_score(G)
  return em, fid, rmse


@pytest.mark.gpu
def test_input_fn_feeds_eval_metric():
  """G6: input_fn -> EvalMetric -> calculate_fid_score; with a mask on, the real statistics still
  come from original_image while the roll-out starts from the masked frames."""
  t = 3
  em0, fid0, rmse0 = _eval_run(0.0)
  em1, fid1, rmse1 = _eval_run(0.25)
  for fid, rmse in ((fid0, rmse0), (fid1, rmse1)):
    assert sorted(fid) == sorted(rmse) == list(range(1, t))
    for i in fid:
      assert np.isfinite(fid[i]) and np.isfinite(rmse[i]), i
  for i in range(1, t):
    assert em0.real_pools[i].shape == (8, 2048)
    np.testing.assert_array_equal(em1.real_pools[i], em0.real_pools[i])
    assert not np.array_equal(em1.generated_pools[i], em0.generated_pools[i])
