"""GAN training manager -- MI355X implementation of the hot-path half of the reference's
trainers/gan_manager.py: model / optimizer construction (:169-183), the cluster step
(:351-385), the EMA hooks (:642-655) and checkpoint save / restore as one .npz.  TFRecord
parsing, TensorFlow checkpoint objects and TensorBoard logging are out of scope (SURVEY.md section
2.1); `train()` runs the same host loop on a synthetic (or user supplied) batch iterator, `test()`
the reference's evaluation loop (:233-322) over parsed trajectory examples: R2RVideoDataset ->
EvalMetric -> one scores_<split>.csv row per checkpoint."""
import abc
import csv
import os
import random
import re
import struct
import zlib
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from se3ds_amd import _lib
from se3ds_amd import gin_lite as gin
from se3ds_amd import hipops  # noqa: F401
from se3ds_amd.trainers import dist_utils
from se3ds_amd.utils import ema


class OneDeviceStrategy:
  """Stands in for tf.distribute.OneDeviceStrategy (reference main.py:55-60)."""
  num_replicas_in_sync = 1
  group = None

  def __init__(self, device='cuda:0'):
    self.device = torch.device(device)


class DataParallelStrategy:
  """One process per GPU over RCCL (torch.distributed 'nccl'); stands in for
  tf.distribute.MirroredStrategy (reference main.py:63)."""

  def __init__(self, device, group=None):
    self.device = torch.device(device)
    self.group = group
    self.num_replicas_in_sync = dist.get_world_size(group)


class AdamState:
  """Keras Adam slots over a model's flat trainable arena (reference :175-183)."""

  def __init__(self, model, lr, beta_1, beta_2, epsilon=1e-7):
    self.model = model
    self.lr, self.beta_1, self.beta_2, self.epsilon = lr, beta_1, beta_2, epsilon
    self.m = torch.zeros_like(model.store.theta)
    self.v = torch.zeros_like(model.store.theta)
    self.iterations = 0
    self.chunks, self.tensor_chunk_start = model.store.chunk_tables()
    self._tcs_host = self.tensor_chunk_start.cpu().tolist()
    dev = model.store.theta.device
    self.partial = torch.empty(self.chunks.shape[0], dtype=torch.float32, device=dev)
    self.sqnorm = torch.empty(len(model.store.trainable_names), dtype=torch.float32, device=dev)
    self.mean_norm = torch.zeros(1, dtype=torch.float32, device=dev)
    self.on_update = None   # tests: f(e0, e1), called right before Adam consumes grad[e0:e1]

  def _sn_ptr(self, fused_sn):
    """fused_sn: the model's spectral layers only ran SpectralGroup.backward_fixup(dots_only=True);
    their fix-up is folded into this clip pass."""
    if not fused_sn:
      return None
    sn = self.model.spectral.tensor_sn(self.model.store)
    return sn.data_ptr() if sn is not None else None

  def clip_gradients(self, clip_norm=5.0, fused_sn=False):
    """Per-tensor tf.clip_by_norm, in place on the gradient arena (se3ds_trainer.py:27-32)."""
    st = self.model.store
    L = _lib.lib()
    nt = len(st.trainable_names)
    sn = self._sn_ptr(fused_sn)
    _lib.check(L.se3ds_multi_sqnorm_sn(st.grad.data_ptr(), self.chunks.data_ptr(),
                                       self.chunks.shape[0], self.tensor_chunk_start.data_ptr(), nt,
                                       self.partial.data_ptr(), self.sqnorm.data_ptr(), sn, 0,
                                       _lib.stream()), 'se3ds_multi_sqnorm_sn')
    _lib.check(L.se3ds_multi_clip_by_norm_sn(st.grad.data_ptr(), self.chunks.data_ptr(),
                                             self.chunks.shape[0], self.sqnorm.data_ptr(), nt,
                                             float(clip_norm), self.mean_norm.data_ptr(), sn,
                                             _lib.stream()), 'se3ds_multi_clip_by_norm_sn')
    return self.mean_norm

  def clip_segment(self, t0, t1, clip_norm=5.0, fused_sn=False):
    """clip_gradients restricted to tensors [t0, t1) (per-segment gradient synchronisation)."""
    st = self.model.store
    L = _lib.lib()
    sn = self._sn_ptr(fused_sn)
    c0, c1 = self._tcs_host[t0], self._tcs_host[t1]
    if c1 <= c0:
      return
    cache = self.__dict__.setdefault('_seg_tcs', {})
    if (t0, t1) not in cache:   # chunk prefix of the segment, relative to its first chunk
      cache[(t0, t1)] = (self.tensor_chunk_start[t0:t1 + 1] - c0).contiguous()
    tcs = cache[(t0, t1)]
    _lib.check(L.se3ds_multi_sqnorm_sn(st.grad.data_ptr(), self.chunks.data_ptr() + 24 * c0, c1 - c0,
                                       tcs.data_ptr(), t1 - t0, self.partial.data_ptr(),
                                       self.sqnorm.data_ptr() + 4 * t0, sn, t0, _lib.stream()),
               'se3ds_multi_sqnorm_sn')
    # chunk rows carry absolute tensor ids: sqnorm is passed from its base
    _lib.check(L.se3ds_multi_clip_by_norm_sn(st.grad.data_ptr(), self.chunks.data_ptr() + 24 * c0,
                                             c1 - c0, self.sqnorm.data_ptr(), t1 - t0,
                                             float(clip_norm), None, sn, _lib.stream()),
               'se3ds_multi_clip_by_norm_sn')

  def clip_apply(self, t0, t1, clip_norm=5.0, fused_sn=False, ema_theta=None, one_minus_decay=0.0):
    """One replica: clip_segment(t0, t1) + apply_segment over the same tensors in ONE pass over the
    gradient arena (se3ds_multi_clip_adam_keras_ema): the clipped gradient only ever exists in
    registers.  Bit-identical to the two calls.  Returns False (nothing done) when a test hook
    wants to see the clipped arena (on_update) -- the caller then takes the separate passes.
    Call begin_step() first, end_step() last, as for apply_segment."""
    if self.on_update is not None:
      return False
    st = self.model.store
    L = _lib.lib()
    sn = self._sn_ptr(fused_sn)
    c0, c1 = self._tcs_host[t0], self._tcs_host[t1]
    if c1 <= c0:
      return True
    cache = self.__dict__.setdefault('_seg_tcs', {})
    if (t0, t1) not in cache:
      cache[(t0, t1)] = (self.tensor_chunk_start[t0:t1 + 1] - c0).contiguous()
    tcs = cache[(t0, t1)]
    _lib.check(L.se3ds_multi_sqnorm_sn(st.grad.data_ptr(), self.chunks.data_ptr() + 24 * c0, c1 - c0,
                                       tcs.data_ptr(), t1 - t0, self.partial.data_ptr(),
                                       self.sqnorm.data_ptr() + 4 * t0, sn, t0, _lib.stream()),
               'se3ds_multi_sqnorm_sn')
    _lib.check(L.se3ds_multi_clip_adam_keras_ema(
        st.theta.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
        self.chunks.data_ptr() + 24 * c0, c1 - c0, self.sqnorm.data_ptr(), float(clip_norm), sn,
        self.lr, self.beta_1, self.beta_2, self.epsilon, self.iterations, _lib.ptr(ema_theta),
        float(one_minus_decay), _lib.stream()), 'se3ds_multi_clip_adam_keras_ema')
    return True

  def mean_clipped_norm(self, clip_norm=5.0):
    _lib.check(_lib.lib().se3ds_mean_clipped_norm(
        self.sqnorm.data_ptr(), len(self.model.store.trainable_names), float(clip_norm),
        self.mean_norm.data_ptr(), _lib.stream()), 'se3ds_mean_clipped_norm')
    return self.mean_norm

  def begin_step(self):
    """Per-segment updates (apply_segment): the Adam step counter advances once per step."""
    self.iterations += 1

  def apply_segment(self, e0, e1, ema_theta=None, one_minus_decay=0.0):
    """The Keras Adam update (+ the EMA of the same variables) on elements [e0, e1) of the arena:
    a module is updated as soon as the backward pass has left it (se3ds_trainer.train_g_d), on a
    side stream, while the rest of the backward pass still runs.  Element-wise, so the result is
    bit-identical to one pass over the whole arena.  Call begin_step() first, end_step() last."""
    st = self.model.store
    if e1 <= e0:
      return
    if self.on_update is not None:
      self.on_update(e0, e1)
    _lib.check(_lib.lib().se3ds_multi_adam_keras_ema(
        st.theta.data_ptr() + 4 * e0, st.grad.data_ptr() + 4 * e0, self.m.data_ptr() + 4 * e0,
        self.v.data_ptr() + 4 * e0, e1 - e0, self.lr, self.beta_1, self.beta_2, self.epsilon,
        self.iterations, (ema_theta.data_ptr() + 4 * e0) if ema_theta is not None else None,
        float(one_minus_decay), _lib.stream()), 'se3ds_multi_adam_keras_ema')

  def end_step(self):
    self.model.store.version += 1

  def apply_gradients(self, group=None, world=1, ema_theta=None, one_minus_decay=0.0):
    """Cross-replica SUM of the (already clipped, already 1/R-scaled) gradients, then the
    Keras Adam update (reference se3ds_trainer.py:253-257).  With `ema_theta` (the EMA model's
    trainable arena) the moving average of these variables is advanced in the same pass."""
    st = self.model.store
    if world > 1:
      dist_utils.allreduce_arena_sum(st.grad, group)
    if self.on_update is not None:
      self.on_update(0, st.theta.numel())
    self.iterations += 1
    _lib.check(_lib.lib().se3ds_multi_adam_keras_ema(
        st.theta.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
        st.theta.numel(), self.lr, self.beta_1, self.beta_2, self.epsilon, self.iterations,
        _lib.ptr(ema_theta), float(one_minus_decay), _lib.stream()), 'se3ds_multi_adam_keras_ema')
    st.version += 1


class Mean:
  """tf.keras.metrics.Mean over device scalars; values are read lazily (no sync per step)."""

  def __init__(self, name):
    self.name = name
    self._vals = []

  def update_state(self, v):
    self._vals.append(v)

  def reset_states(self):
    self._vals = []

  def result(self):
    if not self._vals:
      return np.float32(0.0)
    tot = 0.0
    for v in self._vals:
      if callable(v):
        v = v()
      if isinstance(v, torch.Tensor):
        v = float(v.detach().float().mean().cpu())
      tot += float(v)
    return np.float32(tot / len(self._vals))


def _encode_png(pixels: np.ndarray) -> bytes:
  """8-bit PNG of a uint8 (H,W,1) grey or (H,W,3) RGB array: one IDAT chunk, filter 0 on every
  row (zlib + struct only; no imaging package is assumed)."""
  if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] not in (1, 3):
    raise ValueError(f'uint8 (H,W,1) or (H,W,3) expected, got {pixels.dtype} {pixels.shape}')
  h, w, c = pixels.shape
  rows = np.concatenate([np.zeros((h, 1), np.uint8), pixels.reshape(h, w * c)], axis=1)

  def chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data))

  ihdr = struct.pack('>IIBBBBB', w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
  return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr) +
          chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


def _to_uint8(x: torch.Tensor) -> np.ndarray:
  """tf.image.convert_image_dtype(float -> uint8) on the host: x * 255.5, saturated, truncated."""
  return np.clip(x.detach().float().cpu().numpy() * np.float32(255.5), 0, 255).astype(np.uint8)


@gin.configurable(denylist=['strategy', 'model_dir'])
class GANManager(abc.ABC):
  """Constructor surface of the reference (:98-167)."""

  # 'host' | 'device': who encodes the roll-out PNGs of test() -- zlib on the host, frame by frame,
  # or utils/png.encode_png_batch, all frames of a checkpoint in one batch
  png_encoder = 'host'

  def __init__(self, strategy, model_dir: str = '', image_size: int = 128, seed: int = 1,
               optimizer_type: str = 'adam', beta1: float = 0.0, beta2: float = 0.999,
               g_lr: float = 0.0002, d_lr: float = 0.0002, train_batch_size: int = 128,
               test_batch_size: int = 128, parallel_calls: int = -1, log_every_steps: int = 1000,
               save_every_steps: int = 2000, eval_every_steps: int = 2000, num_epochs: int = 100,
               d_step_per_g_step: int = 1, num_batched_steps: int = 5, show_num: int = 16,
               shuffle_buffer_size: int = 1000, ema_decay: float = 0.999, ema_init_step: int = 0,
               generator_fn=None, discriminator_fn=None, train_dataset_glob: Optional[str] = None,
               test_dataset_glob: Optional[str] = None, eval_size: Optional[int] = 10000,
               test_split: str = 'val_seen', eval_seq_len: int = 4, predict_depth: bool = False,
               compute_dtype=torch.float32):
    self.strategy = strategy
    self.model_dir = model_dir
    self.image_size = image_size
    self.seed = seed
    self.optimizer_type = optimizer_type
    self.beta1, self.beta2 = beta1, beta2
    self.g_lr, self.d_lr = g_lr, d_lr
    self.global_batch_size = train_batch_size
    self.train_batch_size = train_batch_size
    self.test_batch_size = test_batch_size
    self.parallel_calls = parallel_calls
    self.log_every_steps = log_every_steps
    self.save_every_steps = save_every_steps
    self.eval_every_steps = eval_every_steps
    self.num_epochs = num_epochs
    self.d_step_per_g_step = d_step_per_g_step
    self.num_batched_steps = num_batched_steps
    self.show_num = show_num
    self.shuffle_buffer_size = shuffle_buffer_size
    self.ema_decay = ema_decay
    self.ema_init_step = ema_init_step
    self.generator_fn = generator_fn
    self.discriminator_fn = discriminator_fn
    self.train_dataset_glob = train_dataset_glob
    self.test_dataset_glob = test_dataset_glob
    self.eval_size = eval_size
    self.test_split = test_split
    self.eval_seq_len = eval_seq_len
    self.predict_depth = predict_depth
    self.compute_dtype = compute_dtype
    self.global_step = 0
    self.train_ds = None
    if seed > 0:   # reference :164-167 (the shipped configs set seed = 0: nothing is seeded)
      random.seed(seed)
      np.random.seed(seed)
      torch.manual_seed(seed)

  # ----------------------------------------------------------------------------- building
  def _build_model(self):
    """Creates Generator, Discriminator and EMA Generator (reference :169-173)."""
    dev = self.strategy.device
    kw = dict(device=dev, dtype=self.compute_dtype)
    sgn = -1 if getattr(self, 'device_init', False) else 1   # negative seed: on-device init
    self.generator = self.generator_fn(image_size=self.image_size,
                                       seed=sgn * (1000 + max(self.seed, 0)), **kw)
    self.discriminator = self.discriminator_fn(image_size=self.image_size,
                                               seed=sgn * (2000 + max(self.seed, 0)), **kw)
    self.ema_generator = self.generator_fn(image_size=self.image_size,
                                           seed=sgn * (3000 + max(self.seed, 0)), **kw)

  def _build_optimizer(self):
    """Creates optimizers for both Generator and Discriminator (reference :175-183)."""
    if self.optimizer_type == 'adam':
      self.g_optimizer = AdamState(self.generator, self.g_lr, self.beta1, self.beta2)
      self.d_optimizer = AdamState(self.discriminator, self.d_lr, self.beta1, self.beta2)
    else:
      raise NotImplementedError

  def _create_metrics(self):
    self.metrics = {'gen_loss': Mean('gen_loss'), 'disc_loss': Mean('disc_loss')}

  def _create_obj(self):
    """reference :333-349 without the checkpoint objects."""
    self.global_step = 0
    self._build_model()
    self._build_optimizer()
    self._create_metrics()

  def _split_input_dict(self, input_dict, splits):
    """Splits a batch dict along axis 0 into `splits` dicts (reference :351-364)."""
    output = [dict() for _ in range(splits)]
    for key, item in input_dict.items():
      n = item.shape[0]
      if n % splits != 0:
        raise ValueError(f'batch {n} of {key} is not divisible by {splits}')
      for i, part in enumerate(torch.split(item, n // splits)):
        output[i][key] = part
    return output

  @abc.abstractmethod
  def train_d(self, inputs):
    """Learns the Discriminator updates."""

  @abc.abstractmethod
  def train_g_d(self, inputs):
    """Learns both the Generator and Discriminator updates."""

  def train_cluster(self, steps=1):
    """`steps` cluster steps: d_step_per_g_step-1 train_d calls then one train_g_d, each on
    its own chunk of the cluster batch (reference :376-385)."""
    for _ in range(int(steps)):
      inputs = next(self.train_ds)
      input_list = self._split_input_dict(inputs, self.d_step_per_g_step)
      for i in range(self.d_step_per_g_step - 1):
        self.train_d(input_list[i])
      self.train_g_d(input_list[-1])

  def train(self, train_ds=None, num_train_steps=None, logger=None, display_batch=None, checkpoints=None,
            resume=False, max_to_keep=200, snapshot='device', staging_bytes=2 * (256 << 20)):
    """Host loop of the reference (:387-423).  logger: a utils/logger.UniversalLogger; the metrics
    go to it as scalars at every log_every_steps.  With a display_batch as well (a trajectory batch,
    what _get_image_grid takes) the nine image grids of its roll-out go out under the prefix 'train'
    where the reference saves a checkpoint and logs them (:415-420).  Without a logger nothing of
    that is written.

    checkpoints: None (the default: no file is written), 'sync' (save_checkpoint) or 'async'
    (save_checkpoint_async with `snapshot` and `staging_bytes`).  model_dir/ckpt-<step>.npz is saved
    where the reference calls ckpt_manager.save(step) -- step > num_batched_steps and
    step % save_every_steps < num_batched_steps, before the image grids -- and
    ckpt-<num_train_steps>.npz after the loop (:417,422); then the writer is waited for, and a
    failure of it is raised.  After a file is in place the oldest ckpt-*.npz beyond max_to_keep
    (the reference keeps 200, :348-349) are deleted.
    resume: restore the highest-step ckpt-<step>.npz of model_dir, if any, before the first step
    (:327-331); its path is left in self.restored_from (None: started from initialisation).
    The global_step in a file is its value at the moment of the save, which the loop, like the
    reference's, advances only afterwards: a resumed run repeats that loop index with the optimiser
    iterations already advanced, as the reference does."""
    if checkpoints not in (None, 'sync', 'async'):
      raise ValueError(f"checkpoints: None, 'sync' or 'async', got {checkpoints!r}")
    self.global_batch_size = self.train_batch_size
    if not hasattr(self, 'generator'):
      self._create_obj()
    if resume:
      found = self._checkpoint_files()
      self.restored_from = found[-1][1] if found else None
      if found:
        self.restore_checkpoint(self.restored_from)
    if train_ds is not None:
      self.train_ds = iter(train_ds)
    if self.train_ds is None:
      raise ValueError('no training data: pass train_ds (an iterator of batch dicts)')
    if num_train_steps is None:
      num_train_steps = 1 if self.num_epochs == -1 else self.num_batched_steps
    for step in range(self.global_step, num_train_steps, self.num_batched_steps):
      self.train_cluster(self.num_batched_steps)
      if step % self.log_every_steps < self.num_batched_steps:
        result_dict = self._save_metrics_to_dict()
        if logger is not None:
          logger.log_scalars(step, **result_dict)
        self._reset_metrics()
      if checkpoints is not None and step > self.num_batched_steps and (
          step % self.save_every_steps < self.num_batched_steps):
        self._train_save(step, checkpoints, max_to_keep, snapshot, staging_bytes)
      if logger is not None and display_batch is not None and step > self.num_batched_steps and (
          step % self.save_every_steps < self.num_batched_steps):
        image_dict, _ = self._get_image_dict(self._get_image_grid(display_batch), display_batch,
                                             'train')
        logger.log_images(step, **image_dict)
      self.global_step += self.num_batched_steps
    if checkpoints is not None:
      self._train_save(num_train_steps, checkpoints, max_to_keep, snapshot, staging_bytes)
      self.wait_for_checkpoint()

  def _checkpoint_files(self):
    """[(step, path)] of the ckpt-<step>.npz files of model_dir, in step order."""
    found = []
    for name in os.listdir(self.model_dir) if os.path.isdir(self.model_dir) else []:
      m = re.fullmatch(r'ckpt-(\d+)\.npz', name)
      if m:
        found.append((int(m.group(1)), os.path.join(self.model_dir, name)))
    return sorted(found)

  def _prune_checkpoints(self, max_to_keep):
    found = self._checkpoint_files()
    for _, path in found[:max(len(found) - int(max_to_keep), 0)]:
      os.remove(path)

  def _writes_checkpoints(self):
    """One replica, or rank 0 of the strategy's group: the replicas hold the same state."""
    return self.strategy.num_replicas_in_sync == 1 or dist.get_rank(self.strategy.group) == 0

  def _train_save(self, step, mode, max_to_keep, snapshot, staging_bytes):
    path = os.path.join(self.model_dir, f'ckpt-{step}.npz')
    if mode == 'async':
      self.save_checkpoint_async(path, snapshot=snapshot, staging_bytes=staging_bytes,
                                 after=lambda: self._prune_checkpoints(max_to_keep))
    elif self._writes_checkpoints():
      self.save_checkpoint(path)
      self._prune_checkpoints(max_to_keep)

  def _reset_metrics(self):
    for key in self.metrics:
      self.metrics[key].reset_states()

  def _save_metrics_to_dict(self):
    output_dict = {}
    for key, value in self.metrics.items():
      r = value.result()
      if np.any(np.isnan(r)):
        raise ValueError(f'NaN losses recorded for {key}.')
      output_dict[key] = r
    return output_dict

  # ----------------------------------------------------------------------- evaluation loop
  def _get_image_grid(self, inputs, modes=('normal', 'ema')):
    """Video branch of the reference's `_get_image_grid` (:458-541): for the training and the EMA
    generator, roll a trajectory out autoregressively -- project the memory, generate, feed the
    frame back (utils/eval_metric.generated_rollout; unprojection with void_class 0 as :536-539
    does).  inputs: image (N,T,H,W,3), depth (N,T,H,W,1), position (N,T,3), depth_scale (N,).
    Returns {mode: RolloutOutput}; _get_image_dict composes the TensorBoard grids from it."""
    from se3ds_amd.utils import eval_metric
    res = {}
    for mode in modes:
      gen = self.ema_generator if mode == 'ema' else self.generator
      res[mode] = eval_metric.generated_rollout(gen, inputs, self.eval_seq_len,
                                                predict_depth=self.predict_depth,
                                                unproject_void_class=0)
    return res

  def _get_image_dict(self, rollouts, inputs, name_prefix):
    """The second half of the reference's `_get_image_grid` (:558-617): the nine image grids of a
    roll-out -- rollouts = _get_image_grid(inputs), both modes -- as {name_prefix_<family>: uint8
    (1, ny*H, nx*W, 3) device tensor}, and output_dict as :611-616.  Frames are concatenated along
    the batch in frame order; depth and masks fill three channels."""
    from se3ds_amd.utils import image_grid
    normal, ema = rollouts['normal'], rollouts['ema']
    frames = range(self.eval_seq_len)

    def cat(tensors):
      return torch.cat([t if t.dtype in (torch.float32, torch.bfloat16) else t.float()
                        for t in tensors], dim=0)

    pred_depth, ema_pred_depth = cat(normal.pred_depth), cat(ema.pred_depth)
    families = [
        ('_raw_generated', cat(normal.generated)),
        ('_ema_generated', cat(ema.generated)),
        ('_pred_depth', pred_depth),
        ('_ema_pred_depth', ema_pred_depth),
        ('_real_img', cat([inputs['image'][:, k] for k in frames])),
        ('_real_depth', cat([inputs['depth'][:, k] for k in frames])),
        ('_projected', cat(normal.projected)),
        ('_blur_bbox', torch.zeros_like(pred_depth)),   # the video branch feeds zeros (:494)
        ('_proj_mask', cat(normal.proj_mask)),
    ]
    image_dict = {}
    for suffix, x in families:
      image_dict.update(image_grid.get_grid_image_dict(x, self.show_num, self.strategy,
                                                       name_prefix + suffix, out_c=3))
    output_dict = {'ema_generated_image': cat(ema.generated),
                   'ema_pred_depth': ema_pred_depth.expand(-1, -1, -1, 3)}
    return image_dict, output_dict

  def _score_file(self):
    return os.path.join(self.model_dir, f'scores_{self.test_split}.csv')

  def _unevaluated_checkpoints(self):
    """Every ckpt-<step>.npz under model_dir without a row in the score file, in step order (the
    reference's task_manager.unevaluated_checkpoints, :80-141, without the polling and the wait)."""
    done = set()   # absolute: model_dir may be given relative in one run and absolute in the next
    if os.path.exists(self._score_file()):
      with open(self._score_file(), newline='') as f:
        done = {os.path.abspath(r['checkpoint_path']) for r in csv.DictReader(f)}
    found = []
    for name in os.listdir(self.model_dir):
      m = re.fullmatch(r'ckpt-(\d+)\.npz', name)
      path = os.path.join(self.model_dir, name)
      if m and os.path.abspath(path) not in done:
        found.append((int(m.group(1)), path))
    return [path for _, path in sorted(found)]

  @staticmethod
  def _checkpoint_step(checkpoint_path):
    """The number that ends a checkpoint's name ('ckpt-2000.npz', 'test-1'), as the reference's
    add_eval_result takes it (utils/task_manager.py:171)."""
    name = os.path.basename(checkpoint_path)
    m = re.fullmatch(r'.*-(\d+)(\.npz)?', name)
    if not m:
      raise ValueError(f"checkpoint name {name!r} does not end in '-<step>' or '-<step>.npz': "
                       'its row in the score file needs the step')
    return int(m.group(1))

  def _add_eval_result(self, checkpoint_path, step, result_dict):
    """One row of scores_<split>.csv (reference utils/task_manager.py:166-187): checkpoint_path,
    step, then the sorted result keys, floats as '{:.3f}'."""
    header = ['checkpoint_path', 'step'] + sorted(result_dict)
    row = dict(checkpoint_path=checkpoint_path, step=str(step))
    row.update({k: '{:.3f}'.format(float(v)) for k, v in result_dict.items()})
    new = not os.path.exists(self._score_file())
    if not new:
      with open(self._score_file(), newline='') as f:
        have = next(csv.reader(f), None)
      if have != header:   # e.g. another eval_seq_len: columns would be dropped or left blank
        raise ValueError(f'{self._score_file()} has the columns {have}, this run writes {header}')
    with open(self._score_file(), 'a', newline='') as f:
      writer = csv.DictWriter(f, fieldnames=header)
      if new:
        writer.writeheader()
      writer.writerow(row)
    return row

  @staticmethod
  def _rollout_videos(rollout):
    """The roll-out's frames as the PNGs hold them -- x * 255.5, truncated, saturated -- stacked over
    the frame index: (rgb, depth), uint8 device tensors (N,T,H,W,3) and (N,T,H,W,1)."""
    from se3ds_amd.models.models import _quantize
    return tuple(
        torch.stack([_quantize(f.detach().float(), torch.uint8, mul=255.5, div=1.0, lo=0.0, hi=255.0)
                     for f in frames], dim=1)
        for frames in (rollout.generated, rollout.pred_depth))

  def _save_rollout_images(self, rollout, step, video: bool = False, fps: float = 10):
    """images/<split>/<step>/<frame>/<example>_{rgb,depth}.png of the EMA roll-out (:274-296).
    video: also images/<split>/<step>/<example>_{rgb,depth}.gif, the same pixels as animated GIFs
    (depth lossless, rgb through an adaptive palette), all examples encoded in one batch on the
    device (utils/gif.encode_gif_batch)."""
    root = os.path.join(self.model_dir, 'images', self.test_split, str(step))
    if video:
      from se3ds_amd.utils import gif
      os.makedirs(root, exist_ok=True)
      paths, videos = [], []
      for suffix, stacked in zip(('rgb', 'depth'), self._rollout_videos(rollout)):
        for example_idx in range(stacked.shape[0]):
          paths.append(os.path.join(root, f'{example_idx}_{suffix}.gif'))
          videos.append(stacked[example_idx])
      for path, data in zip(paths, gif.encode_gif_batch(videos, fps=fps)):
        with open(path, 'wb') as f:
          f.write(data)
    if self.png_encoder not in ('host', 'device'):
      raise ValueError(f"png_encoder: 'host' or 'device', got {self.png_encoder!r}")
    if self.png_encoder == 'device':
      # the same pixels: _to_uint8's x * 255.5, truncated, saturated, as se3ds_quantize expresses it
      # (one fp32 product, the division by 1 exact); every frame of the checkpoint in one batch
      from se3ds_amd.models.models import _quantize
      from se3ds_amd.utils import png
      paths, images = [], []
      for suffix, frames in (('rgb', rollout.generated), ('depth', rollout.pred_depth)):
        for frame_idx, frame in enumerate(frames):
          frame_dir = os.path.join(root, str(frame_idx))
          os.makedirs(frame_dir, exist_ok=True)
          pixels = _quantize(frame.detach().float(), torch.uint8, mul=255.5, div=1.0, lo=0.0, hi=255.0)
          for example_idx in range(pixels.shape[0]):
            paths.append(os.path.join(frame_dir, f'{example_idx}_{suffix}.png'))
            images.append(pixels[example_idx])
      for path, data in zip(paths, png.encode_png_batch(images)):
        with open(path, 'wb') as f:
          f.write(data)
      return
    for suffix, frames in (('rgb', rollout.generated), ('depth', rollout.pred_depth)):
      for frame_idx, frame in enumerate(frames):
        frame_dir = os.path.join(root, str(frame_idx))
        os.makedirs(frame_dir, exist_ok=True)
        pixels = _to_uint8(frame)
        for example_idx in range(pixels.shape[0]):
          with open(os.path.join(frame_dir, f'{example_idx}_{suffix}.png'), 'wb') as f:
            f.write(_encode_png(pixels[example_idx]))

  def test(self, eval_examples=None, checkpoints=None, unit_test: bool = False, inception=None,
           logger=None, frechet: str = 'host', rollout_video: bool = False,
           image_metrics: bool = False):
    """The evaluation loop of the reference (:233-322) minus the polling task manager.  logger: a
    utils/logger.UniversalLogger; per checkpoint the row's values go to it as scalars and the nine
    image grids of the display batch's roll-out under the prefix test_split (:241,320-321).  eval_examples: parsed trajectory examples (what R2RVideoDataset.input_fn takes: a
    sequence of per-example dicts, or a callable returning a fresh iterator); TFRecord parsing
    stays outside.  checkpoints: .npz paths (save_checkpoint files); None: every ckpt-<step>.npz
    under model_dir that has no row in scores_<test_split>.csv yet, in step order.  unit_test:
    one pass over the randomly initialised model under the checkpoint name 'test-1'.

    Per checkpoint: restore, roll the display batch out (_get_image_grid), write the EMA
    roll-out's frames as PNG, FID / RMSE per frame index for the generator and its EMA, one CSV
    row.  The step of a row (and of its image directory) is the number that ends the checkpoint's
    name.  frechet: EvalMetric's Frechet method, 'host' or 'device'.  rollout_video: also write the
    EMA roll-out of every example as <example>_rgb.gif and <example>_depth.gif next to the frame
    directories and, with a logger, log the generated and the EMA roll-out as videos
    (<split>_raw_generated_video, <split>_ema_generated_video).  image_metrics: the row (and the
    logger's scalars) also get <split>/eval_image/{psnr,ema_psnr,ssim,ema_ssim}@<i>, the PSNR and SSIM
    of every generated frame against its ground-truth frame (EvalMetric.image_scores); a score file
    written without them has other columns and is refused.  Returns the rows written."""
    from se3ds_amd.datasets import indoor_datasets
    from se3ds_amd.utils import eval_metric
    if self.strategy.num_replicas_in_sync != 1:
      raise NotImplementedError('EvalMetric runs on one device; merge FeatureMoments across ranks')
    if eval_examples is None:
      raise ValueError('no evaluation data: pass eval_examples (parsed trajectory examples)')
    if unit_test:
      checkpoints = ['test-1']
    elif checkpoints is None:
      checkpoints = self._unevaluated_checkpoints()
    steps = [self._checkpoint_step(c) for c in checkpoints]   # a bad name fails before any work
    self.global_batch_size = self.test_batch_size
    dataset = indoor_datasets.R2RVideoDataset()   # gin supplies its arguments
    dev = self.strategy.device
    self.eval_ds = dataset.input_fn(eval_examples, self.test_batch_size, seed=self.seed, device=dev)
    # a second, independent stream over the same examples (reference :214-225)
    self.display_batch = next(dataset.input_fn(eval_examples, self.test_batch_size, seed=self.seed,
                                               device=dev))
    self.eval_num = (len(eval_examples) if hasattr(eval_examples, '__len__')
                     else dataset.num_examples[self.test_split])
    metric = eval_metric.EvalMetric(ds=self.eval_ds, eval_num=self.eval_size or self.eval_num,
                                    batch_size=self.test_batch_size, strategy=None, avg_num=1,
                                    eval_seq_len=self.eval_seq_len, inception=inception,
                                    frechet=frechet, image_metrics=image_metrics)
    if not hasattr(self, 'generator'):
      self._create_obj()
    rows = []
    for checkpoint_path, step in zip(checkpoints, steps):
      if not unit_test:
        self.restore_checkpoint(checkpoint_path)
      rollouts = self._get_image_grid(self.display_batch,
                                      modes=('ema',) if logger is None else ('normal', 'ema'))
      self._save_rollout_images(rollouts['ema'], step, video=rollout_video)
      fid, _, rmse = metric.calculate_fid_score(self.generator)
      scores = metric.image_scores
      ema_fid, _, ema_rmse = metric.calculate_fid_score(self.ema_generator)
      columns = [('fid', fid), ('ema_fid', ema_fid), ('rmse', rmse), ('ema_rmse', ema_rmse)]
      if image_metrics:
        columns += [('psnr', scores['psnr']), ('ema_psnr', metric.image_scores['psnr']),
                    ('ssim', scores['ssim']), ('ema_ssim', metric.image_scores['ssim'])]
      result = {}
      for i in fid:
        for k, v in columns:
          result[f'{self.test_split}/eval_image/{k}@{i}'] = v[i]
      rows.append(self._add_eval_result(checkpoint_path, step, result))
      if logger is not None:
        logger.log_scalars(step, **{k: float(rows[-1][k]) for k in result})   # as the row has them
        image_dict, _ = self._get_image_dict(rollouts, self.display_batch, self.test_split)
        logger.log_images(step, **image_dict)
        if rollout_video:
          videos = {f'{self.test_split}_{name}_generated_video': self._rollout_videos(rollouts[mode])[0]
                    for name, mode in (('raw', 'normal'), ('ema', 'ema'))}
          if logger.encoder == 'host':
            videos = {k: v.cpu().numpy() for k, v in videos.items()}
          logger.log_videos(step, **videos)
    return rows

  # -------------------------------------------------------------------------- checkpoint
  # The reference keeps tf.train.Checkpoint(generator, discriminator, ema_generator, g_optimizer,
  # d_optimizer) (:333-349).  TensorFlow's bundle format cannot be read or written here; the same
  # state goes to one .npz whose keys are '<object>/<variable path>' with the variable paths of the
  # ParamStore, which mirror the reference's attribute paths (INTEGRATION.md section 5 has the
  # TF-side exporter that produces a compatible file from a real checkpoint).
  def state_dict(self):
    """Flat {key: numpy array} of everything a resumed run needs."""
    out = {'global_step': np.asarray(self.global_step, np.int64)}
    for prefix, model in (('generator', self.generator), ('discriminator', self.discriminator),
                          ('ema_generator', self.ema_generator)):
      for k, v in model.store.to_dict().items():
        out[f'{prefix}/{k}'] = v
    for prefix, opt in (('g_optimizer', self.g_optimizer), ('d_optimizer', self.d_optimizer)):
      out[f'{prefix}/iter'] = np.asarray(opt.iterations, np.int64)
      st = opt.model.store
      m, v = opt.m.detach().cpu().numpy(), opt.v.detach().cpu().numpy()
      for name in st.trainable_names:
        o, n, shape = st._off_tr[name]
        out[f'{prefix}/{name}/m'] = m[o:o + n].reshape(shape).copy()
        out[f'{prefix}/{name}/v'] = v[o:o + n].reshape(shape).copy()
    return out

  def load_state_dict(self, d, strict=True):
    if not hasattr(self, 'generator'):
      self._create_obj()
    seen = set()
    for prefix, model in (('generator', self.generator), ('discriminator', self.discriminator),
                          ('ema_generator', self.ema_generator)):
      sub = {k[len(prefix) + 1:]: d[k] for k in d if k.startswith(prefix + '/')}
      known = {k: v for k, v in sub.items() if k in model.store.views}
      if strict and set(known) != set(model.store.views):
        missing = sorted(set(model.store.views) - set(known))[:5]
        raise KeyError(f'checkpoint lacks {prefix} variables, e.g. {missing}')
      model.store.load_dict(known)
      seen.update(f'{prefix}/{k}' for k in known)
    for prefix, opt in (('g_optimizer', self.g_optimizer), ('d_optimizer', self.d_optimizer)):
      if f'{prefix}/iter' not in d:
        if strict:
          raise KeyError(f'checkpoint lacks {prefix}/iter')
        continue
      opt.iterations = int(d[f'{prefix}/iter'])
      st = opt.model.store
      for name in st.trainable_names:
        o, n, shape = st._off_tr[name]
        for slot, arena in (('m', opt.m), ('v', opt.v)):
          key = f'{prefix}/{name}/{slot}'
          if key in d:
            arena[o:o + n].copy_(torch.as_tensor(np.asarray(d[key]), dtype=torch.float32)
                                 .reshape(-1).to(arena.device))
            seen.add(key)
          elif strict:
            raise KeyError(f'checkpoint lacks {key}')
    if 'global_step' in d:
      self.global_step = int(d['global_step'])
    return sorted(set(d) - seen - {'global_step', 'g_optimizer/iter', 'd_optimizer/iter'})

  def save_checkpoint(self, path):
    """One uncompressed .npz (reference: checkpoint_manager.save, :425-428)."""
    np.savez(path, **self.state_dict())

  def save_checkpoint_async(self, path, snapshot='device', staging_bytes=2 * (256 << 20), writer_hook=None,
                            after=None):
    """The file of save_checkpoint -- the keys and arrays of state_dict() -- written off the step
    (trainers/async_checkpoint.py): nothing goes through state_dict(), the members'
    zip CRC-32s come from the device (se3ds_crc32z_multi) and one background thread writes the file
    through utils/npz_writer from two pinned slabs of staging_bytes / 2.
    snapshot='device': the training stream copies the ten arenas into one snapshot allocation
    (created at the first save and kept; as large as the arenas) and goes on; the file holds the
    state of this moment whatever the trainer does next.  snapshot='direct': no copy; the live
    arenas are read and this call returns once the last device-to-host copy is queued, which the
    training stream then waits for -- for a model whose snapshot does not fit.
    Returns a handle: .done, .wait() (raises what the writer raised), .path.  A save requested while
    one is in flight first waits for it and raises its failure.  Under DataParallelStrategy only
    rank 0 of the group writes; the others get a finished handle.  writer_hook: a callable the
    writer thread invokes before it consumes each slab; after: one it invokes once the file is in
    place."""
    from se3ds_amd.trainers import async_checkpoint
    if not self._writes_checkpoints():
      return async_checkpoint.CheckpointHandle(path)
    if getattr(self, '_checkpointer', None) is None:
      self._checkpointer = async_checkpoint.AsyncCheckpointer(self)
    return self._checkpointer.save(path, snapshot=snapshot, staging_bytes=staging_bytes,
                                   writer_hook=writer_hook, after=after)

  def wait_for_checkpoint(self):
    """Blocks until the save in flight, if any, is in place; raises what its writer raised."""
    if getattr(self, '_checkpointer', None) is not None:
      self._checkpointer.wait()

  def restore_checkpoint(self, path, strict=True):
    """Returns the keys of the file that matched nothing (reference: checkpoint.restore)."""
    with np.load(path) as f:
      return self.load_state_dict({k: f[k] for k in f.files}, strict=strict)

  # ---------------------------------------------------------------------------------- EMA
  def ema_fused_args(self):
    """(ema arena, 1 - decay) for AdamState.apply_gradients when this step's update_ema_model
    will be a moving-average step (not the copy phase), else (None, 0)."""
    if (os.environ.get('SE3DS_UNFUSED_EMA') != '1' and
        self.global_step >= self.ema_init_step + self.num_batched_steps):
      return self.ema_generator.store.theta, 1.0 - self.ema_decay
    return None, 0.0

  def update_ema_model(self, theta_done=False):
    """reference :642-651.  theta_done: the trainable variables were already averaged by the
    optimiser pass (ema_fused_args); only the non-trainable ones are left."""
    if self.global_step >= self.ema_init_step:
      if self.global_step >= self.ema_init_step + self.num_batched_steps:
        ema.update_ema_variables(self.ema_generator, self.generator, self.ema_decay,
                                 skip_trainable=theta_done)
      else:
        assert not theta_done
        self.assign_ema_model_first_time()

  def assign_ema_model_first_time(self):
    ema.assign_ema_vars_from_initial_values(self.ema_generator, self.generator)
