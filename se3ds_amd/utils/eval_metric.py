"""The autoregressive evaluation roll-out -- the loop body the reference runs in
utils/eval_metric.py `_get_generated_pool.step_fn` (:144-239) and in trainers/gan_manager.py
`_get_image_grid` (:458-541): project the point-cloud memory to the next position, mask, run the
generator in inference mode, quantise, unproject the (ground-truth first, then generated) frame and
append it to the memory -- as ONE on-device pipeline.  Every arithmetic step runs in
libse3ds_hip.so; the memory lives in preallocated HBM buffers (PointCloudMemory), so no frame ever
copies it.

EvalMetric is the other half of the reference's evaluator (:66-343): the FID per frame index of the
roll-out against real frames, averaged over `avg_num` repeats, and the depth RMSE.  Real and
generated frames go through the augment + crop + resize gather and Inception-v3 on the device
(utils/inception_utils.py); their 2048-d pools are reduced there into binary64 moments
(FeatureMoments), so only the mean and covariance reach the host for the Frechet distance -- or, with
frechet='device', nothing but the distance does (inception_utils.frechet_distance_device)."""
from typing import Callable, Dict, Iterator, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from se3ds_amd import _lib
from se3ds_amd import constants
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.models.models import _quantize
from se3ds_amd.utils import image_metrics as image_metrics_lib
from se3ds_amd.utils import inception_utils
from se3ds_amd.utils import pano_utils
from se3ds_amd.utils import point_cloud_utils
from se3ds_amd.utils.point_cloud_utils import PointCloudMemory


class RolloutOutput(NamedTuple):
  generated: List[torch.Tensor]     # per frame (N,H,W,3) fp32 in [0,1]
  pred_depth: List[torch.Tensor]    # per frame (N,H,W,1): the depth that entered the memory
  projected: List[torch.Tensor]     # per frame proj_image (N,H,W,3) fp32
  proj_mask: List[torch.Tensor]     # per frame (N,H,W,1)
  proj_depth: List[torch.Tensor]    # per frame (N,H,W,1)
  depth_rmse: List[torch.Tensor]    # per frame (N,) (eval_metric.py:225-234)
  memory: PointCloudMemory
  psnr: Sequence[torch.Tensor] = ()   # image_metrics=True: per frame (N,) float64, generated[k] against
  ssim: Sequence[torch.Tensor] = ()   # image[:, k] at max_val 1 (utils/image_metrics.py); else empty


def depth_rmse(depth: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
  """sqrt(sum((d - t)^2 * 1[0 < t < 1]) / max(count, 1)) per sample (eval_metric.py:225-234)."""
  n = depth.shape[0]
  p = depth.numel() // n
  dev = depth.device
  L = _lib.lib()
  depth, target = depth.contiguous(), target.contiguous()
  ws = torch.empty(n * 256, dtype=torch.float32, device=dev)
  num = torch.empty(n, dtype=torch.float32, device=dev)
  cnt = torch.empty(n, dtype=torch.float32, device=dev)
  _lib.check(L.se3ds_sample_sum(depth.data_ptr(), target.data_ptr(), None, n, p, 1, 4,
                                num.data_ptr(), ws.data_ptr(), _lib.stream()), 'se3ds_sample_sum')
  _lib.check(L.se3ds_sample_sum(target.data_ptr(), None, None, n, p, 1, 2, cnt.data_ptr(),
                                ws.data_ptr(), _lib.stream()), 'se3ds_sample_sum')
  # N scalars: finished on the host when read (the loop itself never synchronises)
  return torch.sqrt(num / torch.clamp(cnt, min=1))


def generated_rollout(generator_fn: Callable, inputs: Dict[str, torch.Tensor], eval_seq_len: int,
                      predict_depth: bool = True,
                      unproject_void_class: float = constants.INVALID_RGB_VALUE,
                      image_metrics: bool = False) -> RolloutOutput:
  """inputs: image (N,T,H,W,3) fp32 [0,1], depth (N,T,H,W,1), position (N,T,3), depth_scale (N,).
  generator_fn(inputs=[cond, None], training=False) -> [mu, logvar, kld, depth, seg, depth_seg,
  rgb].  `unproject_void_class`: eval_metric.py:236-238 passes INVALID_RGB_VALUE, gan_manager.py:
  536-539 passes 0 -- both are kept.  predict_depth=False feeds the ground-truth depth of every
  frame (gan_manager.py:468-469).  image_metrics=True also scores every generated frame against its
  ground-truth frame: out.psnr[k], out.ssim[k] (N,) float64 (not in the reference)."""
  image, depth, position = inputs['image'], inputs['depth'], inputs['position']
  _lib.require_cuda(image, depth, position)
  n, t, h, w, _ = image.shape
  if eval_seq_len > t:
    raise ValueError(f'eval_seq_len {eval_seq_len} exceeds the {t} frames of the batch')
  depth_scale = float(inputs['depth_scale'][0])   # all depth_scale within a batch are the same
  dev = image.device
  memory = PointCloudMemory(n, 3, torch.int32, dev, capacity=eval_seq_len * h * w)
  out = RolloutOutput([], [], [], [], [], [], memory, [], [])
  prev_rgb = None
  for k in range(eval_seq_len):
    target_depth = depth[:, k].contiguous()
    rgb = image[:, k].contiguous()
    depth_tensor = target_depth
    pos = position[:, k].contiguous()
    # memory - position, projection, splat and the mask (eval_metric.py:160-172) in one call
    pred_depth, pred_rgb, pred_mask = memory.project(
        h, w, constants.INVALID_RGB_VALUE, depth_scale, position=pos, with_mask=True,
        mask_void=constants.INVALID_RGB_VALUE)
    pred_rgb = _quantize(pred_rgb, torch.float32, div=255.0, lo=0.0, hi=1.0)
    if prev_rgb is None:
      prev_rgb = torch.zeros_like(rgb)
    first = 1.0 if k == 0 else 0.0
    cond = {
        'prev_image': prev_rgb, 'proj_image': pred_rgb, 'proj_mask': pred_mask[..., None],
        'proj_depth': pred_depth[..., None], 'blurred_mask': torch.zeros_like(pred_depth)[..., None],
        'first_frame': torch.full((n,), first, device=dev),
        'dataset_type': inputs.get('dataset_type'), 'depth': depth_tensor,
    }
    outs = generator_fn(inputs=[cond, None], training=False)
    depth_out, generated = outs[3], outs[6]
    if k == 0:
      prev_rgb = rgb
      # ground truth: the blurred top / bottom rows never enter the memory (:213-217)
      rgb_mem = pano_utils.mask_pano(rgb, masked_region_value=constants.INVALID_RGB_VALUE)
    else:
      rgb_mem = generated
      prev_rgb = generated
      if predict_depth and depth_out is not None:
        depth_tensor = depth_out
    out.depth_rmse.append(depth_rmse(depth_tensor, target_depth))
    # int32(rgb * 255) clipped to [-1, 255] (:234-236), unprojected at the frame's position
    pc_rgb = _quantize(rgb_mem, torch.int32, mul=255.0, lo=constants.INVALID_RGB_VALUE, hi=255)
    memory.append_equirect(pc_rgb, depth_tensor[..., 0], unproject_void_class, depth_scale,
                           position=pos)
    out.generated.append(generated)
    if image_metrics:
      frame = generated.to(torch.float32)
      out.psnr.append(image_metrics_lib.psnr(frame, rgb, 1.0))
      out.ssim.append(image_metrics_lib.ssim(frame, rgb, 1.0))
    out.pred_depth.append(depth_tensor)
    out.projected.append(pred_rgb)
    out.proj_mask.append(pred_mask[..., None])
    out.proj_depth.append(pred_depth[..., None])
  point_cloud_utils.check_promise(memory.device)   # (the roll-out's results are read next)
  return out


class EvalMetric:
  """FID (and depth RMSE) of a generator's roll-outs (reference utils/eval_metric.py:66-343).

  ds: an iterator of the batch dicts generated_rollout takes (image (N,T,H,W,3) fp32 [0,1], depth,
  position, depth_scale; an `original_image` entry, if present, supplies the real frames as in the
  reference).  eval_num rows per frame index enter each statistic; `inception` defaults to
  inception_utils.inception_model() (gin-configurable).  Augment draws come from a NumPy generator
  seeded with `seed`.  strategy: only None (a single device) is supported; per-rank
  FeatureMoments can be merged by the caller.  keep_pools: also keep the host copies of the pools
  of the real set and of the last repeat (tests).  frechet: 'host' (NumPy / SciPy sqrtm, the
  reference's formulation) or 'device' (FeatureMoments.fid(method='device'): the real set's matrix
  square root is computed once per frame index and reused for every generator and repeat).
  image_metrics: calculate_fid_score also averages the PSNR and SSIM of every generated frame against
  its ground-truth frame into self.image_scores (utils/image_metrics.py; not in the reference)."""

  def __init__(self, ds: Iterator, eval_num: int, batch_size: int, strategy=None, avg_num: int = 3,
               num_splits: int = 1, eval_seq_len: int = 5,
               inception: Optional[inception_utils.InceptionV3] = None, seed: int = 0,
               keep_pools: bool = False, frechet: str = 'host', image_metrics: bool = False) -> None:
    if strategy is not None:
      raise NotImplementedError('EvalMetric runs on one device; merge FeatureMoments across ranks')
    if frechet not in inception_utils.FRECHET_METHODS:
      raise ValueError(f'unknown Frechet method {frechet!r}: one of {inception_utils.FRECHET_METHODS}')
    self.frechet = frechet
    self.image_metrics = image_metrics
    self.image_scores = None
    self.ds = ds
    self.eval_num = eval_num
    self.batch_size = batch_size
    self.strategy = strategy
    self.avg_num = avg_num
    self.num_splits = num_splits
    self.eval_seq_len = eval_seq_len
    self._inception_model = inception if inception is not None else inception_utils.inception_model()
    self._rng = np.random.default_rng(seed)
    self.keep_pools = keep_pools
    self.real_pools = None
    self.generated_pools = None
    self.fid_list = None
    # Real statistics once (:107-131, 269-286)
    def real_fn(batch):
      image = batch.get('original_image', batch['image'])
      return {i: image[:, i] for i in range(1, eval_seq_len)}, None

    self._real = self._moments(real_fn, 'real_pools')

  def _pools(self, frames: torch.Tensor) -> torch.Tensor:
    """augment -> crop_pano(resize_to_original=False) -> get_inception (:114-131, 240-251)."""
    n, _, w, _ = frames.shape
    rf = np.array([indoor_datasets.draw_augment(self._rng, w) for _ in range(n)], np.int32)
    x = inception_utils.preprocess(frames, roll_flip=rf, crop=True, dtype=self._inception_model.dtype)
    pools, _ = self._inception_model(x)
    return pools

  def _moments(self, frames_fn, keep_attr, rows=None):
    """Per frame index 1..T-1: FeatureMoments over the first eval_num rows of
    (eval_num // batch_size + 1) batches (:269-315).  frames_fn(batch) -> (frames, scores): scores is
    None or {name: {i: (N,) tensor}}, per-row values of the same rows; `rows` receives them as
    {name: {i: host array}}."""
    stats = {i: inception_utils.FeatureMoments(device=self._inception_model.device)
             for i in range(1, self.eval_seq_len)}
    kept = {i: [] for i in stats}
    score_rows = {}
    left = self.eval_num
    for _ in range(self.eval_num // self.batch_size + 1):
      batch = next(self.ds)
      frames, scores = frames_fn(batch)
      if left <= 0:
        continue   # (the reference draws the batch and drops it)
      for i in stats:
        pools = self._pools(frames[i].contiguous())[:left]
        stats[i].update(pools)
        if self.keep_pools:
          kept[i].append(pools.cpu().numpy())
        for name, per_frame in (scores or {}).items():
          score_rows.setdefault(name, {k: [] for k in stats})[i].append(per_frame[i][:left].cpu().numpy())
      left -= min(left, frames[1].shape[0])
    if self.keep_pools:
      setattr(self, keep_attr, {i: np.concatenate(v) for i, v in kept.items()})
    if rows is not None:
      rows.update({name: {i: np.concatenate(v) for i, v in per_frame.items()}
                   for name, per_frame in score_rows.items()})
    return stats

  def calculate_fid_score(self, generator_fn: Callable):
    """(fid, fid_std, rmse): dicts keyed by frame index 1..T-1 (:317-343).  With image_metrics the
    call also sets self.image_scores = {'psnr': {i: ...}, 'ssim': {i: ...}}, averaged over the rows
    and the repeats exactly as rmse is."""
    indices = range(1, self.eval_seq_len)

    def frames_fn(batch):
      out = generated_rollout(generator_fn, batch, self.eval_seq_len, image_metrics=self.image_metrics)
      scores = {'rmse': {i: out.depth_rmse[i] for i in indices}}
      if self.image_metrics:
        scores['psnr'] = {i: out.psnr[i] for i in indices}
        scores['ssim'] = {i: out.ssim[i] for i in indices}
      return {i: out.generated[i] for i in indices}, scores

    fid_list = {i: [] for i in indices}
    score_list = {name: {i: [] for i in indices}
                  for name in (('rmse', 'psnr', 'ssim') if self.image_metrics else ('rmse',))}
    for _ in range(self.avg_num):
      totals = {}
      gen = self._moments(frames_fn, 'generated_pools', rows=totals)
      for i in fid_list:
        if self.frechet == 'host':
          fid_list[i].append(gen[i].fid(self._real[i]))
        else:   # the real set owns the cached root; the trace term is symmetric in the two sets
          fid_list[i].append(self._real[i].fid(gen[i], method=self.frechet))
        for name in score_list:
          score_list[name][i].append(np.mean(totals[name][i]))
    self.fid_list = fid_list
    fid = {k: np.mean(v) for k, v in fid_list.items()}
    fid_std = {k: np.std(v) for k, v in fid_list.items()}
    means = {name: {k: np.mean(v) for k, v in per_frame.items()} for name, per_frame in score_list.items()}
    rmse = means.pop('rmse')
    if self.image_metrics:
      self.image_scores = means
    return fid, fid_std, rmse
