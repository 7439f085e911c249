"""Semantic utilities on the device -- utils/utils.py of the reference, under its function names and
argument order (kernels: csrc/semantic.hip, index arithmetic: csrc/nn_inpaint_core.h).

  nearest_neighbor_inpaint(image, void_class=0)   fill the holes of a label panorama (proj_semantic
                                                  is full of INVALID_SEM_VALUE where the splat hit
                                                  nothing) with the nearest label
  compute_sequence_iou / compute_sequence_accuracy   the reference's sequence metrics
  sequence_iou_from_labels                        the IoU of the one-hot encodings of two label maps,
                                                  without forming them (one_hot_mask
                                                  is never materialised)
  create_label_colormap / cmap_to_label / label_to_color   labels <-> PASCAL VOC colours

Every function but create_label_colormap takes device tensors, returns device tensors and never waits
for the device.  There is no CPU fallback: a CPU tensor raises `_lib.Se3dsHipError`.  Shapes and
dtypes are checked first (ValueError), before the device is looked at.

Not carried over: compute_kl, reparameterize (the SE3DS generator returns a zero KLD and
nothing reads them) and get_local_ckpt_path (a gfile copy)."""
from typing import Optional, Tuple

import numpy as np
import torch

from se3ds_amd import _lib

MAX_SIDE = 16384     # csrc/nn_inpaint_core.h kMaxSide
MAX_COLOURS = 256

_INPAINT_DTYPES = (torch.uint8, torch.int32, torch.float32)
_LABEL_DTYPES = (torch.uint8, torch.int32)
_SPATIAL_DTYPES = (torch.bool, torch.uint8, torch.int32, torch.float32)
_SEQ_IOU, _SEQ_ACCURACY, _SEQ_IOU_LABELS = (
    _lib.ABI['SE3DS_SEQ_IOU'], _lib.ABI['SE3DS_SEQ_ACCURACY'], _lib.ABI['SE3DS_SEQ_IOU_LABELS'])

_workspaces = {}   # (purpose, device index, stream) -> uint8 tensor
_cmaps = {}        # (device index, bytes of the int32 table) -> device int32 (K, 3)


def _workspace(purpose, dev, nbytes):
  key = (purpose, dev.index, _lib.stream())
  ws = _workspaces.get(key)
  if ws is None or ws.numel() < nbytes:
    ws = torch.empty((max(int(nbytes), 4096),), dtype=torch.uint8, device=dev)
    _workspaces[key] = ws
  return ws


def _need_tensor(t, name):
  if not isinstance(t, torch.Tensor):
    raise ValueError(f'{name}: a torch tensor is needed, got {type(t).__name__}')


def create_label_colormap() -> np.ndarray:
  """The (256, 3) PASCAL VOC label colour map, host NumPy, dtype int as in the reference: bit 7 - j of
  channel c of label i is bit 3 j + c of i, j = 0..7."""
  label = np.arange(256, dtype=int)
  colormap = np.zeros((256, 3), dtype=int)
  for j in range(8):
    for c in range(3):
      colormap[:, c] |= ((label >> (3 * j + c)) & 1) << (7 - j)
  return colormap


def _cmap_table(cmap, dev):
  """(K, 3) colours, host array or tensor -> device int32 (K, 3); a host table is uploaded once."""
  if isinstance(cmap, torch.Tensor):
    if cmap.dim() != 2 or cmap.shape[1] != 3 or not 1 <= cmap.shape[0] <= MAX_COLOURS:
      raise ValueError(f'cmap: (K, 3) with 1 <= K <= {MAX_COLOURS} is needed, got {tuple(cmap.shape)}')
    if cmap.dtype not in (torch.uint8, torch.int32, torch.int64):
      raise ValueError(f'cmap: unsupported dtype {cmap.dtype}')
    if cmap.is_cuda:
      return cmap.to(device=dev, dtype=torch.int32).contiguous()
    cmap = cmap.numpy()
  table = np.asarray(cmap)
  if table.ndim != 2 or table.shape[1] != 3 or not 1 <= table.shape[0] <= MAX_COLOURS:
    raise ValueError(f'cmap: (K, 3) with 1 <= K <= {MAX_COLOURS} is needed, got {table.shape}')
  if not np.issubdtype(table.dtype, np.integer):
    raise ValueError(f'cmap: unsupported dtype {table.dtype}')
  table = np.ascontiguousarray(np.clip(table, -1, 256).astype(np.int32))   # outside 0..255: no match
  if dev.type != 'cuda':
    return torch.from_numpy(table)
  key = (dev.index, table.tobytes())
  hit = _cmaps.get(key)
  if hit is None:
    if len(_cmaps) >= 16:
      _cmaps.clear()
    hit = _cmaps[key] = torch.from_numpy(table).to(dev)
  return hit


def cmap_to_label(image: torch.Tensor, cmap) -> torch.Tensor:
  """Maps a colour image to labels: the inverse of create_label_colormap.  image (..., 3) uint8 or
  int32 on the device, cmap (K, 3) with K <= 256 (a host array, or a device tensor).  Per pixel the
  first k whose colour equals the pixel, 0 when none does (NumPy's argmax of an all-false row).
  Returns (...) int32 -- NumPy's argmax would give int64."""
  _need_tensor(image, 'image')
  if image.dim() < 1 or image.shape[-1] != 3:
    raise ValueError(f'image: (..., 3) is needed, got {tuple(image.shape)}')
  if image.dtype not in _LABEL_DTYPES:
    raise ValueError(f'image: unsupported dtype {image.dtype} (uint8 or int32)')
  table = _cmap_table(cmap, image.device)
  _lib.require_cuda(image, table)
  image = image.contiguous()
  labels = torch.empty(image.shape[:-1], dtype=torch.int32, device=image.device)
  if labels.numel() == 0:
    return labels
  with torch.cuda.device(image.device):
    _lib.check(_lib.lib().se3ds_cmap_to_label(image.data_ptr(), _lib.dtype_code(image), labels.numel(),
                                              table.data_ptr(), table.shape[0], labels.data_ptr(),
                                              _lib.stream()), 'cmap_to_label')
  return labels


def label_to_color(labels: torch.Tensor, cmap) -> torch.Tensor:
  """(...) uint8 or int32 labels on the device -> (..., 3) uint8 colours cmap[label]; a label outside
  [0, K) becomes (0, 0, 0).  The gather that cmap_to_label inverts."""
  _need_tensor(labels, 'labels')
  if labels.dtype not in _LABEL_DTYPES:
    raise ValueError(f'labels: unsupported dtype {labels.dtype} (uint8 or int32)')
  table = _cmap_table(cmap, labels.device)
  _lib.require_cuda(labels, table)
  labels = labels.contiguous()
  out = torch.empty(tuple(labels.shape) + (3,), dtype=torch.uint8, device=labels.device)
  if labels.numel() == 0:
    return out
  with torch.cuda.device(labels.device):
    _lib.check(_lib.lib().se3ds_label_to_color(labels.data_ptr(), _lib.dtype_code(labels), labels.numel(),
                                               table.data_ptr(), table.shape[0], out.data_ptr(),
                                               _lib.stream()), 'label_to_color')
  return out


def _void_bits(void_class, dtype) -> int:
  if dtype == torch.float32:
    return int(np.array(void_class, dtype=np.float32).view(np.uint32))
  lo, hi = (0, 255) if dtype == torch.uint8 else (-2 ** 31, 2 ** 31 - 1)
  v = int(void_class)
  if v != void_class or not lo <= v <= hi:
    raise ValueError(f'void_class {void_class!r} is no {dtype} value')
  return v & 0xffffffff


def nearest_neighbor_inpaint(image: torch.Tensor, void_class=0, return_indices: bool = False):
  """Fills the pixels of image (N, H, W) uint8 / int32 / float32 that equal void_class with the value of
  the nearest pixel of the same image that does not (squared Euclidean distance in pixels); all other
  pixels are unchanged and values are copied bit for bit.  Among equidistant sources the smallest
  row wins, within it the smallest column: the reference's argmin over tf.where's row-major list.
  Equality is == of the dtype: for floats -0.0 equals a 0.0 void class and a NaN pixel is never void.

  return_indices=True returns (filled, indices): indices (N, H, W) int32 holds the flat index
  y * W + x of every pixel's source -- its own for a non-void pixel -- so that a depth or RGB plane
  can be filled with the same neighbours; -1 where the image has no non-void pixel at all.

  An image without a non-void pixel comes back unchanged.  The reference fails there (argmin over an
  empty axis); detecting it here would need a synchronisation with the host, which this function
  never does.  An image without a void pixel is returned unchanged.  1 <= H, W <= 16384."""
  _need_tensor(image, 'image')
  if image.dim() != 3:
    raise ValueError(f'image: (N, H, W) is needed, got {tuple(image.shape)}')
  if image.dtype not in _INPAINT_DTYPES:
    raise ValueError(f'image: unsupported dtype {image.dtype} (uint8, int32 or float32)')
  bits = _void_bits(void_class, image.dtype)
  _lib.require_cuda(image)
  image = image.contiguous()
  n, h, w = image.shape
  L = _lib.lib()
  out = torch.empty_like(image)
  indices = torch.empty((n, h, w), dtype=torch.int32, device=image.device) if return_indices else None
  with torch.cuda.device(image.device):
    ws_bytes = int(L.se3ds_nn_inpaint_workspace_bytes(n, h, w))   # 0 for a shape the call refuses
    ws = _workspace('inpaint', image.device, ws_bytes)
    _lib.check(L.se3ds_nn_inpaint(image.data_ptr(), _lib.dtype_code(image), bits, n, h, w, out.data_ptr(),
                                  _lib.ptr(indices), ws.data_ptr(), ws.numel(), 3, _lib.stream()),
               'nn_inpaint')
  return (out, indices) if return_indices else out


def _seq_mask(mask, n, t, dev):
  _need_tensor(mask, 'mask')
  if tuple(mask.shape) != (n, t):
    raise ValueError(f'mask: ({n}, {t}) is needed, got {tuple(mask.shape)}')
  return mask


def _finalize(sums, mask, n, t, mode):
  dev = sums.device
  mask = mask.to(dtype=torch.float32).contiguous()
  seq = torch.empty((n, t), dtype=torch.float32, device=dev)
  mean = torch.empty((), dtype=torch.float32, device=dev)
  _lib.check(_lib.lib().se3ds_seq_finalize(sums.data_ptr(), mask.data_ptr(), n, t, mode, seq.data_ptr(),
                                           mean.data_ptr(), _lib.stream()), 'seq_finalize')
  return seq, mean


def compute_sequence_iou(one_hot_pred: torch.Tensor, one_hot_true: torch.Tensor, mask: torch.Tensor,
                         spatial_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
  """Mean intersection over union of two one-hot sequences (N, T, H, W, C) float32.  mask (N, T): 0
  for padding frames; spatial_mask (N, T, H, W) float32: 0 for pixels that do not count.  Per frame
  I = sum p t s and S = sum (p + t) s in binary64, then in float32 seq_iou = divide_no_nan(I mask,
  (S - I) mask), per example sum_t seq_iou / sum_t mask (divide_no_nan), and the mean over N.
  Returns (seq_iou (N, T), mean ()), both float32 on the device."""
  for name, x in (('one_hot_pred', one_hot_pred), ('one_hot_true', one_hot_true)):
    _need_tensor(x, name)
    if x.dim() != 5:
      raise ValueError(f'{name}: (N, T, H, W, C) is needed, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
      raise ValueError(f'{name}: unsupported dtype {x.dtype} (float32)')
  if one_hot_pred.shape != one_hot_true.shape:
    raise ValueError(f'one_hot_true: {tuple(one_hot_true.shape)} for a prediction of {tuple(one_hot_pred.shape)}')
  n, t, h, w, c = one_hot_pred.shape
  _seq_mask(mask, n, t, one_hot_pred.device)
  if spatial_mask is not None:
    _need_tensor(spatial_mask, 'spatial_mask')
    if tuple(spatial_mask.shape) != (n, t, h, w):
      raise ValueError(f'spatial_mask: {(n, t, h, w)} is needed, got {tuple(spatial_mask.shape)}')
    if spatial_mask.dtype != torch.float32:
      raise ValueError(f'spatial_mask: unsupported dtype {spatial_mask.dtype} (float32)')
  _lib.require_cuda(one_hot_pred, one_hot_true, mask, spatial_mask)
  pred, true = one_hot_pred.contiguous(), one_hot_true.contiguous()
  spatial = None if spatial_mask is None else spatial_mask.contiguous()
  L = _lib.lib()
  dev = pred.device
  with torch.cuda.device(dev):
    sums = torch.empty((max(n * t, 1), 2), dtype=torch.float64, device=dev)
    ws_bytes = int(L.se3ds_seq_sums_workspace_bytes(n * t, h * w * c))
    ws = _workspace('sums', dev, ws_bytes)
    _lib.check(L.se3ds_seq_iou_sums(pred.data_ptr(), true.data_ptr(), _lib.ptr(spatial), n * t, h * w, c,
                                    sums.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), 'seq_iou_sums')
    return _finalize(sums, mask, n, t, _SEQ_IOU)


def _label_sums(class_pred, class_gt, mask, spatial_mask, mode):
  for name, x in (('class_pred', class_pred), ('class_gt', class_gt)):
    _need_tensor(x, name)
    if x.dim() != 4:
      raise ValueError(f'{name}: (N, T, H, W) is needed, got {tuple(x.shape)}')
    if x.dtype not in _LABEL_DTYPES:
      raise ValueError(f'{name}: unsupported dtype {x.dtype} (uint8 or int32)')
  if class_pred.shape != class_gt.shape or class_pred.dtype != class_gt.dtype:
    raise ValueError(f'class_gt: {tuple(class_gt.shape)} {class_gt.dtype} for a prediction of '
                     f'{tuple(class_pred.shape)} {class_pred.dtype}')
  n, t, h, w = class_pred.shape
  _seq_mask(mask, n, t, class_pred.device)
  if spatial_mask is not None:
    _need_tensor(spatial_mask, 'spatial_mask')
    if tuple(spatial_mask.shape) != (n, t, h, w):
      raise ValueError(f'spatial_mask: {(n, t, h, w)} is needed, got {tuple(spatial_mask.shape)}')
    if spatial_mask.dtype not in _SPATIAL_DTYPES:
      raise ValueError(f'spatial_mask: unsupported dtype {spatial_mask.dtype} (bool, uint8, int32 or float32)')
  _lib.require_cuda(class_pred, class_gt, mask, spatial_mask)
  pred, gt = class_pred.contiguous(), class_gt.contiguous()
  spatial, spatial_code = None, -1
  if spatial_mask is not None:
    spatial = spatial_mask.contiguous()
    if spatial.dtype == torch.bool:
      spatial = spatial.view(torch.uint8)   # one byte, 0 or 1
    spatial_code = _lib.dtype_code(spatial)
  L = _lib.lib()
  dev = pred.device
  with torch.cuda.device(dev):
    sums = torch.empty((max(n * t, 1), 2), dtype=torch.float64, device=dev)
    ws_bytes = int(L.se3ds_seq_sums_workspace_bytes(n * t, h * w))
    ws = _workspace('sums', dev, ws_bytes)
    _lib.check(L.se3ds_seq_label_match(pred.data_ptr(), gt.data_ptr(), _lib.dtype_code(pred), _lib.ptr(spatial),
                                       spatial_code, n * t, h * w, sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.stream()), 'seq_label_match')
    return _finalize(sums, mask, n, t, mode)


def compute_sequence_accuracy(class_pred: torch.Tensor, class_gt: torch.Tensor, mask: torch.Tensor,
                              spatial_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
  """Pixel accuracy of two label sequences (N, T, H, W), both uint8 or both int32.  Per frame
  sum [pred == gt] s / sum s (divide_no_nan; s = spatial_mask (N, T, H, W) bool / uint8 / int32 /
  float32, absent: 1), then per example sum_t / sum_t mask and the mean over N as in
  compute_sequence_iou.  Returns (seq_accuracy (N, T), mean ()), float32 on the device."""
  return _label_sums(class_pred, class_gt, mask, spatial_mask, _SEQ_ACCURACY)


def sequence_iou_from_labels(class_pred: torch.Tensor, class_gt: torch.Tensor, mask: torch.Tensor,
                             spatial_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
  """What compute_sequence_iou gives for the one-hot encodings of two label maps, without forming
  them: for one-hot inputs I = sum [pred == gt] s and S = 2 sum s, the reduction of the accuracy.
  Not in the reference, whose IoU needs the (N, T, H, W, C) tensors this project never builds.
  Arguments and results as compute_sequence_accuracy."""
  return _label_sums(class_pred, class_gt, mask, spatial_mask, _SEQ_IOU_LABELS)
