"""Image grids for the TensorBoard summaries: the reference's utils/image_grid.py with the cast and
the tiling in one kernel (`se3ds_grid_quantize`, csrc/png_encode.hip).  Same names, signatures and
dictionary keys; the sheets are uint8 device tensors (1, ny*h, nx*w, c)."""
import logging
import math
from typing import Dict, List, Union

import torch

from se3ds_amd import _lib


def _quantize_to_grid(x: torch.Tensor, ny: int, nx: int, out_c: int) -> torch.Tensor:
  """(N,h,w,c) fp32 / bf16 on the device, N >= ny * nx -> uint8 (1, ny*h, nx*w, out_c):
  tf.cast(x * 255.0, tf.uint8) of the first ny * nx images, image i at row i // nx, column i % nx."""
  _lib.require_cuda(x)
  if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16):
    raise ValueError(f'fp32 or bf16 (N,h,w,c) expected, got {x.dtype} {tuple(x.shape)}')
  x = x.contiguous()
  n, h, w, c = x.shape
  out = torch.empty((1, ny * h, nx * w, out_c), dtype=torch.uint8, device=x.device)
  with torch.cuda.device(x.device):
    rc = _lib.lib().se3ds_grid_quantize(_lib.ptr(x), _lib.dtype_code(x), n, h, w, c, ny, nx, out_c,
                                        _lib.ptr(out), _lib.stream())
  _lib.check(rc, 'se3ds_grid_quantize')
  return out


def images_to_grid(images: torch.Tensor) -> torch.Tensor:
  """Transfer batch images to image grid: (ny, nx, h, w, c) float -> uint8 (1, ny*h, nx*w, c)."""
  ny, nx, h, w, c = images.shape
  return _quantize_to_grid(images.reshape(ny * nx, h, w, c), ny, nx, c)


def get_grid_image(x: torch.Tensor, show_num: int, strategy=None, out_c: int = None) -> torch.Tensor:
  """Concatenate image in each replica together for image grid (reference :33-51).  `strategy` is
  accepted for the reference's call sites; the local result of a tensor is the tensor itself.
  out_c = 3 replicates a 1-channel input, as the reference tiles depth and masks before the call
  (trainers/gan_manager.py:560-567)."""
  del strategy
  if x.shape[0] < show_num:
    logging.info('show_num is cut by the small batch size to %s', x.shape[0])
    show_num = x.shape[0]
  h_num = int(math.sqrt(show_num))
  w_num = int(show_num / h_num)
  return _quantize_to_grid(x, h_num, w_num, x.shape[3] if out_c is None else out_c)


def get_grid_image_dict(images: Union[torch.Tensor, List[torch.Tensor], Dict[str, torch.Tensor]],
                        show_num: int, strategy=None, name_prefix: str = '',
                        out_c: int = None) -> Dict[str, torch.Tensor]:
  """Concatenate image in each replica together for image grid as dict (reference :54-96): a list
  gives name_prefix_<i>, a dict name_prefix_<key>, a tensor name_prefix."""
  out_dict = {}
  if isinstance(images, list):
    for i in range(len(images)):
      out_dict[name_prefix + '_' + str(i)] = get_grid_image(images[i], show_num, strategy, out_c)
  elif isinstance(images, dict):
    for key, value in images.items():
      out_dict[name_prefix + '_' + key] = get_grid_image(value, show_num, strategy, out_c)
  else:
    out_dict[name_prefix] = get_grid_image(images, show_num, strategy, out_c)
  return out_dict
