"""The reference's utils/logger.UniversalLogger without TensorFlow: scalars and image grids go to
a TensorBoard event file (utils/tf_events.py) and, for scalars, to the log.  Images are PNG-encoded
on the device in one batch per call (utils/png.encode_png_batch), or on the host for NumPy arrays;
image_format='jpeg' writes baseline JPEG instead (utils/jpeg.encode_jpeg_batch, device only).
Videos go out as animated GIFs in image summaries (utils/gif.py), on the device or on the host."""
import logging
from typing import Callable, Optional

import numpy as np

from se3ds_amd.utils import gif, jpeg, png, tf_events


class UniversalLogger:
  """Constructor surface of the reference (:36-55) plus `encoder`: 'device' takes uint8 device
  tensors, 'host' NumPy arrays (a CPU-only process can write summaries), and `image_format`: 'png'
  (the default) or 'jpeg' at `jpeg_quality`, 4:2:0, which needs encoder='device'; a one-channel
  image becomes a grey file."""

  def __init__(self, workdir: str, step: int, num_train_steps: Optional[int] = None,
               logging_fn: Optional[Callable[[str], None]] = None, encoder: str = 'device',
               image_format: str = 'png', jpeg_quality: int = 90):
    if encoder not in ('host', 'device'):
      raise ValueError(f"encoder: 'host' or 'device', got {encoder!r}")
    if image_format not in ('png', 'jpeg'):
      raise ValueError(f"image_format: 'png' or 'jpeg', got {image_format!r}")
    if image_format == 'jpeg' and encoder != 'device':
      raise ValueError("image_format: 'jpeg' is encoded on the device only (encoder='device')")
    if image_format == 'jpeg':
      jpeg.quality_tables(jpeg_quality)   # ValueError naming quality
    self.image_format, self.jpeg_quality = image_format, jpeg_quality
    self.summary_writer = tf_events.EventFileWriter(workdir)
    self.encoder = encoder
    self._num_train_steps = num_train_steps
    self._print = logging_fn or logging.info
    self._steps_per_sec_start_step = step

  def log_scalars(self, step: int, **kwargs):
    """Log scalars (given as keyword arguments)."""
    log_msg = ', '.join([f'{k} = {v:.3f}' for k, v in sorted(kwargs.items())])
    self._print(f'[{step}] {log_msg}')
    for k, v in sorted(kwargs.items()):
      self.summary_writer.add_scalar(k, float(v), step)
    self.summary_writer.flush()

  def log_images(self, step: int, max_outputs: int = 10, **kwargs):
    """Log images (given as keyword arguments): each value uint8 (k,H,W,C), C 1 or 3.  The first
    min(k, max_outputs) go out under the tag `name` (k = 1) or `name/image/<i>`, as tf.summary.image
    names them; all images of the call are encoded in one batch."""
    tags, images = [], []
    for name, value in sorted(kwargs.items()):
      if len(value.shape) != 4:
        raise ValueError(f'{name}: uint8 (k,H,W,C) expected, got {tuple(value.shape)}')
      if self.encoder == 'host' and not isinstance(value, np.ndarray):
        raise ValueError(f"{name}: encoder='host' takes NumPy arrays")
      count = min(int(value.shape[0]), int(max_outputs))
      for i in range(count):
        tags.append(name if value.shape[0] == 1 else f'{name}/image/{i}')
        images.append(value[i])
    if not images:
      return
    if self.image_format == 'jpeg':
      files = jpeg.encode_jpeg_batch(images, quality=self.jpeg_quality)
    elif self.encoder == 'device':
      files = png.encode_png_batch(images)
    else:
      files = [png.encode_png_host(x) for x in images]
    for tag, x, data in zip(tags, images, files):
      self.summary_writer.add_image(tag, data, int(x.shape[0]), int(x.shape[1]), step,
                                    channels=int(x.shape[2]))
    self.summary_writer.flush()

  def log_videos(self, step: int, fps: float = 10, max_outputs: int = 3, **kwargs):
    """Log videos (given as keyword arguments): each value uint8 (k,T,H,W,C), C 1 or 3.  The first
    min(k, max_outputs) go out as animated GIFs at `fps` under the tag `name` (k = 1) or
    `name/video/<i>`, in an image summary, which is how TensorBoard's image dashboard plays them;
    all videos of the call are encoded in one batch (utils/gif.encode_gif_batch, or encode_gif_host
    for the NumPy arrays of encoder='host')."""
    tags, videos = [], []
    for name, value in sorted(kwargs.items()):
      if len(value.shape) != 5 or value.shape[4] not in (1, 3):
        raise ValueError(f'{name}: uint8 (k,T,H,W,1|3) expected, got {tuple(value.shape)}')
      if (self.encoder == 'host') != isinstance(value, np.ndarray):
        raise ValueError(f"{name}: encoder='host' takes NumPy arrays, encoder='device' device tensors")
      count = min(int(value.shape[0]), int(max_outputs))
      for i in range(count):
        tags.append(name if value.shape[0] == 1 else f'{name}/video/{i}')
        videos.append(value[i])
    if not videos:
      return
    if self.encoder == 'device':
      files = gif.encode_gif_batch(videos, fps=fps)
    else:
      files = [gif.encode_gif_host(x, fps=fps) for x in videos]
    for tag, x, data in zip(tags, videos, files):
      self.summary_writer.add_image(tag, data, int(x.shape[1]), int(x.shape[2]), step,
                                    channels=int(x.shape[3]))
    self.summary_writer.flush()

  def close(self):
    self.summary_writer.close()
