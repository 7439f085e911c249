"""Builders of synthetic R2R records for the tests: a training Example of seven PNG planes and an
evaluation trajectory Example of serialized tensors, each with the arrays it encodes."""
import numpy as np

import _png_ref
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.utils import tf_records


def image_record(h, rng, filters=None, **overrides):
  """A synthetic training Example at (h, 2h) and the pixel arrays it encodes."""
  w = 2 * h
  pix = dict(image=rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
             proj_image=rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
             depth=rng.integers(0, 65536, (h, w)).astype(np.uint16),
             proj_depth=rng.integers(0, 65536, (h, w)).astype(np.uint16),
             proj_mask=rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255),
             blurred_mask=rng.integers(0, 3, (h, w), dtype=np.uint8),
             segmentation=rng.integers(0, 42, (h, w), dtype=np.uint8))
  feats = {}
  for name, (feature, _, _) in indoor_datasets.IMAGE_PLANES.items():
    ft = rng.integers(0, 5, h) if filters is None else [filters] * h
    feats[feature] = _png_ref.encode_png(pix[name], ft)
  feats.update(overrides)
  return tf_records.encode_example(feats), pix


def video_record(h, rng, pathdreamer=True):
  t, w = 8, 2 * h
  arrays = dict(image=rng.random((t, h, w, 3), dtype=np.float32),
                position=rng.random((t, 4), dtype=np.float32),
                mask=(rng.random(t) < 0.7).astype(np.float32),
                segmentation=rng.integers(0, 42, (t, h, w), dtype=np.uint8),
                depth=rng.random((t, h, w), dtype=np.float32))
  feats = {'id': np.array([17]), 'video/num_frames': np.array([t]), 'scan_id': b'scanA',
           'video/rgb': tf_records.serialize_tensor(arrays['image']),
           'video/position': tf_records.serialize_tensor(arrays['position']),
           'video/mask': tf_records.serialize_tensor(arrays['mask']),
           'video/segmentations': tf_records.serialize_tensor(arrays['segmentation']),
           'video/depth': tf_records.serialize_tensor(arrays['depth'])}
  if pathdreamer:
    arrays['pathdreamer_segmentation'] = rng.integers(0, 42, (t, h, w), dtype=np.uint8)
    arrays['pathdreamer_depth'] = rng.random((t, h, w), dtype=np.float32)
    feats['video/pathdreamer_segmentations'] = tf_records.serialize_tensor(
        arrays['pathdreamer_segmentation'].astype(np.int32))
    feats['video/pathdreamer_depth'] = tf_records.serialize_tensor(arrays['pathdreamer_depth'])
  arrays.update(id=np.int64(17), dataset_type=np.int64(0), depth_scale=np.float32(20.0))
  return tf_records.encode_example(feats), arrays
