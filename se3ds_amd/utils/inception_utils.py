"""Inception-v3 FID and Inception Score -- the reference's utils/inception_utils.py on the device.

The network is Keras `InceptionV3(include_top=True)` at 299 x 299 (94 Conv2D + 94
BatchNormalization + the `predictions` Dense layer; 23,851,784 parameters of which 34,432 are the
BN moving statistics).  Keras `conv2d_bn` is Conv2D without bias -> BatchNormalization(scale=False,
eps=1e-3) on its moving statistics -> ReLU; the batch norm is folded at load time into fp32 weights
w * rsqrt(var + eps) per output channel with bias beta - mean * rsqrt(var + eps), so every layer is
one se3ds_conv2d_fwd with its bias + ReLU epilogue.  Pooling, the input gather, the global average
pool, the softmax and the binary64 feature moments are csrc/inception.hip.  The Frechet distance runs
on the host in NumPy / SciPy as in the reference (sqrtm of a 2048 x 2048 product; the default), or,
opt-in, on the device (csrc/frechet.hip, `frechet_distance_device`, `FeatureMoments.fid(method=
'device')`): tr sqrt(S1 S2) = tr sqrt(R S2 R) with R = sqrt(S1), both roots of symmetric PSD matrices
by a coupled Newton-Schulz iteration on a binary64 MFMA GEMM.  The Inception Score stays in NumPy.

Weights: a `tf.train.Checkpoint(inception_v3=model)` directory (reference
inception_utils.py:_inception_model_v3) read with utils/tf_bundle.py, or an .npz keyed by Keras layer
names (`conv2d_17/kernel`, `batch_normalization_17/moving_mean`, `predictions/bias`, ...).  The
ImageNet weights themselves are not shipped: `checkpoint_path=None` (a download in the reference) is
an error here.

CHECKPOINT MAPPING UNPINNED: a Keras functional model reaches its layers through
`layer_with_weights-<k>`, k counting the layers that own variables in `model.layers` order
(`Functional._layer_checkpoint_dependencies`).  That order is not the creation order: tf.keras 2.x
`functional._map_graph_network` sorts the layers by depth -- the longest path to the output, deepest
first -- and breaks ties by the pre-order index of a depth-first walk from the output that visits each
node's inputs in order (`_build_map`).  `keras_layer_order` restates that algorithm on the layer graph
of applications/inception_v3.py (Input, Conv2D, BatchNormalization, Activation, pooling, Concatenate,
GlobalAveragePooling2D, Dense nodes) and `bundle_keys` numbers the weighted layers from it: the stem
is k = 0..9 in creation order, but at mixed0 k = 10 is conv2d_8, the first 1x1 of the deepest branch.
The restatement is checked against hand-derived indices, not against a checkpoint written by
TensorFlow (not available to this project).  Every shape is checked at load.
"""
import os
import warnings
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
from scipy import linalg
import torch

from se3ds_amd import _lib
from se3ds_amd import gin_lite as gin
from se3ds_amd.utils import pano_utils
from se3ds_amd.utils import tf_bundle
from se3ds_amd.utils.tf_checkpoint_keys import SUFFIX

INPUT_SIZE = 299
POOL_DIM, NUM_CLASSES = 2048, 1000
BN_EPS = 1e-3
BUNDLE_ROOT = 'inception_v3'
_RELU = 1


class ShapeNotMatchError(Exception):
  """Prints error when the shape of two tensor does not match."""
  pass


class ImaginaryComponentError(Exception):
  """Prints error when the input has imaginary component."""
  pass


# ------------------------------------------------------------------------------ architecture
def _name(base, i):
  return base if i == 0 else f'{base}_{i}'


def _architecture(ops, x):
  """Keras applications/inception_v3.py, channels_last, in its layer creation order.  `ops` is a
  shape tracer (_Specs) or the device executor (_Device)."""
  cbn = ops.conv_bn
  x = cbn(x, 32, 3, 3, 2, 'valid')
  x = cbn(x, 32, 3, 3, 1, 'valid')
  x = cbn(x, 64, 3, 3)
  x = ops.maxpool(x)
  x = cbn(x, 80, 1, 1, 1, 'valid')
  x = cbn(x, 192, 3, 3, 1, 'valid')
  x = ops.maxpool(x)
  for pool_c in (32, 64, 64):                    # mixed0..2: 35 x 35 x 256 / 288 / 288
    b1 = cbn(x, 64, 1, 1)
    b5 = cbn(cbn(x, 48, 1, 1), 64, 5, 5)
    bd = cbn(cbn(cbn(x, 64, 1, 1), 96, 3, 3), 96, 3, 3)
    bp = cbn(ops.avgpool(x), pool_c, 1, 1)
    x = ops.concat([b1, b5, bd, bp])
  b3 = cbn(x, 384, 3, 3, 2, 'valid')             # mixed3: 17 x 17 x 768
  bd = cbn(cbn(cbn(x, 64, 1, 1), 96, 3, 3), 96, 3, 3, 2, 'valid')
  x = ops.concat([b3, bd, ops.maxpool(x)])
  for c7 in (128, 160, 160, 192):                # mixed4..7: 17 x 17 x 768
    b1 = cbn(x, 192, 1, 1)
    b7 = cbn(cbn(cbn(x, c7, 1, 1), c7, 1, 7), 192, 7, 1)
    bd = cbn(x, c7, 1, 1)
    bd = cbn(bd, c7, 7, 1)
    bd = cbn(bd, c7, 1, 7)
    bd = cbn(bd, c7, 7, 1)
    bd = cbn(bd, 192, 1, 7)
    bp = cbn(ops.avgpool(x), 192, 1, 1)
    x = ops.concat([b1, b7, bd, bp])
  b3 = cbn(cbn(x, 192, 1, 1), 320, 3, 3, 2, 'valid')   # mixed8: 8 x 8 x 1280
  b7 = cbn(cbn(cbn(cbn(x, 192, 1, 1), 192, 1, 7), 192, 7, 1), 192, 3, 3, 2, 'valid')
  x = ops.concat([b3, b7, ops.maxpool(x)])
  for _ in range(2):                             # mixed9, 10: 8 x 8 x 2048
    b1 = cbn(x, 320, 1, 1)
    b3 = cbn(x, 384, 1, 1)
    b3 = ops.concat([cbn(b3, 384, 1, 3), cbn(b3, 384, 3, 1)])
    bd = cbn(cbn(x, 448, 1, 1), 384, 3, 3)
    bd = ops.concat([cbn(bd, 384, 1, 3), cbn(bd, 384, 3, 1)])
    bp = cbn(ops.avgpool(x), 192, 1, 1)
    x = ops.concat([b1, b3, bd, bp])
  return ops.head(x)


class _Specs:
  """Shape tracer: x = (h, w, c); records (cin, cout, kh, kw, stride, padding) per conv."""

  def __init__(self):
    self.convs = []

  def conv_bn(self, x, cout, kh, kw, stride=1, padding='same'):
    h, w, c = x
    self.convs.append((c, cout, kh, kw, stride, padding))
    if padding == 'valid':
      return ((h - kh) // stride + 1, (w - kw) // stride + 1, cout)
    return (-(-h // stride), -(-w // stride), cout)

  def maxpool(self, x):
    h, w, c = x
    return ((h - 3) // 2 + 1, (w - 3) // 2 + 1, c)

  def avgpool(self, x):
    return x

  def concat(self, parts):
    return parts[0][:2] + (sum(p[2] for p in parts),)

  def head(self, x):
    assert x == (8, 8, POOL_DIM), x
    return x


def conv_specs():
  s = _Specs()
  _architecture(s, (INPUT_SIZE, INPUT_SIZE, 3))
  return s.convs


def weight_shapes() -> Dict[str, tuple]:
  """Keras layer-name keyed shapes of every variable, in layer creation order."""
  out = {}
  for i, (cin, cout, kh, kw, _, _) in enumerate(conv_specs()):
    out[_name('conv2d', i) + '/kernel'] = (kh, kw, cin, cout)
    bn = _name('batch_normalization', i)
    for v in ('beta', 'moving_mean', 'moving_variance'):
      out[f'{bn}/{v}'] = (cout,)
  out['predictions/kernel'] = (POOL_DIM, NUM_CLASSES)
  out['predictions/bias'] = (NUM_CLASSES,)
  return out


class _Graph:
  """Layer-graph tracer: one node per Keras layer of applications/inception_v3.py.  A node is
  (name, input node ids); x is a node id."""

  def __init__(self):
    self.nodes = [('input', [])]
    self.i = 0

  def _add(self, name, inputs):
    self.nodes.append((name, inputs))
    return len(self.nodes) - 1

  def conv_bn(self, x, cout, kh, kw, stride=1, padding='same'):
    x = self._add(_name('conv2d', self.i), [x])
    x = self._add(_name('batch_normalization', self.i), [x])
    self.i += 1
    return self._add('activation', [x])

  def maxpool(self, x):
    return self._add('max_pooling2d', [x])

  def avgpool(self, x):
    return self._add('average_pooling2d', [x])

  def concat(self, parts):
    return self._add('concatenate', list(parts))

  def head(self, x):
    return self._add('predictions', [self._add('avg_pool', [x])])


def keras_layer_order() -> List[str]:
  """Names of InceptionV3's layers in Keras `model.layers` order (tf.keras 2.x
  functional._map_graph_network): depth = longest path to the output, deepest first, ties by the
  pre-order index of _build_map's depth-first walk from the output (inputs visited in order)."""
  g = _Graph()
  out = _architecture(g, 0)
  index, post, done = {}, [], set()

  def visit(v):   # _build_map_helper: pre-order index, post-order node list
    index[v] = len(index)
    for u in g.nodes[v][1]:
      if u not in done:
        visit(u)
    done.add(v)
    post.append(v)

  visit(out)
  depth = {}
  for v in reversed(post):   # consumers before producers
    d = depth.setdefault(v, 0)
    for u in g.nodes[v][1]:
      depth[u] = max(depth.get(u, 0), d + 1)
  order = sorted(post, key=lambda v: (-depth[v], index[v]))
  return [g.nodes[v][0] for v in order]


def bundle_keys() -> Dict[str, str]:
  """Keras variable name -> object-graph key of a tf.train.Checkpoint(inception_v3=model):
  `layer_with_weights-<k>` numbers the weighted layers in keras_layer_order()."""
  weighted = [n for n in keras_layer_order()
              if n.startswith(('conv2d', 'batch_normalization')) or n == 'predictions']
  out = {}
  for k, layer in enumerate(weighted):
    if layer.startswith('conv2d'):
      names = ('kernel',)
    elif layer == 'predictions':
      names = ('kernel', 'bias')
    else:
      names = ('beta', 'moving_mean', 'moving_variance')
    for v in names:
      out[f'{layer}/{v}'] = f'{BUNDLE_ROOT}/layer_with_weights-{k}/{v}{SUFFIX}'
  return out


# ------------------------------------------------------------------------------ weights
def random_weights(seed: int = 0) -> Dict[str, np.ndarray]:
  """Deterministic random weights with non-trivial BN statistics (tests, benchmarks): He-normal
  kernels, beta / moving_mean in +-0.1, moving_variance in [0.5, 1.5]."""
  rng = np.random.default_rng(seed)
  out = {}
  for k, shape in weight_shapes().items():
    if k == 'predictions/kernel':
      lim = np.sqrt(6.0 / (shape[0] + shape[1]))
      a = rng.uniform(-lim, lim, shape)
    elif k.endswith('/kernel'):
      a = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))
    elif k.endswith('moving_variance'):
      a = rng.uniform(0.5, 1.5, shape)
    else:
      a = rng.uniform(-0.1, 0.1, shape)
    out[k] = a.astype(np.float32)
  return out


def _checked(weights: Dict[str, np.ndarray], source: str) -> Dict[str, np.ndarray]:
  shapes = weight_shapes()
  missing = [k for k in shapes if k not in weights]
  if missing:
    raise ValueError(f'{source}: {len(missing)} InceptionV3 variables missing, e.g. {missing[:3]}')
  out = {}
  for k, shape in shapes.items():
    a = np.asarray(weights[k])
    if tuple(a.shape) != shape:
      raise ValueError(f'{source}: {k} has shape {tuple(a.shape)}, InceptionV3 needs {shape}')
    out[k] = a.astype(np.float32)
  return out


def _latest_prefix(directory):
  """tf.train.latest_checkpoint: the `model_checkpoint_path` of the directory's `checkpoint` file."""
  path = os.path.join(directory, 'checkpoint')
  if not os.path.exists(path):
    raise FileNotFoundError(f'no Inception v3 checkpoint found in {directory}')
  for line in open(path):
    key, _, val = line.partition(':')
    if key.strip() == 'model_checkpoint_path':
      p = val.strip().strip('"')
      return p if os.path.isabs(p) else os.path.join(directory, p)
  raise ValueError(f'{path} names no model_checkpoint_path')


def load_weights(checkpoint_path: str) -> Dict[str, np.ndarray]:
  """Keras-name keyed fp32 weights from an .npz, a checkpoint directory or a bundle prefix."""
  if checkpoint_path.endswith('.npz'):
    with np.load(checkpoint_path) as z:
      return _checked({k: z[k] for k in z.files}, checkpoint_path)
  prefix = (_latest_prefix(checkpoint_path) if os.path.isdir(checkpoint_path) else checkpoint_path)
  keys = bundle_keys()
  raw = tf_bundle.read_bundle(prefix, keys=list(keys.values()))
  return _checked({k: raw[v] for k, v in keys.items() if v in raw}, prefix)


# ------------------------------------------------------------------------------ device network
def _L():
  return _lib.lib()


def _chk(rc, what):
  _lib.check(rc, what)


class _MaxPool:
  """A pending 3x3/s2 max pool (written straight into a concatenation's channel slice)."""

  def __init__(self, x):
    n, h, w, c = x.shape
    self.x, self.shape = x, (n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c)
    self.dense = None


class _Cat:
  """A pending channel concatenation (nested ones are flattened: one copy per part)."""

  def __init__(self, parts):
    self.parts = []
    for p in parts:
      self.parts += p.parts if isinstance(p, _Cat) else [p]
    self.shape = tuple(parts[0].shape[:3]) + (sum(p.shape[3] for p in self.parts),)
    self.dense = None


class _Device:
  def __init__(self, model):
    self.m = model
    self.i = 0

  def _dense(self, x):
    if isinstance(x, torch.Tensor):
      return x
    if x.dense is not None:   # (a block's input is read by every branch: built once)
      return x.dense
    y = torch.empty(x.shape, dtype=self.m.dtype, device=self.m.device)
    parts = x.parts if isinstance(x, _Cat) else [x]
    c0 = 0
    for p in parts:
      self._write(p, y, c0)
      c0 += p.shape[3]
    x.dense = y
    return y

  def _write(self, p, y, c0):
    ctot = y.shape[3]
    if isinstance(p, _MaxPool):
      n, h, w, c = p.x.shape
      _chk(_L().se3ds_inception_maxpool3s2(p.x.data_ptr(), self.m.code, n, h, w, c, y.data_ptr(),
                                           ctot, c0, _lib.stream()), 'se3ds_inception_maxpool3s2')
    else:
      c = p.shape[3]
      _chk(_L().se3ds_copy_channels(p.data_ptr(), self.m.code, c, 0, y.data_ptr(), self.m.code, ctot,
                                    c0, c, p.numel() // c, _lib.stream()), 'se3ds_copy_channels')

  def conv_bn(self, x, cout, kh, kw, stride=1, padding='same'):
    x = self._dense(x)
    n, h, w, cin = x.shape
    wt, bias = self.m._conv_operands(self.i)
    self.i += 1
    if padding == 'valid':
      ho, wo, pt, pl = (h - kh) // stride + 1, (w - kw) // stride + 1, 0, 0
    else:
      assert stride == 1
      ho, wo, pt, pl = h, w, (kh - 1) // 2, (kw - 1) // 2
    y = torch.empty((n, ho, wo, cout), dtype=self.m.dtype, device=self.m.device)
    _chk(_L().se3ds_conv2d_fwd(x.data_ptr(), wt.data_ptr(), y.data_ptr(), self.m.code, n, h, w, cin, ho,
                               wo, cout, kh, kw, stride, pt, pl, 0, None, 0, None, bias.data_ptr(),
                               None, None, _RELU, 0.0, _lib.stream()), 'se3ds_conv2d_fwd')
    return y

  def maxpool(self, x):
    return _MaxPool(self._dense(x))

  def avgpool(self, x):
    x = self._dense(x)
    n, h, w, c = x.shape
    y = torch.empty_like(x)
    _chk(_L().se3ds_inception_avgpool3s1(x.data_ptr(), self.m.code, n, h, w, c, y.data_ptr(), c, 0,
                                         _lib.stream()), 'se3ds_inception_avgpool3s1')
    return y

  def concat(self, parts):
    return _Cat(parts)

  def head(self, x):
    x = self._dense(x)
    n, h, w, c = x.shape
    pools = torch.empty((n, c), dtype=torch.float32, device=self.m.device)
    _chk(_L().se3ds_global_avg_pool(x.data_ptr(), self.m.code, n, h * w, c, pools.data_ptr(),
                                    _lib.stream()), 'se3ds_global_avg_pool')
    xin = pools
    if self.m.dtype != torch.float32:
      xin = torch.empty((n, c), dtype=self.m.dtype, device=self.m.device)
      _chk(_L().se3ds_copy_channels(pools.data_ptr(), _lib.F32, c, 0, xin.data_ptr(), self.m.code, c, 0,
                                    c, n, _lib.stream()), 'se3ds_copy_channels')
    wt, bias = self.m._dense_operands()
    logits = torch.empty((n, NUM_CLASSES), dtype=self.m.dtype, device=self.m.device)
    _chk(_L().se3ds_conv2d_fwd(xin.data_ptr(), wt.data_ptr(), logits.data_ptr(), self.m.code, n, 1, 1,
                               c, 1, 1, NUM_CLASSES, 1, 1, 1, 0, 0, 0, None, 0, None, bias.data_ptr(),
                               None, None, 0, 0.0, _lib.stream()), 'se3ds_conv2d_fwd')
    preds = torch.empty((n, NUM_CLASSES), dtype=torch.float32, device=self.m.device)
    _chk(_L().se3ds_softmax_rows(logits.data_ptr(), self.m.code, n, NUM_CLASSES, preds.data_ptr(),
                                 _lib.stream()), 'se3ds_softmax_rows')
    return pools, preds


def fold_batch_norm(weights: Dict[str, np.ndarray]) -> List[tuple]:
  """[(kernel HWIO fp32, bias fp32)] per conv2d_bn: w * rsqrt(var + eps), beta - mean * rsqrt(...)
  (evaluated in binary64, rounded once)."""
  out = []
  for i in range(len(conv_specs())):
    k = weights[_name('conv2d', i) + '/kernel'].astype(np.float64)
    bn = _name('batch_normalization', i)
    r = 1.0 / np.sqrt(weights[bn + '/moving_variance'].astype(np.float64) + BN_EPS)
    b = weights[bn + '/beta'].astype(np.float64) - weights[bn + '/moving_mean'].astype(np.float64) * r
    out.append(((k * r).astype(np.float32), b.astype(np.float32)))
  return out


class InceptionV3:
  """Keras InceptionV3(include_top=True) inference on libse3ds_hip.so.  __call__(images (N,299,299,3)
  in [-1, 1], fp32 or the model dtype) -> (pools (N,2048) fp32, preds (N,1000) fp32 softmax)."""

  def __init__(self, weights: Dict[str, np.ndarray], device='cuda', dtype=torch.float32,
               max_batch: int = 64):
    if dtype not in (torch.float32, torch.bfloat16):
      raise ValueError(f'InceptionV3 runs in fp32 or bf16, not {dtype}')
    self.weights = _checked(weights, 'weights')
    self.device, self.dtype, self.max_batch = torch.device(device), dtype, max_batch
    self.code = _lib.BF16 if dtype == torch.bfloat16 else _lib.F32
    self.specs = conv_specs()
    self._folded = [(torch.from_numpy(k).to(self.device), torch.from_numpy(b).to(self.device))
                    for k, b in fold_batch_norm(self.weights)]
    self._dense = (torch.from_numpy(self.weights['predictions/kernel']).to(self.device),
                   torch.from_numpy(self.weights['predictions/bias']).to(self.device))
    self._ops = {}

  def count_params(self):
    """(total, non-trainable) as Keras counts them (the BN moving statistics are non-trainable)."""
    total = sum(a.size for a in self.weights.values())
    frozen = sum(a.size for k, a in self.weights.items() if '/moving_' in k)
    return total, frozen

  def _prep(self, w):
    kh, kw, cin, cout = w.shape
    K = kh * kw * cin
    wt = torch.empty((cout, K), dtype=self.dtype, device=self.device)
    _chk(_L().se3ds_weight_prep(w.data_ptr(), K, cout, self.code, wt.data_ptr(), None, _lib.stream()),
         'se3ds_weight_prep')
    return wt

  def _conv_operands(self, i):
    if i not in self._ops:
      self._ops[i] = (self._prep(self._folded[i][0]), self._folded[i][1])
    return self._ops[i]

  def _dense_operands(self):
    if 'dense' not in self._ops:
      self._ops['dense'] = (self._prep(self._dense[0].view(1, 1, POOL_DIM, NUM_CLASSES)), self._dense[1])
    return self._ops['dense']

  def __call__(self, images: torch.Tensor):
    _lib.require_cuda(images)
    if tuple(images.shape[1:]) != (INPUT_SIZE, INPUT_SIZE, 3):
      raise ValueError(f'InceptionV3 takes (N,{INPUT_SIZE},{INPUT_SIZE},3), got {tuple(images.shape)}')
    images = images.to(self.dtype).contiguous()
    pools, preds = [], []
    for b0 in range(0, images.shape[0], self.max_batch):
      p, q = _architecture(_Device(self), images[b0:b0 + self.max_batch])
      pools.append(p)
      preds.append(q)
    if len(pools) == 1:
      return pools[0], preds[0]
    return torch.cat(pools), torch.cat(preds)


@gin.configurable
def inception_model(version: str = 'V3', checkpoint_path: Optional[str] = None,
                    init: Optional[str] = None, seed: int = 0, dtype=torch.float32, device='cuda'):
  """Inception model loading function (reference inception_utils.inception_model).  Weights from
  `checkpoint_path` (a tf.train.Checkpoint(inception_v3=...) directory, a bundle prefix or an .npz),
  or init='random' for deterministic random weights (tests, benchmarks)."""
  if version != 'V3':
    raise ValueError(f'{version} is not valid input.')
  if init == 'random':
    weights = random_weights(seed)
  elif init is not None:
    raise ValueError(f'unknown init {init!r}')
  elif checkpoint_path is None:
    raise ValueError('inception_model needs checkpoint_path: the ImageNet InceptionV3 weights are not '
                     'downloaded here.  Convert them once to a tf.train.Checkpoint(inception_v3=model) '
                     'directory or a Keras-name keyed .npz and pass its path.')
  else:
    weights = load_weights(checkpoint_path)
  return InceptionV3(weights, device=device, dtype=dtype)


def preprocess(frames: torch.Tensor, roll_flip: Optional[np.ndarray] = None, crop: bool = True,
               re_normalize: bool = True, dtype=torch.float32) -> torch.Tensor:
  """(N,H,W,3) fp32 in [0,1] -> (N,299,299,3) network input in one kernel: augment roll / flip
  (roll_flip (N,2) int (roll, flip) per image, or None), crop_pano(resize_to_original=False) (crop),
  bilinear resize and clip(x*2-1, -1, 1)."""
  _lib.require_cuda(frames)
  if not re_normalize:
    raise NotImplementedError('the fused preprocess always renormalises to [-1, 1]')
  frames = frames.to(torch.float32).contiguous()
  n, h, w, c = frames.shape
  if c != 3:
    raise ValueError(f'expected RGB frames, got {c} channels')
  rf = None
  if roll_flip is not None:
    rf = torch.from_numpy(np.asarray(roll_flip, np.int32).reshape(n, 2)).to(frames.device)
  out = torch.empty((n, INPUT_SIZE, INPUT_SIZE, 3), dtype=dtype, device=frames.device)
  crop_rows = int(h * 0.125) if crop else 0
  _chk(_L().se3ds_inception_preprocess(frames.data_ptr(), n, h, w, _lib.ptr(rf), crop_rows, INPUT_SIZE,
                                       INPUT_SIZE, out.data_ptr(), _lib.dtype_code(out), _lib.stream()),
       'se3ds_inception_preprocess')
  return out


def get_inception(image: torch.Tensor, model: InceptionV3, resize_mode: str = 'bilinear',
                  re_normalize: bool = True):
  """Returns Inception model pools and predictions (reference get_inception): images not 299 x 299
  are resized (bilinear, half-pixel centres); re_normalize maps [0, 1] to clip(x*2-1, -1, 1).
  Only resize_mode='bilinear' is implemented."""
  if resize_mode != 'bilinear':
    raise NotImplementedError(f'resize_mode {resize_mode!r} (bilinear only)')
  if re_normalize:
    x = preprocess(image, crop=False, dtype=model.dtype)
  else:
    x = pano_utils.resize(image.to(torch.float32), INPUT_SIZE, INPUT_SIZE, 'bilinear')
  return model(x)


# ------------------------------------------------------------------------------ statistics
def _calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
  """d^2 = ||mu_1 - mu_2||^2 + Tr(C_1 + C_2 - 2*sqrt(C_1*C_2)) (reference semantics)."""
  mu1 = np.atleast_1d(mu1)
  mu2 = np.atleast_1d(mu2)
  sigma1 = np.atleast_2d(sigma1)
  sigma2 = np.atleast_2d(sigma2)
  if mu1.shape != mu2.shape:
    raise ShapeNotMatchError('Training and test mean vectors have different lengths')
  if sigma1.shape != sigma2.shape:
    raise ShapeNotMatchError('Training and test covariances have different dimensions')
  diff = mu1 - mu2
  # product might be almost singular
  covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
  if not np.isfinite(covmean).all():
    msg = ('fid calculation produces singular product; adding %s to diagonal of'
           ' cov estimates') % eps
    warnings.warn(msg)
    offset = np.eye(sigma1.shape[0]) * eps
    covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
  # numerical error might give slight imaginary component
  if np.iscomplexobj(covmean):
    if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
      m = np.max(np.abs(covmean.imag))
      raise ImaginaryComponentError('Imaginary component {}'.format(m))
    covmean = covmean.real
  tr_covmean = np.trace(covmean)
  return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


def calculate_fid(pool1, pool2):
  """NumPy FID of two (N, D) pools (reference calculate_fid)."""
  mu1 = np.mean(pool1, axis=0)
  mu2 = np.mean(pool2, axis=0)
  sigma1 = np.cov(pool1, rowvar=False)
  sigma2 = np.cov(pool2, rowvar=False)
  return _calculate_frechet_distance(mu1, sigma1, mu2, sigma2)


def calculate_inception_score(pred, num_splits=10):
  """(mean, std) of exp(E KL(p(y|x) || p(y))) over `num_splits` chunks (reference semantics)."""
  scores = []
  for index in range(num_splits):
    pred_chunk = pred[index * (pred.shape[0] // num_splits):(index + 1) * (pred.shape[0] // num_splits), :]
    kl_inception = pred_chunk * (np.log(pred_chunk) - np.log(np.expand_dims(np.mean(pred_chunk, 0), 0)))
    kl_inception = np.mean(np.sum(kl_inception, 1))
    scores.append(np.exp(kl_inception))
  return np.mean(scores), np.std(scores)

# ------------------------------------------------------------------------------ device Frechet distance
SQRT_CONVERGED, SQRT_CAP_REACHED, SQRT_NONFINITE = (
    _lib.ABI['SE3DS_SQRT_CONVERGED'], _lib.ABI['SE3DS_SQRT_CAP_REACHED'], _lib.ABI['SE3DS_SQRT_NONFINITE'])
FRECHET_METHODS = ('host', 'device')


class SqrtTrace(NamedTuple):
  root: Optional[torch.Tensor]   # sqrt(A) on the device, or None
  trace: float                   # tr sqrt(A)
  iterations: int
  status: int                    # SQRT_CONVERGED / SQRT_CAP_REACHED / SQRT_NONFINITE
  norm: float                    # ||A||_F


class FrechetResult(NamedTuple):
  value: float
  iterations: Tuple[int, int]    # of sqrt(sigma1) (0 when root1 was passed) and of sqrt(R sigma2 R)
  converged: bool


def _square_f64(name, *mats):
  _lib.require_cuda(*mats)
  n = mats[0].shape[-1]
  for m in mats:
    if m.dtype != torch.float64 or m.dim() != 2 or tuple(m.shape) != (n, n):
      raise ValueError(f'{name}: expected binary64 ({n}, {n}) matrices, got {m.dtype} {tuple(m.shape)}')
  return n


def f64_gemm(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0, diag: float = 0.0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
  """alpha * a @ b + diag * I of square binary64 device matrices (se3ds_f64_gemm)."""
  n = _square_f64('f64_gemm', a, b)
  a, b = a.contiguous(), b.contiguous()
  if out is None:
    out = torch.empty((n, n), dtype=torch.float64, device=a.device)
  _chk(_L().se3ds_f64_gemm(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, alpha, diag, _lib.stream()),
       'se3ds_f64_gemm')
  return out


def _queue_sqrt_trace(a, max_iters, tol, root, result):
  """Queues se3ds_sqrt_trace of `a` (contiguous); nothing is read back."""
  n = a.shape[0]
  nbytes = _L().se3ds_sqrt_trace_workspace_bytes(n)
  ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
  _chk(_L().se3ds_sqrt_trace(a.data_ptr(), n, max_iters, tol, _lib.ptr(root), ws.data_ptr(), nbytes,
                             result.data_ptr(), _lib.stream()), 'se3ds_sqrt_trace')


def sqrt_trace_device(a: torch.Tensor, max_iters: int = 48, tol: float = 1e-10,
                      want_root: bool = True) -> SqrtTrace:
  """tr sqrt(a), and sqrt(a), of a symmetric PSD binary64 device matrix by the coupled Newton-Schulz
  iteration (se3ds_sqrt_trace): the whole iteration is queued, then one 4-number block is read."""
  n = _square_f64('sqrt_trace_device', a)
  a = a.contiguous()
  root = torch.empty((n, n), dtype=torch.float64, device=a.device) if want_root else None
  result = torch.empty(4, dtype=torch.float64, device=a.device)
  _queue_sqrt_trace(a, max_iters, tol, root, result)
  r = result.cpu().tolist()
  return SqrtTrace(root, r[0], int(r[1]), int(r[2]), r[3])


def frechet_distance_device(mu1: torch.Tensor, sigma1: torch.Tensor, mu2: torch.Tensor,
                            sigma2: torch.Tensor, root1: Optional[torch.Tensor] = None,
                            max_iters: int = 48, tol: float = 1e-10) -> FrechetResult:
  """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(R S2 R), R = sqrt(S1), of binary64 device statistics.
  For symmetric PSD covariances tr sqrt(S1 S2) = tr sqrt(R S2 R), so both roots are of symmetric PSD
  matrices.  root1 = sqrt(sigma1) is computed unless passed (FeatureMoments.sqrt_cov_device caches
  it).  Everything is queued on the current stream; one block of 11 numbers is read at the end.
  converged: both roots met the stop rule and the value is finite."""
  _lib.require_cuda(mu1, mu2)
  n = _square_f64('frechet_distance_device', sigma1, sigma2, *([] if root1 is None else [root1]))
  for m in (mu1, mu2):
    if m.dtype != torch.float64 or tuple(m.shape) != (n,):
      raise ValueError(f'expected binary64 ({n},) means, got {m.dtype} {tuple(m.shape)}')
  mu1, mu2, sigma1, sigma2 = (t.contiguous() for t in (mu1, mu2, sigma1, sigma2))
  res = torch.zeros(12, dtype=torch.float64, device=sigma1.device)
  if root1 is None:
    root1 = torch.empty((n, n), dtype=torch.float64, device=sigma1.device)
    _queue_sqrt_trace(sigma1, max_iters, tol, root1, res[0:4])
  else:
    root1 = root1.contiguous()
  m = f64_gemm(f64_gemm(root1, sigma2), root1)
  _queue_sqrt_trace(m, max_iters, tol, None, res[4:8])
  _chk(_L().se3ds_frechet_terms(mu1.data_ptr(), mu2.data_ptr(), sigma1.data_ptr(), sigma2.data_ptr(), n,
                                res[8:11].data_ptr(), _lib.stream()), 'se3ds_frechet_terms')
  r = res.cpu().tolist()
  value = r[8] + r[9] + r[10] - 2 * r[4]
  ok = int(r[2]) == SQRT_CONVERGED and int(r[6]) == SQRT_CONVERGED and bool(np.isfinite(value))
  return FrechetResult(value, (int(r[1]), int(r[5])), ok)


class FeatureMoments:
  """Running count, sum and Gram matrix of (B, dim) fp32 feature rows, accumulated in binary64 on
  the device (se3ds_feature_moments_accumulate: fixed order, bit-reproducible).  The statistics are
  additive: merge() folds in another accumulator (another rank's, another shard's) on the host."""

  def __init__(self, dim: int = POOL_DIM, device='cuda'):
    self.dim, self.device = dim, torch.device(device)
    self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
    self._sum = torch.zeros(dim, dtype=torch.float64, device=self.device)
    self._gram = torch.zeros((dim, dim), dtype=torch.float64, device=self.device)
    self._extra = None   # merged host-side (count, sum, full gram)
    self._root = None    # cached (mean, cov, sqrt(cov), iterations, status) on the device

  def update(self, pools: torch.Tensor):
    _lib.require_cuda(pools)
    self._root = None
    if pools.dim() != 2 or pools.shape[1] != self.dim or pools.dtype != torch.float32:
      raise ValueError(f'expected fp32 (B, {self.dim}) rows, got {pools.dtype} {tuple(pools.shape)}')
    pools = pools.contiguous()
    _chk(_L().se3ds_feature_moments_accumulate(pools.data_ptr(), pools.shape[0], self.dim,
                                               self._count.data_ptr(), self._sum.data_ptr(),
                                               self._gram.data_ptr(), _lib.stream()),
         'se3ds_feature_moments_accumulate')
    return self

  def state(self):
    """(count, sum (dim,), gram (dim, dim) symmetric) in binary64 on the host."""
    g = self._gram.cpu().numpy()
    g = np.triu(g) + np.triu(g, 1).T
    n, s = int(self._count.cpu()[0]), self._sum.cpu().numpy()
    if self._extra is not None:
      n, s, g = n + self._extra[0], s + self._extra[1], g + self._extra[2]
    return n, s, g

  def merge(self, other: 'FeatureMoments'):
    n, s, g = other.state()
    self._root = None
    if self._extra is None:
      self._extra = (n, s, g)
    else:
      self._extra = (self._extra[0] + n, self._extra[1] + s, self._extra[2] + g)
    return self

  @property
  def count(self):
    n = int(self._count.cpu()[0])
    return n + (self._extra[0] if self._extra is not None else 0)

  def mean_cov(self):
    """(mean, np.cov(rows, rowvar=False) with ddof 1) from one download of the moments."""
    n, s, g = self.state()
    if n < 2:
      raise ValueError('a covariance needs at least two rows')
    return s / n, (g - np.outer(s, s) / n) / (n - 1)

  def mean(self):
    n, s, _ = self.state()
    return s / n

  def cov(self):
    return self.mean_cov()[1]

  def mean_cov_device(self):
    """(mean (dim,), cov (dim, dim) full symmetric) as binary64 device tensors, the formula of
    mean_cov() evaluated by se3ds_moments_mean_cov from the device moments: no download.  An
    accumulator that merged host-side state uploads its merged state() first."""
    if self.count < 2:
      raise ValueError('a covariance needs at least two rows')
    count, total, gram = self._count, self._sum, self._gram
    if self._extra is not None:
      n, s, g = self.state()
      count = torch.tensor([n], dtype=torch.int64, device=self.device)
      total, gram = torch.from_numpy(s).to(self.device), torch.from_numpy(g).to(self.device)
    mean = torch.empty(self.dim, dtype=torch.float64, device=self.device)
    cov = torch.empty((self.dim, self.dim), dtype=torch.float64, device=self.device)
    _chk(_L().se3ds_moments_mean_cov(count.data_ptr(), total.data_ptr(), gram.data_ptr(), self.dim,
                                     mean.data_ptr(), cov.data_ptr(), _lib.stream()),
         'se3ds_moments_mean_cov')
    return mean, cov

  def _root_device(self, max_iters, tol):
    if self._root is None or self._root[5:] != (max_iters, tol):
      mean, cov = self.mean_cov_device()
      r = sqrt_trace_device(cov, max_iters, tol)
      self._root = (mean, cov, r.root, r.iterations, r.status, max_iters, tol)
    return self._root

  def sqrt_cov_device(self, max_iters: int = 48, tol: float = 1e-10) -> torch.Tensor:
    """sqrt(cov) on the device (sqrt_trace_device), cached until the next update() / merge()."""
    return self._root_device(max_iters, tol)[2]

  def fid(self, other: 'FeatureMoments', method: str = 'host', max_iters: int = 48,
          tol: float = 1e-10):
    """The Frechet distance to `other`.  method='host': NumPy / SciPy on the downloaded moments
    (the reference's sqrtm formulation).  method='device': frechet_distance_device with this
    accumulator's cached root; if that does not converge or is not finite, a warning and the host
    value."""
    if method not in FRECHET_METHODS:
      raise ValueError(f'unknown Frechet method {method!r}: one of {FRECHET_METHODS}')
    if method == 'device':
      mu1, sigma1, root1, _, status, _, _ = self._root_device(max_iters, tol)
      mu2, sigma2 = other.mean_cov_device()
      r = frechet_distance_device(mu1, sigma1, mu2, sigma2, root1=root1, max_iters=max_iters, tol=tol)
      if r.converged and status == SQRT_CONVERGED:
        return r.value
      warnings.warn(f'device Frechet distance did not converge (root status {status}, iterations '
                    f'{r.iterations}, value {r.value}); using the host path')
    mu1, sigma1 = self.mean_cov()
    mu2, sigma2 = other.mean_cov()
    return _calculate_frechet_distance(mu1, sigma1, mu2, sigma2)
