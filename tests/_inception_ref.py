"""CPU restatement of Keras InceptionV3(include_top=True) and of the evaluator's input chain, for the
tests: torch fp64 on the host, written from Keras applications/inception_v3.py independently of
se3ds_amd/utils/inception_utils.py (unfolded batch norm, nested concatenations)."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3


class _Net:
  def __init__(self, weights):
    self.w = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in weights.items()}
    self.i = 0

  def cbn(self, x, cout, kh, kw, strides=1, padding='same'):
    sfx = '' if self.i == 0 else f'_{self.i}'
    self.i += 1
    k = self.w[f'conv2d{sfx}/kernel']                      # (kh, kw, cin, cout)
    assert k.shape[:2] == (kh, kw) and k.shape[3] == cout
    if padding == 'same':
      x = F.pad(x, ((kw - 1) // 2, kw // 2, (kh - 1) // 2, kh // 2))
    y = F.conv2d(x, k.permute(3, 2, 0, 1), stride=strides)
    bn = f'batch_normalization{sfx}'
    m, v, b = (self.w[f'{bn}/{n}'][None, :, None, None] for n in ('moving_mean', 'moving_variance', 'beta'))
    return torch.relu((y - m) / torch.sqrt(v + BN_EPS) + b)


def _maxpool(x):
  return F.max_pool2d(x, 3, 2)


def _avgpool(x):
  return F.avg_pool2d(x, 3, 1, padding=1, count_include_pad=False)


def inception_v3(weights, images):
  """images (N,299,299,3) in [-1,1] -> (pools (N,2048), preds (N,1000)) in fp64."""
  net = _Net(weights)
  c = net.cbn
  x = torch.from_numpy(np.asarray(images, np.float64)).permute(0, 3, 1, 2)
  x = c(x, 32, 3, 3, 2, 'valid')
  x = c(x, 32, 3, 3, 1, 'valid')
  x = c(x, 64, 3, 3)
  x = _maxpool(x)
  x = c(x, 80, 1, 1, 1, 'valid')
  x = c(x, 192, 3, 3, 1, 'valid')
  x = _maxpool(x)
  for pc in (32, 64, 64):
    b1 = c(x, 64, 1, 1)
    b5 = c(x, 48, 1, 1)
    b5 = c(b5, 64, 5, 5)
    bd = c(x, 64, 1, 1)
    bd = c(bd, 96, 3, 3)
    bd = c(bd, 96, 3, 3)
    bp = c(_avgpool(x), pc, 1, 1)
    x = torch.cat([b1, b5, bd, bp], 1)
  b3 = c(x, 384, 3, 3, 2, 'valid')
  bd = c(x, 64, 1, 1)
  bd = c(bd, 96, 3, 3)
  bd = c(bd, 96, 3, 3, 2, 'valid')
  x = torch.cat([b3, bd, _maxpool(x)], 1)
  for c7 in (128, 160, 160, 192):
    b1 = c(x, 192, 1, 1)
    b7 = c(x, c7, 1, 1)
    b7 = c(b7, c7, 1, 7)
    b7 = c(b7, 192, 7, 1)
    bd = c(x, c7, 1, 1)
    bd = c(bd, c7, 7, 1)
    bd = c(bd, c7, 1, 7)
    bd = c(bd, c7, 7, 1)
    bd = c(bd, 192, 1, 7)
    bp = c(_avgpool(x), 192, 1, 1)
    x = torch.cat([b1, b7, bd, bp], 1)
  b3 = c(x, 192, 1, 1)
  b3 = c(b3, 320, 3, 3, 2, 'valid')
  b7 = c(x, 192, 1, 1)
  b7 = c(b7, 192, 1, 7)
  b7 = c(b7, 192, 7, 1)
  b7 = c(b7, 192, 3, 3, 2, 'valid')
  x = torch.cat([b3, b7, _maxpool(x)], 1)
  for _ in range(2):
    b1 = c(x, 320, 1, 1)
    b3 = c(x, 384, 1, 1)
    b3 = torch.cat([c(b3, 384, 1, 3), c(b3, 384, 3, 1)], 1)
    bd = c(x, 448, 1, 1)
    bd = c(bd, 384, 3, 3)
    bd = torch.cat([c(bd, 384, 1, 3), c(bd, 384, 3, 1)], 1)
    bp = c(_avgpool(x), 192, 1, 1)
    x = torch.cat([b1, b3, bd, bp], 1)
  assert net.i == 94 and x.shape[1:] == (2048, 8, 8)
  pools = x.mean((2, 3))
  logits = pools @ net.w['predictions/kernel'] + net.w['predictions/bias']
  return pools.numpy(), torch.softmax(logits, 1).numpy()


def preprocess_np(frames, roll_flip, out=299):
  """NumPy statement of augment (tf.roll + flip) -> crop_pano -> tf.image.resize bilinear
  (half-pixel centres) -> clip(x*2-1, -1, 1), fp32 frames (N,H,W,3), in fp32."""
  frames = np.asarray(frames, np.float32)
  n, h, w, _ = frames.shape
  res = np.empty((n, out, out, 3), np.float32)
  for b in range(n):
    x = frames[b]
    if roll_flip is not None:
      x = np.roll(x, int(roll_flip[b][0]), axis=1)
      if roll_flip[b][1]:
        x = x[:, ::-1]
    mh = int(h * 0.125)
    x = x[mh:h - mh]
    ch = x.shape[0]
    # source coordinates in fp32, one rounding per op, as TF's half-pixel resize computes them
    f32 = np.float32
    o = np.arange(out, dtype=f32)
    fy = (o + f32(0.5)) * (f32(ch) / f32(out)) - f32(0.5)
    fx = (o + f32(0.5)) * (f32(w) / f32(out)) - f32(0.5)
    y0 = np.floor(fy).astype(int)
    x0 = np.floor(fx).astype(int)
    ty, tx = (fy - y0)[:, None, None], (fx - x0)[None, :, None]
    y1, x1 = np.clip(y0 + 1, 0, ch - 1), np.clip(x0 + 1, 0, w - 1)
    y0, x0 = np.clip(y0, 0, ch - 1), np.clip(x0, 0, w - 1)
    top = x[y0][:, x0] + (x[y0][:, x1] - x[y0][:, x0]) * tx
    bot = x[y1][:, x0] + (x[y1][:, x1] - x[y1][:, x0]) * tx
    v = top + (bot - top) * ty
    res[b] = np.clip(v * f32(2) - f32(1), -1, 1)
  return res
