"""Integer-lattice references for the convolution family (no GPU needed).

If activations, weights and incoming gradients are drawn from {-1, 0, 1}, every product is exact in
bf16 and in fp32 and every partial sum is an integer below 2^24 as long as the reduction is shorter
than 2^24 terms.  An fp32 accumulator is then exact in ANY summation order, tiling, split or MFMA
shape: each output element has exactly one legal bit pattern and a kernel is compared with `==`.
One dropped, duplicated or misplaced term is an integer error of at least 1 at known coordinates.

The epilogue slots stay on the lattice too: `scale`, `row_a` from {0.5, 1, 2}, `row_b` / masks
from {0, 1}, integer biases in [-3, 3], integer prior gradients in [-8, 8], LeakyReLU slopes that
are powers of two.  The same argument makes torch's fp32 CPU convolution an exact reference; every
reference below asserts the preconditions it rests on.

bf16-stored outputs: the expected value is the exact fp32 result rounded once to nearest-even.
Where bf16 spacing exceeds the error quantum (|value| >= 256 quanta) a unit error can round away;
`assert_visible` bounds the share of such elements at 10 % from the reference alone.
"""
import numpy as np
import torch
import torch.nn.functional as F

LIMIT = 1 << 24          # integers below this are exact in fp32
MAX_INVISIBLE = 0.10     # allowed share of bf16 elements whose spacing exceeds one error quantum


# ---------------------------------------------------------------------------------------------
# generators (all values exact in bf16)

def _gen(seed):
  return torch.Generator().manual_seed(int(seed) & 0x7fffffff)


def ternary(shape, seed):
  """fp32 tensor of {-1, 0, 1}, each with probability 1/3."""
  return (torch.randint(0, 3, tuple(shape), generator=_gen(seed)) - 1).float()


def integers(shape, seed, lo, hi):
  """fp32 tensor of integers in [lo, hi]."""
  return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).float()


def choice(shape, seed, values):
  v = torch.tensor(values, dtype=torch.float32)
  return v[torch.randint(0, len(values), tuple(shape), generator=_gen(seed))]


def bias_ints(c, seed):
  return integers((c,), seed, -3, 3)


def pow2_scale(seed):
  """The 1/sigma slot: one device scalar from {0.5, 1, 2}."""
  return choice((1,), seed, (0.5, 1.0, 2.0))


def pow2_rows(rows, seed):
  return choice((rows,), seed, (0.5, 1.0, 2.0))


def binary_rows(rows, seed):
  return choice((rows,), seed, (0.0, 1.0))


def binary_mask(n, h, w, seed, band=True):
  """(n, h, w) mask of {0, 1} with random holes, a fully masked band of rows and a hole-free
  region (the shape of the projection masks: indoor_datasets.py:281-304)."""
  m = (torch.rand((n, h, w), generator=_gen(seed)) > 0.3).float()
  if band:
    m[:, :, :max(1, w // 4)] = 1
    m[:, h // 3:h // 3 + max(1, h // 8)] = 0
  return m


def prior_grad(shape, seed):
  """Prior gradients of the _acc / accumulate entry points: integers in [-8, 8]."""
  return integers(shape, seed, -8, 8)


# ---------------------------------------------------------------------------------------------
# preconditions

def assert_on_lattice(t, name, quantum=1.0, bound=None):
  """Every value of t is an integer multiple of `quantum` (a power of two), |t| <= bound."""
  t = torch.as_tensor(t, dtype=torch.float32)
  q = t / quantum
  assert bool(torch.all(q == torch.round(q))), f'{name}: not on the lattice of {quantum}'
  if bound is not None:
    assert float(t.abs().max()) <= bound, f'{name}: |value| > {bound}'
  r = t.bfloat16().float()
  assert bool(torch.all(r == t)), f'{name}: not exact in bf16'


def assert_ternary(t, name):
  assert_on_lattice(t, name, 1.0, 1.0)


def assert_pow2(v, name):
  v = float(v)
  m, _ = np.frexp(abs(v))
  assert v != 0 and m == 0.5, f'{name} = {v}: not a power of two'


def assert_reduction(length, name):
  assert 0 < int(length) < LIMIT, f'{name} = {length}: partial sums may leave the exact range'


def assert_exact_range(t, name, quantum=1.0):
  """fp32-stored results: every value (in quanta) is an integer below 2^24 -- full visibility."""
  m = float(torch.as_tensor(t).abs().max()) / quantum if torch.as_tensor(t).numel() else 0.0
  assert m < LIMIT, f'{name}: max |exact| = {m} quanta >= 2^24'


def rne_bf16(t):
  """Exact fp32 value -> the one legal bf16 value (round to nearest even), as fp32."""
  return t.float().bfloat16().float()


def invisible_share(exact, quantum=1.0):
  """Share of elements whose magnitude is >= 256 quanta: bf16 spacing there exceeds one quantum,
  so a unit error may round away.  `quantum` broadcasts against `exact` (per-row epilogue
  multipliers); elements whose quantum is 0 (rows multiplied by 0) are dead by definition of the
  operation and count as visible."""
  e = torch.as_tensor(exact, dtype=torch.float32).abs()
  q = torch.as_tensor(quantum, dtype=torch.float32).abs()
  q = torch.broadcast_to(q, e.shape) if q.dim() else q.expand(e.shape)
  bad = (e >= 256.0 * q) & (q > 0)
  return float(bad.float().mean()) if e.numel() else 0.0


def assert_visible(exact, name, quantum=1.0):
  s = invisible_share(exact, quantum)
  assert s <= MAX_INVISIBLE, f'{name}: {100 * s:.2f} % of elements have |value| >= 256 quanta'
  return s


# ---------------------------------------------------------------------------------------------
# geometry

def _pads(size, out, k, stride, pad_lo):
  """Explicit low padding, high padding follows from the output size (may be negative: the
  trailing input rows are never read)."""
  return pad_lo, (out - 1) * stride + k - pad_lo - size


def out_size(size, k, stride, padding, pad=0):
  """(output size, low padding) of a conv on `size` + 2 * pad explicit zero rows (the PadLayer in
  front of a VALID conv) or with TF 'SAME'."""
  if padding.upper() == 'SAME':
    o = -(-size // stride)
    total = max((o - 1) * stride + k - size, 0)
    return o, total // 2
  return (size + 2 * pad - k) // stride + 1, pad


def _pad_input(xn, ho, wo, kh, kw, stride, pad_t, pad_l, wrap_w):
  """xn: NCHW.  Zero padding top / left as given, bottom / right as the output size asks;
  wrap_w: the columns are taken circularly instead."""
  n, c, h, w = xn.shape
  pt, pb = _pads(h, ho, kh, stride, pad_t)
  pl, pr = _pads(w, wo, kw, stride, pad_l)
  if wrap_w:
    idx = (torch.arange(-pl, w + max(pr, 0)) % w)
    xn = xn[:, :, :, idx]
    if pr < 0:
      xn = xn[:, :, :, :xn.shape[3] + pr]
  else:
    xn = F.pad(xn, (pl, max(pr, 0), 0, 0))
    if pr < 0:
      xn = xn[:, :, :, :xn.shape[3] + pr]
  xn = F.pad(xn, (0, 0, pt, max(pb, 0)))
  if pb < 0:
    xn = xn[:, :, :xn.shape[2] + pb]
  return xn


def conv_acc(x, w, ho, wo, stride=1, pad_t=0, pad_l=0, wrap_w=0, in_mask=None):
  """The accumulator of se3ds_conv2d_fwd: conv(x * in_mask, W); x NHWC, w HWIO, fp32."""
  kh, kw, cin, cout = w.shape
  assert_reduction(kh * kw * cin, 'K')
  if in_mask is not None:
    x = x * in_mask[..., None]
  xn = _pad_input(x.permute(0, 3, 1, 2), ho, wo, kh, kw, stride, pad_t, pad_l, wrap_w)
  y = F.conv2d(xn.contiguous(), w.permute(3, 2, 0, 1).contiguous(), stride=stride)
  assert y.shape[2] == ho and y.shape[3] == wo, (tuple(y.shape), ho, wo)
  return y.permute(0, 2, 3, 1).contiguous()


def act_apply(t, act, alpha):
  if act == 1:
    return torch.where(t > 0, t, torch.zeros_like(t))
  if act == 2:
    assert_pow2(alpha, 'act_alpha')
    return torch.where(t > 0, t, t * alpha)
  return t


def _check_inputs(**named):
  for name, t in named.items():
    if t is not None:
      assert_ternary(t, name)


def conv2d_fwd(x, w, ho, wo, stride=1, pad_t=0, pad_l=0, wrap_w=0, in_mask=None, scale=None,
               bias=None, row_a=None, row_b=None, act=0, alpha=0.0):
  """Exact se3ds_conv2d_fwd (include/se3ds_hip.h): returns (y, pre, quantum) in fp32 -- y the
  value before storage rounding, pre the value before the activation, quantum the per-element size
  of a unit accumulator error in `pre` (for the visibility figure)."""
  _check_inputs(x=x, w=w)
  if in_mask is not None:
    assert_on_lattice(in_mask, 'in_mask', 1.0, 1.0)
    assert bool(torch.all(in_mask >= 0))
  n = x.shape[0]
  acc = conv_acc(x, w, ho, wo, stride, pad_t, pad_l, wrap_w, in_mask)
  assert_exact_range(acc, 'accumulator')
  s = 1.0
  if scale is not None:
    s = float(scale)
    assert_pow2(s, 'scale')
  t = acc * s
  q = torch.full((n, ho, wo, 1), abs(s))
  if row_a is not None:
    assert_on_lattice(row_a, 'row_a', 0.5, 2.0)
    ra = row_a.reshape(n, ho, wo, 1)
    if bias is not None:
      assert_on_lattice(bias, 'bias', 1.0, 3.0)
      assert_on_lattice(row_b, 'row_b', 1.0, 1.0)
      rb = row_b.reshape(n, ho, wo, 1)
      t = ((t - bias) * ra + bias) * rb
      q = q * ra * rb
    else:
      t = t * ra
      q = q * ra
  elif bias is not None:
    assert_on_lattice(bias, 'bias', 1.0, 3.0)
    t = t + bias
  return act_apply(t, act, alpha), t, q


def conv2d_grads(x, w, dy, stride=1, pad_t=0, pad_l=0, wrap_w=0, in_mask=None, dy_row_scale=None,
                 need_x=True, need_w=True):
  """(d/dx, d/dW) of sum(conv(x * in_mask, W) * dy * dy_row_scale): the accumulators of
  se3ds_conv2d_dgrad (without the in_mask factor, which that entry point takes as row_a) and of
  se3ds_conv2d_wgrad.  fp32 autograd of the forward reference: integer sums, exact in any order."""
  _check_inputs(x=x, w=w, dy=dy)
  n, ho, wo, cout = dy.shape
  kh, kw, cin, _ = w.shape
  assert_reduction(kh * kw * cout, 'data-gradient K')
  assert_reduction(n * ho * wo, 'weight-gradient pixel count')
  g = dy
  if dy_row_scale is not None:
    assert_on_lattice(dy_row_scale, 'row_scale', 0.5, 2.0)
    g = dy * dy_row_scale.reshape(n, ho, wo, 1)
  xm = x if in_mask is None else x * in_mask[..., None]
  xr = xm.clone().requires_grad_(need_x)
  wr = w.clone().requires_grad_(need_w)
  y = conv_acc(xr, wr, ho, wo, stride, pad_t, pad_l, wrap_w)
  y.backward(g)
  for grad, name in ((xr.grad, 'dx accumulator'), (wr.grad, 'dW accumulator')):
    if grad is not None:
      assert_exact_range(grad, name, 0.5)
  return xr.grad, wr.grad


def conv2d_dgrad(dy, w, x_shape, stride=1, pad_t=0, pad_l=0, wrap_w=0, dy_row_scale=None,
                 scale=None, bias=None, row_a=None, act=0, alpha=0.0, addend=None):
  """Exact se3ds_conv2d_dgrad[_acc]: returns (dx, pre, quantum) like conv2d_fwd."""
  n, h, wd, cin = x_shape
  dxa, _ = conv2d_grads(torch.zeros(x_shape), w, dy, stride, pad_t, pad_l, wrap_w, None,
                        dy_row_scale, need_w=False)
  s = 1.0
  if scale is not None:
    s = float(scale)
    assert_pow2(s, 'scale')
  t = dxa * s
  q = torch.full((n, h, wd, 1), abs(s))
  if dy_row_scale is not None:
    q = q * 0.5
  if row_a is not None:
    assert_on_lattice(row_a, 'row_a', 0.5, 2.0)
    t = t * row_a.reshape(n, h, wd, 1)
    q = q * row_a.reshape(n, h, wd, 1)
  if bias is not None:
    assert_on_lattice(bias, 'bias', 1.0, 3.0)
    t = t + bias
  out = act_apply(t, act, alpha)
  if addend is not None:
    assert_on_lattice(addend, 'addend', 1.0, 8.0)
    out = out + addend
    t = t + addend
  return out, t, q


def conv2d_wgrad(x, dy, w_shape, stride=1, pad_t=0, pad_l=0, wrap_w=0, in_mask=None,
                 row_scale=None, out_scale=None, prior=None):
  """Exact se3ds_conv2d_wgrad: dW (+)= out_scale * sum_pixels (x * in_mask)^T (dy * row_scale)."""
  if in_mask is not None:
    assert_on_lattice(in_mask, 'in_mask', 1.0, 1.0)
  _, dw = conv2d_grads(x, torch.zeros(w_shape), dy, stride, pad_t, pad_l, wrap_w, in_mask,
                       row_scale, need_x=False)
  if out_scale is not None:
    assert_pow2(float(out_scale), 'out_scale')
    dw = dw * float(out_scale)
  if prior is not None:
    assert_on_lattice(prior, 'prior dW', 1.0, 8.0)
    dw = dw + prior
  assert_exact_range(dw, 'dW', 0.25)
  return dw


def conv2d_wgrad_swapped(x, dy, k, pad, prior=None):
  """se3ds_conv2d_wgrad_swapped: the weight gradient of a stride-1 same-size k x k conv."""
  n, h, w, cin = x.shape
  return conv2d_wgrad(x, dy, (k, k, cin, dy.shape[3]), 1, pad, pad, 0, prior=prior)


def conv_transpose2x2(x, kern, bias=None):
  """se3ds_conv_transpose2x2_fwd: y[n, 2i+ky, 2j+kx, co] = sum_ci x[n,i,j,ci] kern[ky,kx,co,ci]."""
  _check_inputs(x=x, kern=kern)
  n, h, w, cin = x.shape
  cout = kern.shape[2]
  assert_reduction(cin, 'K')
  y = torch.einsum('nijc,yxoc->niyjxo', x, kern).reshape(n, 2 * h, 2 * w, cout)
  if bias is not None:
    assert_on_lattice(bias, 'bias', 1.0, 3.0)
    y = y + bias
  assert_exact_range(y, 'y')
  return y


def column_stats(stored):
  """What se3ds_conv2d_fwd_stats emits once its rows are reduced: per-channel sum and sum of
  squares of the STORED output (..., c).  Asserts that both stay exact in fp32."""
  s = stored.double().reshape(-1, stored.shape[-1])
  s1, s2 = s.sum(0), (s * s).sum(0)
  assert float(s2.max()) < LIMIT and float(s1.abs().max()) < LIMIT, 'statistics leave 2^24'
  q = stored.reshape(-1) * 4
  assert bool(torch.all(q == torch.round(q))), 'stored output finer than 1/4'
  return s1.float(), s2.float()


def weight_operands(w, dtype=torch.float32):
  """se3ds_weight_prep's layouts of the HWIO kernel viewed [K][cout]: wt [cout][K], wn [K][cout]."""
  k = w.shape[0] * w.shape[1] * w.shape[2]
  wn = w.reshape(k, w.shape[3]).to(dtype).contiguous()
  return wn.t().contiguous(), wn


# ---------------------------------------------------------------------------------------------
# comparator

def _hist(values, name, top=8):
  u, c = np.unique(values, return_counts=True)
  order = np.argsort(-c)[:top]
  return f'  by {name}: ' + ', '.join(f'{int(u[i])}: {int(c[i])}' for i in order)


def mismatch_report(got, exp, layout='nhwc', cin=None, limit=10):
  """None when got == exp bit for bit (NaN never equals), else a text that locates the errors:
  count, first coordinates, got / expected, histograms by tile-relative position."""
  got = np.asarray(got, dtype=np.float32)
  exp = np.asarray(exp, dtype=np.float32)
  assert got.shape == exp.shape, (got.shape, exp.shape)
  bad = ~(got == exp)
  # -0.0 == 0.0: zeros compare equal whatever their sign (x * 0 epilogues)
  if not bad.any():
    return None
  idx = np.argwhere(bad)
  lines = [f'{len(idx)} of {got.size} elements differ ({layout})']
  names = '(n, y, x, c)' if layout == 'nhwc' else '(ky, kx, ci, co)'
  for i in idx[:limit]:
    t = tuple(int(v) for v in i)
    lines.append(f'  {names} = {t}: got {got[t]!r} expected {exp[t]!r}')
  if got.ndim == 4 and layout == 'nhwc':
    n, h, w, c = got.shape
    pix = (idx[:, 0] * h + idx[:, 1]) * w + idx[:, 2]
    lines += [_hist(idx[:, 2] % 32, 'x % 32'), _hist(idx[:, 1] % 8, 'y % 8'),
              _hist(pix % 128, 'pixel % 128'), _hist(idx[:, 3] % 64, 'c % 64'),
              _hist(idx[:, 0], 'n'), _hist(idx[:, 1], 'y'), _hist(idx[:, 2], 'x')]
  elif got.ndim == 4:
    kh, kw, ci, co = got.shape
    kidx = (idx[:, 0] * kw + idx[:, 1]) * ci + idx[:, 2]
    lines += [_hist(idx[:, 0] * kw + idx[:, 1], 'tap'), _hist(kidx // 32, 'K step of 32'),
              _hist(idx[:, 2] % 64, 'ci % 64'), _hist(idx[:, 3] % 64, 'c % 64')]
  else:
    flat = np.flatnonzero(bad.reshape(-1))
    lines += [_hist(flat % 64, 'index % 64'), _hist(flat // 64, 'index // 64')]
  d = np.abs(got.astype(np.float64) - exp.astype(np.float64))[bad]
  lines.append(f'  |got - expected|: min {np.nanmin(d) if np.isfinite(d).any() else float("nan")}, '
               f'max {np.nanmax(d) if np.isfinite(d).any() else float("nan")}, '
               f'non-finite {int((~np.isfinite(d)).sum())}')
  return '\n'.join(lines)


def assert_bit_equal(got, exp, what, layout='nhwc'):
  r = mismatch_report(got, exp, layout)
  assert r is None, f'{what}: {r}'
