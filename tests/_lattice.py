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


# =============================================================================================
# Optimiser, spectral-norm and loss references (NumPy float64; se3ds_amd/csrc/optim.hip and the
# loss / head kernels of pointwise.hip).  Same idea as above: inputs sit on a lattice on which
# every sum, dot product, rank-one fix-up, count and sign gradient is exact in fp32 in ANY order,
# so each output has one legal bit pattern.  Where an operation rounds (sqrt, division) it has
# exact fp32 inputs and is correctly rounded by IEEE-754, so it still has ONE legal result; the
# reference takes it in float64 and rounds once (float64 -> fp32 after sqrt or a quotient of two
# fp32 values equals the correctly rounded fp32 operation: 53 >= 2 * 24 + 2).
# Nothing here looks at the code under test.

def rng(seed):
  return np.random.default_rng(int(seed) & 0x7fffffff)


def f32(x):
  """One rounding float64 -> fp32."""
  return np.asarray(x, dtype=np.float64).astype(np.float32)


def assert_np_lattice(a, name, quantum=1.0, bound=None):
  """NumPy twin of assert_on_lattice without the bf16 condition (fp32-stored data)."""
  assert_pow2(quantum, name + ' quantum')
  a = np.asarray(a, dtype=np.float64)
  q = a / quantum
  assert np.array_equal(q, np.round(q)), f'{name}: not on the lattice of {quantum}'
  m = float(np.abs(q).max()) if a.size else 0.0
  assert m < LIMIT, f'{name}: |value| = {m} quanta >= 2^24'
  if bound is not None:
    assert m * quantum <= bound, f'{name}: |value| > {bound}'


def assert_exact_sum(terms, name, quantum=1.0):
  """sum(terms) is exact in fp32 in any order: integer quanta, sum of magnitudes < 2^24."""
  t = np.asarray(terms, dtype=np.float64) / quantum
  assert np.array_equal(t, np.round(t)), f'{name}: terms off the lattice of {quantum}'
  assert_reduction(float(np.abs(t).sum()) + 1, name)
  return float(t.sum()) * quantum


def is_pow4(x):
  m, e = np.frexp(float(x))
  return x > 0 and m == 0.5 and (e - 1) % 2 == 0


def shuffled_f32_sum(terms, seed):
  """Sequential fp32 accumulation of the terms in a random order (the CPU pins compare it with
  the float64 sum: equal bits are the proof that the order cannot matter)."""
  t = np.asarray(terms, dtype=np.float32).reshape(-1)
  t = t[rng(seed).permutation(t.size)]
  return np.cumsum(t, dtype=np.float32)[-1] if t.size else np.float32(0)


# ------------------------------------------------------------------ squared norm and clip
def sqnorm(g, quantum=1.0):
  """sum g^2 of one tensor; asserts that an fp32 accumulator holds it exactly."""
  g = np.asarray(g, dtype=np.float64).reshape(-1)
  assert_np_lattice(g, 'g', quantum)
  return assert_exact_sum(g * g, 'sum g^2', quantum * quantum)


def pow4_gradient(n, seed, scale=1.0, zero=False):
  """Ternary gradient times a power-of-two scale whose sum of squares is scale^2 * 4^j: a few
  entries are switched on or off until the count of non-zeros is the nearest reachable power of
  four.  sqrt and the clip division are then exact whatever the device's sqrtf does."""
  assert_pow2(scale, 'scale')
  assert_reduction(n, 'n')
  r = rng(seed)
  g = r.integers(-1, 2, n).astype(np.float64)
  if zero:
    return np.zeros(n)
  nz = int(np.count_nonzero(g))
  t = 1
  while t * 4 <= max(nz, 1):
    t *= 4
  if 4 * t <= n and 4 * t - nz < nz - t:
    t *= 4
  if nz > t:
    on = np.flatnonzero(g)
    g[on[r.permutation(on.size)[:nz - t]]] = 0
  elif nz < t:
    off = np.flatnonzero(g == 0)
    pick = off[r.permutation(off.size)[:t - nz]]
    g[pick] = r.choice((-1.0, 1.0), pick.size)
  g *= scale
  assert is_pow4(sqnorm(g, scale) / (scale * scale)), 'sum g^2 is not scale^2 * 4^j'
  return g


def clip_by_norm(g, clip, sq=None):
  """tf.clip_by_norm: (g * clip) / max(sqrt(sum g^2), clip), norm 0 where the sum is 0.  Returns
  the fp32 result.  g * clip must be exact; sqrt and the quotient are rounded once each -- when
  sum g^2 is a power of four (pow4_gradient) the norm is exact and the whole result is the
  float64 value rounded once."""
  g = np.asarray(g, dtype=np.float64)
  clip = float(f32(clip))
  sq = sqnorm(g) if sq is None else float(sq)
  assert float(f32(sq)) == sq, 'sum g^2 is not an fp32 value'
  norm = float(f32(np.sqrt(sq))) if sq > 0 else 0.0
  num = g * clip
  assert np.array_equal(f32(num).astype(np.float64), num), 'g * clip rounds'
  return f32(num / max(norm, clip))


def mean_clipped_norm(sqs, clip):
  """The trainer's metric: mean over tensors of norm * clip / max(norm, clip) (0 for NaN)."""
  clip = float(f32(clip))
  terms = []
  for sq in sqs:
    norm = float(f32(np.sqrt(sq))) if sq > 0 else 0.0
    terms.append(float(f32(float(f32(norm * clip)) / max(norm, clip))))
  s = assert_exact_sum(terms, 'sum of clipped norms', 2.0 ** -6)
  out = np.float32(s) / np.float32(len(terms))
  return np.float32(0) if np.isnan(out) else out


# ------------------------------------------------------------------ spectral fix-up
def sn_case(K, C, seed, inv, dot, density=2.0 / 3.0):
  """Lattice inputs of one spectral layer: G, W ternary [K, C] (G non-zero with probability
  `density`) with <G, W> forced to `dot` by switching a few entries of W; v [K], uhat [C] sparse
  integers in [-2, 2] (three quarters zero) with non-zero end points."""
  assert dot != 0
  r = rng(seed)
  n = K * C
  G = (r.integers(-1, 2, n) * (r.random(n) < 1.5 * density)).astype(np.float64)
  if not G.any():
    G[0] = 1.0
  W = r.integers(-1, 2, n).astype(np.float64)
  for _ in range(3):
    c = G * W
    delta = int(dot - c.sum())
    if delta == 0:
      break
    cand = np.flatnonzero((G != 0) & ((c < 1) if delta > 0 else (c > -1)))
    pick = cand[r.permutation(cand.size)[:abs(delta)]]
    W[pick] += np.sign(delta) * G[pick]
  def sparse(m):
    x = (r.integers(1, 3, m) * r.choice((-1, 1), m) * (r.random(m) < 0.25)).astype(np.float64)
    x[0], x[-1] = 2.0, -1.0 if m > 1 else 2.0
    return x
  return dict(G=G.reshape(K, C), W=W.reshape(K, C), v=sparse(K), uhat=sparse(C), inv=float(inv))


def sn_fixup(G, W, v, uhat, inv):
  """Gradient through sigma = v W u^T: inv * G - inv^2 <G, W> v u^T.  Returns (fixed gradient,
  dict of the exact reductions and of the closed-form squared norm
  inv^2 <G,G> - 2 inv coef <G, v u^T> + coef^2 |v|^2 |u|^2, coef = inv^2 <G, W>)."""
  assert_pow2(inv, 'inv')
  for a, name in ((G, 'G'), (W, 'W')):
    assert_np_lattice(a, name, 1.0, 1.0)
  assert_np_lattice(v, 'v', 1.0, 2.0)
  assert_np_lattice(uhat, 'uhat', 1.0, 2.0)
  vu = np.outer(v, uhat)
  r = dict(dot=assert_exact_sum(G * W, '<G,W>'), gg=assert_exact_sum(G * G, '<G,G>'),
           gvu=assert_exact_sum(G * vu, '<G, v u^T>'), nv=assert_exact_sum(v * v, '|v|^2'),
           nu=assert_exact_sum(uhat * uhat, '|u|^2'))
  coef = inv * inv * r['dot']
  assert float(f32(coef)) == coef
  out = inv * G - coef * vu
  q = min(inv, inv * inv, 1.0)
  assert_np_lattice(out, 'fixed gradient', q)
  sq = inv * inv * r['gg'] - 2 * inv * coef * r['gvu'] + coef * coef * r['nv'] * r['nu']
  assert abs(sq) < 2.0 ** 52 and sq == float((out * out).sum()), 'closed form != sum of squares'
  r.update(coef=coef, sq=sq, quantum=q)
  return out, r


# ------------------------------------------------------------------ power iteration
SN_EPS = 1e-10


def power_iteration(W, u, dtype=np.float64):
  """oracle/nets_torch.power_iteration (models/layers.py:312-331) on W [K, C], u [C]:
  v = W u, vhat = v / (|v| + eps), u' = vhat W, uhat = u' / (|u'| + eps), sigma = u' . uhat.
  Returns dict(v=vhat, uhat, sigma, inv = 1 / (sigma + eps)).  dtype=np.float32 is the plain fp32
  restatement whose error against float64 is the measured floor of the GPU test."""
  W = np.asarray(W, dtype=dtype)
  u = np.asarray(u, dtype=dtype).reshape(-1)
  eps = dtype(SN_EPS)
  v = W @ u
  vhat = v / (np.sqrt((v * v).sum(dtype=dtype)) + eps)
  un = vhat @ W
  uhat = un / (np.sqrt((un * un).sum(dtype=dtype)) + eps)
  sigma = (un * uhat).sum(dtype=dtype)
  return dict(v=vhat, uhat=uhat, sigma=sigma, inv=dtype(1) / (sigma + eps))


def scaled_err(got, ref):
  """max |got - ref| / max |ref| in float64 (the measure of the floor-based tolerances)."""
  got = np.asarray(got, dtype=np.float64)
  ref = np.asarray(ref, dtype=np.float64)
  return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))


# ------------------------------------------------------------------ Adam (Keras form) and EMA
# fp32 roundings of each output, counted from the formulas in adam_keras / ema below, one per
# arithmetic operation (a fused multiply-add only ever removes one):
#   m': (g - m), (1 - b1), product, sum                                         -> 4
#   v': g * g, (.. - v), (1 - b2), product, sum                                 -> 5
#   p': m' (4) + v' (5) + m' * alpha, sqrt, + eps, quotient, difference         -> 14
#   e': (e - p), product, difference                                            -> 3 (+ 14 when p = p')
K_M, K_V, K_P, K_E = 4, 5, 14, 3
ULP = 2.0 ** -24


def adam_alpha(lr, b1, b2, step):
  """Keras step size lr * sqrt(1 - b2^t) / (1 - b1^t): one pow per power, taken in float64 and
  rounded to fp32, then every operation rounded to fp32."""
  lr, b1, b2 = np.float32(lr), np.float32(b1), np.float32(b2)
  b1p = np.float32(np.power(np.float64(b1), np.float64(step)))
  b2p = np.float32(np.power(np.float64(b2), np.float64(step)))
  return np.float32(np.float32(lr * np.sqrt(np.float32(np.float32(1) - b2p))) /
                    np.float32(np.float32(1) - b1p))


def adam_keras(p, g, m, v, lr, b1, b2, step, eps=1e-7, dtype=np.float64):
  """ResourceApplyAdam with the hyper-parameters as fp32 values:
      m' = m + (g - m) * (1 - b1)
      v' = v + (g * g - v) * (1 - b2)
      p' = p - (m' * alpha) / (sqrt(v') + eps),   alpha = adam_alpha(lr, b1, b2, step)
  Returns (p', m', v', mag) where mag = dict(m, v, p) holds per element the largest magnitude
  among the inputs, intermediates and result of that output's formula (in float64): the bound of
  an output is K * 2^-24 * mag.  dtype=np.float32 evaluates the same formula in plain fp32."""
  p, g, m, v = (np.asarray(a, dtype=dtype) for a in (p, g, m, v))
  one = dtype(1)
  b1, b2, eps = dtype(np.float32(b1)), dtype(np.float32(b2)), dtype(np.float32(eps))
  alpha = dtype(adam_alpha(lr, b1, b2, step))
  def mx(*a):
    out = np.zeros(p.shape)
    for x in a:
      np.maximum(out, np.abs(np.asarray(x, np.float64)), out=out)
    return out
  d1 = g - m
  t1 = d1 * (one - b1)
  m2 = m + t1
  gg = g * g
  d2 = gg - v
  t2 = d2 * (one - b2)
  v2 = v + t2
  num = m2 * alpha
  rt = np.sqrt(v2)
  den = rt + eps
  quo = num / den
  p2 = p - quo
  mag = dict(m=mx(g, m, d1, t1, m2), v=mx(gg, v, d2, t2, v2))
  mag['p'] = mx(mag['m'], mag['v'], num, rt, den, quo, p, p2)
  return p2, m2, v2, mag


def ema(e, p, omd, dtype=np.float64):
  """utils/ema.py: e' = e - (e - p) * omd with omd = fp32(1 - decay).  Returns (e', mag)."""
  e, p = np.asarray(e, dtype=dtype), np.asarray(p, dtype=dtype)
  omd = dtype(np.float32(omd))
  d = e - p
  t = d * omd
  e2 = e - t
  mag = np.zeros(e.shape)
  for a in (e, p, d, t, e2):
    np.maximum(mag, np.abs(a.astype(np.float64)), out=mag)
  return e2, mag


def bound_ratio(got, ref, k, mag):
  """max over elements of |got - ref| / (k * 2^-24 * mag): <= 1 passes."""
  err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
  lim = k * ULP * np.asarray(mag, np.float64)
  bad = (lim == 0) & (err > 0)
  assert not bad.any(), 'error where the bound is 0'
  return float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0.0))) if err.size else 0.0


# ------------------------------------------------------------------ losses and heads
DEPTH_VALUES = (0.0, 0.25, 0.5, 0.75, 1.0)          # both ends of the strict mask 0 < t < 1
COARSE_DEPTHS = (0.0, 0.5, 1.0)                      # (a - b)^2 on the lattice of 1/4
LOGIT_VALUES = (-2.0, -1.25, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0)   # bf16-exact, +-1 included


def pick(shape, seed, values):
  """Random choice of `values`; the first elements run through all of them, and (for the second
  operand of a pair drawn with seed + 1) equal values occur."""
  v = np.asarray(values, dtype=np.float64)
  a = v[rng(seed).integers(0, len(v), int(np.prod(shape)))]
  a[:min(len(v), a.size)] = v[:min(len(v), a.size)]
  return a.reshape(shape)


def hinge(logits, cd, cg):
  """logits [2 * half] = [fake | real]: sums = (sum(-fake), sum(relu(1 - real) + relu(1 + fake))),
  dlog_d = cd * d sums[1] / d logits, dlog_g = cg * d sums[0] / d logits (real half 0)."""
  x = np.asarray(logits, dtype=np.float64).reshape(-1)
  assert_np_lattice(x, 'logits', 0.25, 2.0)
  assert (x == 1).any() and (x == -1).any(), 'logits must hit +1 and -1'
  half = x.size // 2
  f, r = x[:half], x[half:]
  sums = np.array([assert_exact_sum(-f, 'sum(-fake)', 0.25),
                   assert_exact_sum(np.maximum(1 - r, 0) + np.maximum(1 + f, 0), 'disc', 0.25)])
  dd = np.concatenate([np.where(1 + f > 0, cd, 0.0), np.where(1 - r > 0, -cd, 0.0)])
  dg = np.concatenate([np.full(half, -cg), np.zeros(half)])
  return f32(sums), f32(dd), f32(dg)


SUM_QUANTUM = {0: 0.25, 1: 0.25, 2: 1.0, 3: 0.25, 4: 1.0 / 16}


def sample_sum(a, b, m, mode):
  """Per-sample sums over (p, c).  a, b [n, p, c], m [n, p] or None.  mode 0: sum(a);
  1: sum(|a - b| * m); 2: count(0 < a < 1); 3: sum(a * (1 - b)); 4: sum((a - b)^2 * 1[0 < b < 1])."""
  a = np.asarray(a, dtype=np.float64)
  n = a.shape[0]
  if mode == 0:
    t = a
  elif mode == 1:
    t = np.abs(a - b) * (1.0 if m is None else np.asarray(m, np.float64)[..., None])
  elif mode == 2:
    t = ((a > 0) & (a < 1)).astype(np.float64)
  elif mode == 3:
    t = a * (1 - np.asarray(b, np.float64))
  else:
    b = np.asarray(b, dtype=np.float64)
    t = (a - b) ** 2 * ((b > 0) & (b < 1))
  t = t.reshape(n, -1)
  return f32([assert_exact_sum(t[i], f'sample_sum mode {mode}', SUM_QUANTUM[mode]) for i in range(n)])


def l1_grad(a, b, m, m2, coef, mode):
  """coef[n] * sign(a - b) * w; w = 1[0 < b < 1] (modes 0, 2) or m * (1 - m2) (modes 1, 3);
  modes 2 and 3 return w alone, broadcast to [n, p, c]."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  if mode in (0, 2):
    w = ((b > 0) & (b < 1)).astype(np.float64)
  else:
    w = np.broadcast_to((np.asarray(m, np.float64) * (1 - np.asarray(m2, np.float64)))[..., None],
                        a.shape)
  if mode >= 2:
    return f32(w)
  for c in np.asarray(coef).reshape(-1):
    assert_pow2(c, 'coef')
  assert (a == b).any(), 'a == b (sign 0) must occur'
  return f32(np.asarray(coef, np.float64).reshape(-1, 1, 1) * np.sign(a - b) * w)


def recip_clamp(sums, scale):
  """scale / max(sums, 1): one correctly rounded division."""
  return f32(float(f32(scale)) / np.maximum(f32(sums).astype(np.float64), 1.0))


def head_fwd(x, kind, dtype=np.float64):
  """kind 0: (tanh(x) + 1) / 2; kind 1: clip(x, 0, 1) (exact)."""
  x = np.asarray(x, dtype=dtype)
  return (np.tanh(x) + dtype(1)) / dtype(2) if kind == 0 else np.clip(x, dtype(0), dtype(1))


def head_bwd(dy, y, x, kind, dtype=np.float64):
  """kind 0: dy * (1 - t^2) / 2 with t = 2 y - 1; kind 1: dy where 0 <= x <= 1 (tf.clip_by_value
  passes the gradient at both ends), else 0 (exact)."""
  dy = np.asarray(dy, dtype=dtype)
  if kind == 0:
    t = dtype(2) * np.asarray(y, dtype=dtype) - dtype(1)
    return dy * (dtype(1) - t * t) * dtype(0.5)
  x = np.asarray(x, dtype=dtype)
  return np.where((x >= 0) & (x <= 1), dy, dtype(0))


# =============================================================================================
# Norm, pooling and pad references (NumPy float64; se3ds_amd/csrc/norm.hip and the pooling / pad /
# copy kernels of pointwise.hip), written from the formulas of include/se3ds_hip.h and the TF
# semantics only.  Every stage of the norm takes the previous stage's results as ARGUMENTS, so
# each gets lattice inputs of its own: activations and gradients small integers, row factors /
# rstd / gamma / alpha signed powers of two, mean / beta / shift small integers, count a power of
# two (a free parameter: it need not equal the row count).  Every product, FMA and sum of any
# algebraic rearrangement of the documented formula is then exact in fp32 and each output has one
# legal value: the float64 result rounded once to the storage type.

def rne_np(a, bf16):
  """float64 -> the stored value: one rounding to fp32, then (bf16) one to nearest-even bf16."""
  a = f32(a)
  if bf16:
    a = torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()
  return a


def exact32(a, name):
  """Asserts that a float64 intermediate is an fp32 value (no rounding happened) and returns it."""
  a = np.asarray(a, dtype=np.float64)
  assert np.array_equal(f32(a).astype(np.float64), a), f'{name}: rounds in fp32'
  return a


def assert_all_pow2(a, name):
  m, _ = np.frexp(np.abs(np.asarray(a, dtype=np.float64)))
  assert np.all(m == 0.5), f'{name}: not signed powers of two'


def small_ints(shape, seed, lo, hi, zero_share=0.0):
  """float64 integers in [lo, hi]; a share of them forced to 0 (post-ReLU zeros, ties)."""
  r = rng(seed)
  a = r.integers(lo, hi + 1, shape).astype(np.float64)
  if zero_share:
    a[r.random(shape) < zero_share] = 0.0
  return a


def signed_pow2(shape, seed, mags=(0.5, 1.0, 2.0), signed=True):
  r = rng(seed)
  a = np.asarray(mags, dtype=np.float64)[r.integers(0, len(mags), shape)]
  return a * r.choice((-1.0, 1.0), shape) if signed else a


def assert_exact_colsum(terms, name, quantum):
  """Column sums over axis -2 that are exact in fp32 in ANY order: every term an integer multiple
  of `quantum`, the sum of magnitudes of every column below 2^24 quanta.  Returns the sums."""
  assert_pow2(quantum, name + ' quantum')
  t = np.asarray(terms, dtype=np.float64) / quantum
  assert np.array_equal(t, np.round(t)), f'{name}: terms off the lattice of {quantum}'
  assert_reduction(float(np.abs(t).sum(axis=-2).max()) + 1, name)
  return t.sum(axis=-2) * quantum


def assert_any_order(quantum, bound, name):
  """Every intermediate of any rearrangement is a multiple of `quantum` and at most `bound`."""
  assert_pow2(quantum, name + ' quantum')
  assert bound / quantum < LIMIT, f'{name}: {bound} / {quantum} >= 2^24'


def _qmin(a, cap=1.0):
  """Power-of-two quantum contributed by a factor whose values are signed powers of two."""
  a = np.abs(np.asarray(a, dtype=np.float64))
  return min(cap, float(a.min())) if a.size else cap


def act_np(t, act, alpha):
  if act == 1:
    return np.where(t > 0, t, 0.0)
  if act == 2:
    assert_pow2(alpha, 'alpha')
    return np.where(t > 0, t, t * alpha)
  return t


def act_grad_np(pos, act, alpha):
  """Derivative of the activation from `pos` = (its stored output > 0)."""
  if act == 1:
    return np.where(pos, 1.0, 0.0)
  if act == 2:
    assert_pow2(alpha, 'alpha')
    return np.where(pos, 1.0, float(alpha))
  return np.ones(np.shape(pos))


def pack_mask(y):
  """act_mask: bit e of byte i = (y[8 i + e] > 0) over the flattened stored output."""
  return np.packbits((np.asarray(y) > 0).reshape(-1, 8), axis=1, bitorder='little').reshape(-1)


def unpack_mask(bits, shape):
  return np.unpackbits(np.asarray(bits, np.uint8).reshape(-1, 1), axis=1,
                       bitorder='little').reshape(shape).astype(bool)


# ------------------------------------------------------------------ statistics
def norm_stats(x, row_scale=None):
  """sums[g][0][c] = sum_r x * row_scale, sums[g][1][c] = sum_r (x * row_scale)^2.  x [g, r, c]
  integers, row_scale [g * r] signed powers of two in [1/2, 2]."""
  x = np.asarray(x, dtype=np.float64)
  g, r, c = x.shape
  assert_np_lattice(x, 'x', 1.0, 4.0)
  q = 1.0
  v = x
  if row_scale is not None:
    assert_all_pow2(row_scale, 'row_scale')
    q = _qmin(row_scale)
    v = x * np.asarray(row_scale, np.float64).reshape(g, r, 1)
  return f32(np.stack([assert_exact_colsum(v, 'sum x', q),
                       assert_exact_colsum(v * v, 'sum x^2', q * q)], axis=1))


def reduce_rows(partial, quantum=0.25):
  """sums[2][c] = sum over rows of partial[rows][2][c]."""
  p = np.asarray(partial, dtype=np.float64)
  rows = p.shape[0]
  return f32(assert_exact_colsum(p.reshape(rows, -1), 'partial rows', quantum).reshape(p.shape[1:]))


# ------------------------------------------------------------------ finalize
# fp32 roundings of the bounded outputs of se3ds_norm_finalize, counted from the documented
# formula rstd = rsqrt(var + eps) (a hardware estimate within one ulp, refined by one Newton step
# r (1.5 - 0.5 (var + eps) r r)), scale = gamma * rstd, shift = beta - mean * scale.  All errors
# are relative to rstd (the subtraction's operands are 1.5 and ~0.5 and its result ~1):
#   rstd:  var + eps (1), estimate within one ulp (2), two products (2), difference (1),
#          final product (1)                                                       -> 7
#   scale: rstd (7) + product with gamma (1; 0 for a power of two)                 -> 8
#   shift: scale (8, scaled by |mean|) + product (1) + difference (1)              -> 10
K_RSTD, K_SCALE, K_SHIFT = 7, 8, 10


def norm_finalize(sums, count, gamma, beta, eps, momentum, moving_mean=None, moving_var=None,
                  use_moving=0):
  """mean = S0 / count, var = S1 / count - mean^2, rstd = 1 / sqrt(var + eps), scale = gamma *
  rstd, shift = beta - mean * scale; moving <- moving - (moving - batch) * (1 - momentum).
  Returns a dict; mean, var and the moving statistics are asserted to be exact in fp32 (so they
  have one legal bit pattern), rstd / scale / shift are float64 with their magnitudes."""
  sums = np.asarray(sums, dtype=np.float64)
  g, _, c = sums.shape
  count = float(f32(count))
  eps = float(f32(eps))
  out = {}
  if use_moving:
    mean = np.broadcast_to(exact32(moving_mean, 'moving_mean'), (g, c)).copy()
    var = np.broadcast_to(exact32(moving_var, 'moving_var'), (g, c)).copy()
    out['moving_mean'], out['moving_var'] = f32(moving_mean), f32(moving_var)
  else:
    assert_pow2(count, 'count')
    mean = exact32(sums[:, 0] / count, 'mean')
    ex2 = exact32(sums[:, 1] / count, 'S1 / count')
    var = exact32(ex2 - exact32(mean * mean, 'mean^2'), 'var')
    if moving_mean is not None:
      assert g == 1
      omm = float(exact32(1.0 - float(f32(momentum)), '1 - momentum'))
      for key, mov, new in (('moving_mean', moving_mean, mean[0]), ('moving_var', moving_var, var[0])):
        mov = exact32(mov, key)
        d = exact32(mov - new, key + ' difference')
        out[key] = f32(exact32(mov - exact32(d * omm, key + ' step'), key + ' update'))
  ve = var + eps
  assert np.all(ve > 0)
  rstd = 1.0 / np.sqrt(ve)
  gm = np.ones(c) if gamma is None else np.asarray(gamma, np.float64)
  bt = np.zeros(c) if beta is None else np.asarray(beta, np.float64)
  scale = rstd * gm
  prod = mean * scale
  shift = bt - prod
  out.update(mean=f32(mean), var=f32(var), ve=ve, rstd=rstd, scale=scale, shift=shift,
             mag_rstd=np.abs(rstd), mag_scale=np.abs(scale),
             mag_shift=np.maximum(np.maximum(np.abs(prod), np.abs(bt)), np.abs(shift)))
  return out


def exactly_rounded_share(got, ref):
  """Share of elements equal to the float64 reference rounded once to fp32."""
  got = np.asarray(got, np.float32).reshape(-1)
  return float(np.mean(got == f32(ref).reshape(-1))) if got.size else 1.0


# ------------------------------------------------------------------ apply
def norm_apply(x, scale, shift, res=None, post=None, act=0, alpha=0.0, bf16=False):
  """y = act(x * scale + shift [+ res]) [+ post]; x, res, post [g, r, c], scale / shift [g, c].
  Returns (stored y as fp32, packed act_mask of the stored y or None when c % 8 != 0)."""
  x = np.asarray(x, dtype=np.float64)
  g, r, c = x.shape
  assert_np_lattice(x, 'x', 1.0, 4.0)
  assert_all_pow2(scale, 'scale')
  assert_np_lattice(shift, 'shift', 1.0, 8.0)
  q, bound = _qmin(scale), 4.0 * float(np.abs(scale).max()) + 8.0
  v = x * np.asarray(scale, np.float64).reshape(g, 1, c) + np.asarray(shift, np.float64).reshape(g, 1, c)
  if res is not None:
    assert_np_lattice(res, 'res', 1.0, 4.0)
    v = v + res
    bound += 4.0
  if act == 2:
    q *= min(1.0, float(alpha))
  v = act_np(v, act, alpha)
  if post is not None:
    assert_np_lattice(post, 'post', 1.0, 4.0)
    v = v + post
    bound += 4.0
  assert_any_order(q, bound, 'norm_apply')
  y = rne_np(exact32(v, 'y'), bf16)
  return y, (pack_mask(y) if c % 8 == 0 else None)


# ------------------------------------------------------------------ backward
def _dpre(dy, pos, act, alpha):
  dy = np.asarray(dy, dtype=np.float64)
  assert_np_lattice(dy, 'dy', 1.0, 2.0)
  return dy * act_grad_np(pos, act, alpha) if act else dy


def _xhat(x, mean, rstd):
  x = np.asarray(x, dtype=np.float64)
  g, r, c = x.shape
  assert_np_lattice(x, 'x', 1.0, 4.0)
  assert_np_lattice(mean, 'mean', 1.0, 2.0)
  assert_all_pow2(rstd, 'rstd')
  return (x - np.asarray(mean, np.float64).reshape(g, 1, c)) * np.asarray(rstd, np.float64).reshape(g, 1, c)


def norm_bwd_stats(dy, pos, x, mean, rstd, act=0, alpha=0.0):
  """sums[g][0][c] = sum dpre, sums[g][1][c] = sum dpre * xhat; dpre = dy * act'(y), pos = y > 0."""
  d = _dpre(dy, pos, act, alpha)
  xh = _xhat(x, mean, rstd)
  qd = min(1.0, float(alpha)) if act == 2 else 1.0
  return f32(np.stack([assert_exact_colsum(d, 'sum dpre', qd),
                       assert_exact_colsum(d * xh, 'sum dpre xhat', qd * _qmin(rstd))], axis=1))


def norm_bwd_apply(dy, pos, x, mean, rstd, gamma, sums, count, act=0, alpha=0.0, in_act=0,
                   in_alpha=0.0, bf16=False, sum_row=None, out_row=None, sums_quantum=None):
  """dx = gamma * rstd * (dpre - S0 / count - xhat * S1 / count) [* act'(x) for in_act]; dres =
  dpre.  With sum_row / out_row (the ROWS variants): colsum[c] = sum_r rounded dx * sum_row[r] and
  dx is stored as rounded dx * out_row[r].  Returns dict(dx, dres[, colsum]) of stored values.
  sums_quantum: lattice of S0 / S1 (default: integer multiples of count)."""
  x = np.asarray(x, dtype=np.float64)
  g, r, c = x.shape
  d = _dpre(dy, pos, act, alpha)
  xh = _xhat(x, mean, rstd)
  count = float(f32(count))
  assert_pow2(count, 'count')
  sums = np.asarray(sums, dtype=np.float64)
  qs = count if sums_quantum is None else sums_quantum
  assert_np_lattice(sums, 'sums', qs)
  gm = np.ones(c) if gamma is None else np.asarray(gamma, np.float64)
  assert_all_pow2(gm, 'gamma')
  s0 = (sums[:, 0] / count).reshape(g, 1, c)
  s1 = (sums[:, 1] / count).reshape(g, 1, c)
  gr = (gm.reshape(1, c) * np.asarray(rstd, np.float64).reshape(g, c)).reshape(g, 1, c)
  dx = gr * (d - s0 - xh * s1)
  # any rearrangement (the fast kernels evaluate gr * d + (-k1 * x + c0k)): products of subsets
  # of the factors are multiples of the product of the factors' quanta, and bounded by the
  # product of their largest magnitudes
  qd = min(1.0, float(alpha)) if act == 2 else 1.0
  q = _qmin(gm) * _qmin(rstd) ** 2 * qd * min(1.0, qs / count)
  ar = float(np.abs(rstd).max())
  xm = float(np.abs(x).max()) + float(np.abs(np.asarray(mean, np.float64)).max())
  bound = float(np.abs(gm).max()) * max(ar, 1.0) * (2.0 + float(np.abs(s0).max()) +
                                                    2.0 * max(ar, 1.0) * xm * float(np.abs(s1).max()) + 1.0)
  if in_act:
    assert in_act in (1, 2)
    if in_act == 2:
      q *= min(1.0, float(in_alpha))
    dx = dx * act_grad_np(x > 0, in_act, in_alpha)
  assert_any_order(q, bound, 'norm_bwd_apply')
  exact32(dx, 'dx')
  out = dict(dres=rne_np(exact32(d, 'dres'), bf16))
  if sum_row is None:
    out['dx'] = rne_np(dx, bf16)
    return out
  assert g == 1 and bf16 and not in_act
  assert_np_lattice(sum_row, 'sum_row', 1.0, 1.0)
  assert_all_pow2(out_row, 'out_row')
  vr = rne_np(dx, True).astype(np.float64)          # rounding to bf16 keeps multiples of q
  out['colsum'] = f32(assert_exact_colsum(vr[0] * np.asarray(sum_row, np.float64).reshape(r, 1),
                                          'bias sum of rounded dx', q))
  out['dx'] = rne_np(exact32(vr * np.asarray(out_row, np.float64).reshape(1, r, 1), 'dx * out_row'), True)
  return out


def cancelling_rows(r, c, seed, free=5, zero_share=0.3):
  """dy, x, pos [1, r, c] for se3ds_norm_bwd_cg, whose sums come from the data: cancelling row
  PAIRS (same x, same mask bits, opposite dy) at random positions plus `free` (or free + 1) rows
  of their own, so S0 and S1 are small integers whatever r is."""
  rg = rng(seed)
  nfree = free if (r - free) % 2 == 0 else free + 1
  nfree = min(nfree, r) if r >= nfree else r
  if (r - nfree) % 2:
    nfree += 1
  half = (r - nfree) // 2
  order = rg.permutation(r)
  dy = np.zeros((r, c))
  x = np.zeros((r, c))
  pos = np.zeros((r, c), dtype=bool)
  a, b, f = order[:half], order[half:2 * half], order[2 * half:]
  dy[a] = small_ints((half, c), seed + 1, -2, 2)
  dy[b] = -dy[a]
  x[a] = small_ints((half, c), seed + 2, -2, 2, zero_share)
  x[b] = x[a]
  pos[a] = rg.random((half, c)) < 0.5
  pos[b] = pos[a]
  dy[f] = small_ints((f.size, c), seed + 3, -2, 2)
  x[f] = small_ints((f.size, c), seed + 4, -2, 2)
  pos[f] = rg.random((f.size, c)) < 0.5
  return dy[None], x[None], pos[None]


def affine_bwd(dy, pos, scale, act=0, alpha=0.0, bf16=False):
  """Inference-mode backward: dx = dpre * scale, dres = dpre."""
  d = _dpre(dy, pos, act, alpha)
  g, r, c = d.shape
  assert_all_pow2(scale, 'scale')
  dx = exact32(d * np.asarray(scale, np.float64).reshape(g, 1, c), 'dx')
  return rne_np(dx, bf16), rne_np(d, bf16)


def colsum_row_scale(x, sum_row, out_row):
  """se3ds_colsum_row_scale (bf16): scaled = x * out_row[row], colsum[c] = sum_r x * sum_row[r]."""
  x = np.asarray(x, dtype=np.float64)
  r, c = x.shape
  assert_np_lattice(x, 'x', 1.0, 4.0)
  assert_all_pow2(out_row, 'out_row')
  assert_all_pow2(sum_row, 'sum_row')
  scaled = rne_np(exact32(x * np.asarray(out_row, np.float64).reshape(r, 1), 'scaled'), True)
  return scaled, f32(assert_exact_colsum(x * np.asarray(sum_row, np.float64).reshape(r, 1), 'colsum',
                                          _qmin(sum_row)))


# ------------------------------------------------------------------ pooling (NHWC)
def tie_ints(shape, seed, zero_run=0.5):
  """Integers in [-2, 2] with runs of zeros along W (post-ReLU zeros): ties, whole-window ties
  included, are frequent."""
  r = rng(seed)
  a = r.integers(-2, 3, shape).astype(np.float64)
  n, h, w, c = shape
  run = np.repeat(r.random((n, h, (w + 1) // 2, c)) < zero_run, 2, axis=2)[:, :, :w]
  rows = np.repeat(r.random((n, (h + 1) // 2, 1, c)) < 0.7, 2, axis=1)[:, :h]
  a[run & rows] = 0.0
  return a


def _windows2(h, w):
  for oy in range((h + 1) // 2):
    for ox in range((w + 1) // 2):
      yield oy, ox, [(sy, sx) for sy in (2 * oy, 2 * oy + 1) for sx in (2 * ox, 2 * ox + 1)
                     if sy < h and sx < w]


def maxpool2x2_fwd(x):
  """Keras MaxPool2D(2, padding='SAME'): windows clipped at the bottom / right edge."""
  x = np.asarray(x, dtype=np.float64)
  n, h, w, c = x.shape
  y = np.empty((n, (h + 1) // 2, (w + 1) // 2, c))
  for oy, ox, taps in _windows2(h, w):
    y[:, oy, ox] = np.max(np.stack([x[:, sy, sx] for sy, sx in taps]), axis=0)
  return y


def maxpool2x2_bwd(dy, x):
  """TF MaxPoolGrad: the gradient goes to the FIRST maximum in row-major window order
  (-0.0 == 0.0).  Returns (dx, share of windows that contain a tie for the maximum)."""
  x = np.asarray(x, dtype=np.float64)
  dy = np.asarray(dy, dtype=np.float64)
  n, h, w, c = x.shape
  dx = np.zeros_like(x)
  ties = total = 0
  for oy, ox, taps in _windows2(h, w):
    v = np.stack([x[:, sy, sx] for sy, sx in taps])           # [taps, n, c]
    hit = v == v.max(axis=0)
    first = hit & (np.cumsum(hit, axis=0) == 1)
    for k, (sy, sx) in enumerate(taps):
      dx[:, sy, sx] = np.where(first[k], dy[:, oy, ox], 0.0)
    ties += int((hit.sum(axis=0) > 1).sum())
    total += hit[0].size
  return dx, ties / max(total, 1)


def _avg_geom(size):
  o = (size + 1) // 2
  return o, max((o - 1) * 2 + 3 - size, 0) // 2


def _avg_taps(size):
  o, p = _avg_geom(size)
  return [[s for s in range(2 * i - p, 2 * i - p + 3) if 0 <= s < size] for i in range(o)]


def assert_lattice36(a, name):
  """Values in 36 * {-3..3}: divisible by every tap count (4, 6, 9) and exact in bf16."""
  q = np.asarray(a, dtype=np.float64) / 36.0
  assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 3, f'{name}: not in 36 * [-3, 3]'


def avgpool3s2_fwd(x, bf16=False, lattice36=True):
  """tf.nn.avg_pool(3, 2, 'SAME'): the divisor is the count of in-bounds taps.  lattice36: x in
  36 * {-3..3}, every quotient an integer; otherwise plain integers: the exact sum divided once
  (correctly rounded: float64 quotient -> fp32) and stored."""
  x = np.asarray(x, dtype=np.float64)
  n, h, w, c = x.shape
  if lattice36:
    assert_lattice36(x, 'x')
  else:
    assert_np_lattice(x, 'x', 1.0, 8.0)
  ty, tx = _avg_taps(h), _avg_taps(w)
  y = np.empty((n, len(ty), len(tx), c))
  for oy, ys in enumerate(ty):
    for ox, xs in enumerate(tx):
      s = sum(x[:, sy, sx] for sy in ys for sx in xs)       # integers: exact in any order
      y[:, oy, ox] = s / (len(ys) * len(xs))
  if lattice36:
    assert_np_lattice(y, 'y', 1.0, 255.0)
  return rne_np(y, bf16)


def avgpool3s2_bwd(dy, h, w, bf16=False):
  """dx[s] = sum over the windows that hold s of dy / (taps of that window); dy in 36 * {-3..3}:
  every quotient is an integer and the sum of up to four of them stays below 256."""
  dy = np.asarray(dy, dtype=np.float64)
  assert_lattice36(dy, 'dy')
  n, _, _, c = dy.shape
  ty, tx = _avg_taps(h), _avg_taps(w)
  dx = np.zeros((n, h, w, c))
  for oy, ys in enumerate(ty):
    for ox, xs in enumerate(tx):
      qv = dy[:, oy, ox] / (len(ys) * len(xs))
      assert np.array_equal(qv, np.round(qv))
      for sy in ys:
        for sx in xs:
          dx[:, sy, sx] += qv
  assert_np_lattice(dx, 'dx', 1.0, 255.0)
  return rne_np(dx, bf16)


def upsample2x_fwd(x):
  return np.repeat(np.repeat(np.asarray(x, np.float64), 2, axis=1), 2, axis=2)


def upsample2x_bwd(dy, bf16=False):
  dy = np.asarray(dy, dtype=np.float64)
  n, h2, w2, c = dy.shape
  assert_np_lattice(dy, 'dy', 1.0, 8.0)
  return rne_np(dy.reshape(n, h2 // 2, 2, w2 // 2, 2, c).sum(axis=(2, 4)), bf16)


PAD_MODES = {0: 'constant', 1: 'reflect', 2: 'symmetric'}


def pad2d(x, pad, mode, wrap_w, value=0.0):
  """PadLayer: H and W padded by `pad`; mode 0 CONSTANT(value) / 1 REFLECT / 2 SYMMETRIC;
  wrap_w: W is padded circularly instead."""
  x = np.asarray(x, dtype=np.float64)
  kw = dict(constant_values=value) if mode == 0 else {}
  y = np.pad(x, ((0, 0), (pad, pad), (0, 0), (0, 0)), mode=PAD_MODES[mode], **kw)
  if wrap_w:
    return np.pad(y, ((0, 0), (0, 0), (pad, pad), (0, 0)), mode='wrap')
  return np.pad(y, ((0, 0), (0, 0), (pad, pad), (0, 0)), mode=PAD_MODES[mode], **kw)


def copy_channels(src, src_c0, dst, dst_c0, ncopy, dst_bf16):
  """dst[r, dst_c0 + i] = convert(src[r, src_c0 + i]); the rest of dst is untouched."""
  out = np.array(dst, dtype=np.float64)
  out[:, dst_c0:dst_c0 + ncopy] = rne_np(np.asarray(src)[:, src_c0:src_c0 + ncopy], dst_bf16)
  return out


def row_scale(x, scale, bf16=False):
  x = np.asarray(x, dtype=np.float64)
  assert_all_pow2(scale, 'scale')
  return rne_np(exact32(x * np.asarray(scale, np.float64).reshape(-1, 1), 'x * scale'), bf16)


def add(a, b, bf16=False):
  return rne_np(exact32(np.asarray(a, np.float64) + np.asarray(b, np.float64), 'a + b'), bf16)


def act_bwd(dy, y, act, alpha, bf16=False):
  return rne_np(exact32(np.asarray(dy, np.float64) * act_grad_np(np.asarray(y) > 0, act, alpha),
                        'dx'), bf16)


# ------------------------------------------------------------------ partial-conv mask window
# ratio = kh kw / (cnt + 1e-6) * um: sum (1), quotient (1), product with um in {0, 1} (0) -> 2;
# bu = (1 - ratio) * um: ratio (2) + difference (1) -> 3; ru = ratio * um = ratio.
K_RATIO, K_BU = 2, 3
MASK_EPS = np.float32(1e-6)


def mask_window(mask, ho, wo, kh, kw, stride, pad_t, pad_l, wrap_w):
  """cnt = window sum of the {0, 1} mask (exact), um = clip(cnt, 0, 1), ratio = kh kw / (cnt +
  1e-6) * um, ru = ratio * um, bu = (1 - ratio) * um.  Returns a dict: um (exact), cnt, the
  float64 values ratio / ru / bu with their magnitudes, and ratio32 / bu32: the same formula
  with one fp32 rounding per operation."""
  m = np.asarray(mask, dtype=np.float64)
  n, h, w = m.shape
  assert_np_lattice(m, 'mask', 1.0, 1.0)
  assert m.min() >= 0
  cnt = np.zeros((n, ho, wo))
  for ky in range(kh):
    for kx in range(kw):
      for oy in range(ho):
        sy = oy * stride - pad_t + ky
        if not 0 <= sy < h:
          continue
        for ox in range(wo):
          sx = ox * stride - pad_l + kx
          if wrap_w:
            sx %= w
          if 0 <= sx < w:
            cnt[:, oy, ox] += m[:, sy, sx]
  um = np.clip(cnt, 0.0, 1.0)
  k = float(kh * kw)
  ratio = k / (cnt + float(MASK_EPS)) * um
  bu = (1.0 - ratio) * um
  den32 = (cnt.astype(np.float32) + MASK_EPS).astype(np.float32)
  ratio32 = ((np.float32(k) / den32).astype(np.float32) * um.astype(np.float32)).astype(np.float32)
  bu32 = ((np.float32(1) - ratio32).astype(np.float32) * um.astype(np.float32)).astype(np.float32)
  return dict(cnt=cnt, um=f32(um), ratio=ratio, ru=ratio * um, bu=bu, ratio32=ratio32, bu32=bu32,
              mag_ratio=np.abs(ratio), mag_bu=np.maximum(np.maximum(np.abs(ratio), 1.0) * um, np.abs(bu)))
