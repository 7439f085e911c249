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
