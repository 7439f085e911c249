"""Bit-exact integer-lattice tests of every convolution kernel route (tests/_lattice.py).

Inputs are drawn from {-1, 0, 1} (epilogue slots from powers of two, {0, 1} and small integers), so
every kernel result has exactly one legal bit pattern whatever the tiling, split or MFMA shape, and
the comparison is `==`.  Each route case first asserts, through se3ds_debug_conv_route_history, that
the kernel instantiation it is named for really ran; the last test asserts that the route table
names every route the library reports, so a new kernel without a lattice case fails the suite.

The exported entry points are called through ctypes: operand copies, epilogue vectors, masks,
workspaces and the guard bands around every output are under the test's control.  Every output
buffer has 256 bytes of NaN on both sides and is pre-filled with NaN (or with the integer prior
where the entry point accumulates): the bands must be intact and no NaN may survive inside.
"""
import ctypes

import numpy as np
import pytest
import torch

from se3ds_amd import _lib
import se3ds_amd.hipops  # noqa: F401  registers the conv signatures
import _lattice as LT
from test_prod_shapes_gpu import PROD_CONVS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD_BYTES = 256
_DT = {'bf16': torch.bfloat16, 'f32': torch.float32}


def _L():
  return _lib.lib()


def route_names():
  out, i = [], 0
  while True:
    s = _L().se3ds_debug_conv_route_name(i)
    if s is None:
      return out
    out.append(s.decode())
    i += 1


def last_routes(count):
  """Names of the calling thread's last `count` launches, oldest first."""
  L = _L()
  ids = [L.se3ds_debug_conv_route_history(b) for b in range(count - 1, -1, -1)]
  return [L.se3ds_debug_conv_route_name(i).decode() if i >= 0 else None for i in ids]


class Guarded:
  """A device buffer with NaN guard bands of 256 bytes on both sides."""

  def __init__(self, shape, dtype, fill=None):
    self.g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape))
    self.flat = torch.full((n + 2 * self.g,), float('nan'), dtype=dtype, device=DEV)
    self.view = self.flat[self.g:self.g + n].view(*shape)
    if fill is not None:
      self.view.copy_(fill.to(dtype))

  def ptr(self):
    return self.view.data_ptr()

  def result(self, what):
    torch.cuda.synchronize()
    lo, hi = self.flat[:self.g], self.flat[-self.g:]
    assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), f'{what}: guard band overwritten'
    out = self.view.float().cpu()
    assert not bool(torch.isnan(out).any()), (
        f'{what}: {int(torch.isnan(out).sum())} elements never written, first at '
        f'{tuple(int(v) for v in torch.nonzero(torch.isnan(out))[0])}')
    return out


def dev(t, dtype=torch.float32):
  return None if t is None else t.to(dtype).to(DEV).contiguous()


def p(t):
  return None if t is None else t.data_ptr()


def khw(c):
  """case dict -> (kh, kw): a case may carry its own 'kh' / 'kw', both default to 'k'."""
  return c.get('kh', c['k']), c.get('kw', c['k'])


def geom(c):
  """case dict -> (ho, wo, pad_t, pad_l)."""
  (kh, kw), s = khw(c), c.get('stride', 1)
  ho, pt = LT.out_size(c['h'], kh, s, c.get('padding', 'VALID'), c.get('pad', 0))
  wo, pl = LT.out_size(c['w'], kw, s, c.get('padding', 'VALID'), c.get('pad', 0))
  return ho, wo, c.get('pad_t', pt), c.get('pad_l', pl)


def C(cin, cout, k, stride, padding, pad, n, h, w, **kw):
  d = dict(cin=cin, cout=cout, k=k, stride=stride, padding=padding, pad=pad, n=n, h=h, w=w)
  d.update(kw)
  return d


def _seed(c, salt):
  kh, kw = khw(c)
  if kh != kw:   # (square cases keep the seeds they always had)
    return hash((c['cin'], c['cout'], c['k'], c['n'], c['h'], c['w'], kh, kw, salt)) % (2 ** 31)
  return hash((c['cin'], c['cout'], c['k'], c['n'], c['h'], c['w'], salt)) % (2 ** 31)


def _note_visibility(pre, q, what):
  """Asserts the case's own share (<= 10 %) on the reference alone and prints it (-s shows it)."""
  s = LT.assert_visible(pre, what, q)
  if s > 0:
    print('invisible share %.4f %% in %s' % (100 * s, what))
  return s


def _expected_stored(y, pre, q, dt, what):
  if dt == 'bf16':
    _note_visibility(pre, q, what)
    return LT.rne_bf16(y)
  LT.assert_exact_range(y, what, 0.25)
  return y


_MEMO = {}


def _memo(kind, c, fn):
  """The exact reference of a case serves its bf16 and its fp32 run (same seeds, same inputs): the
  last one per entry point is kept."""
  key = repr(sorted(c.items()))
  if _MEMO.get(kind, (None, None))[0] != key:
    _MEMO[kind] = (key, fn())
  return _MEMO[kind][1]


def _mask_args(c, n, h, w, seed):
  """mask option -> (cpu mask or None, in_mask_binary flag)."""
  m = c.get('mask')
  if not m:
    return None, 0
  return LT.binary_mask(n, h, w, seed), 1 if m == 'binary' else 0


# ---------------------------------------------------------------------------------------------
# runners: one per entry point; each returns the route names of its launches, oldest first

def run_fwd(c, dt, stats=False):
  """se3ds_conv2d_fwd / _fwd_stats with the epilogue form c['epi']:
  none | scale | bias | bias_relu | bias_leaky | partial_bias | partial."""
  L, T = _L(), _DT[dt]
  n, h, w, cin, cout, s = c['n'], c['h'], c['w'], c['cin'], c['cout'], c.get('stride', 1)
  kh, kw = khw(c)
  ho, wo, pt, pl = geom(c)
  x, kern = LT.ternary((n, h, w, cin), _seed(c, 1)), LT.ternary((kh, kw, cin, cout), _seed(c, 2))
  mask, mbin = _mask_args(c, n, h, w, _seed(c, 3))
  epi = c.get('epi', 'none')
  scale = LT.pow2_scale(_seed(c, 4)) if epi in ('scale', 'partial_bias', 'partial', 'bias_leaky') else None
  bias = LT.bias_ints(cout, _seed(c, 5)) if epi.startswith('bias') or epi == 'partial_bias' else None
  row_a = LT.pow2_rows(n * ho * wo, _seed(c, 6)) if epi.startswith('partial') else None
  row_b = LT.binary_rows(n * ho * wo, _seed(c, 7)) if epi == 'partial_bias' else None
  act, alpha = {'bias_relu': (1, 0.0), 'bias_leaky': (2, 0.25)}.get(epi, (0, 0.0))
  y, pre, q = _memo('fwd', c, lambda: LT.conv2d_fwd(x, kern, ho, wo, s, pt, pl, c.get('wrap', 0), mask,
                                                     scale, bias, row_a, row_b, act, alpha))
  what = f'fwd {dt} {c}'
  exp = _expected_stored(y, pre, q, dt, what)
  wt, _ = LT.weight_operands(kern, T)
  out = Guarded((n, ho, wo, cout), T)
  dx, dwt, dm = dev(x, T), dev(wt, T), dev(mask)
  ds, db, da, drb = dev(scale), dev(bias), dev(row_a), dev(row_b)
  args = [p(dx), p(dwt), out.ptr(), _lib.dtype_code(dx), n, h, w, cin, ho, wo, cout, kh, kw, s, pt, pl,
          c.get('wrap', 0), p(dm), mbin, p(ds), p(db), p(da), p(drb), act, alpha]
  if stats:
    rows = L.se3ds_conv2d_fwd_stats_rows(_lib.dtype_code(dx), n, cin, ho, wo, cout, kh, kw, s,
                                         int(mask is not None), mbin)
    assert rows > 0, f'{what}: no fused statistics path'
    st = Guarded((rows, 2, cout), torch.float32)
    _lib.check(L.se3ds_conv2d_fwd_stats(*args, st.ptr(), _lib.stream()), what)
  else:
    _lib.check(L.se3ds_conv2d_fwd(*args, _lib.stream()), what)
  routes = last_routes(1)
  LT.assert_bit_equal(out.result(what), exp, what)
  if stats:
    s1, s2 = LT.column_stats(exp)
    got = st.result(what + ' stats').double().sum(0).float()
    LT.assert_bit_equal(got[0], s1, what + ' column sums', 'flat')
    LT.assert_bit_equal(got[1], s2, what + ' column sums of squares', 'flat')
    # and through the library's own row reduction
    ws_b = L.se3ds_norm_workspace_bytes(2, cout) + rows * 2 * cout * 4 + 4096
    ws = torch.empty(ws_b, dtype=torch.uint8, device=DEV)
    red = Guarded((2, cout), torch.float32)
    _lib.check(L.se3ds_norm_reduce_rows(st.ptr(), rows, cout, red.ptr(), ws.data_ptr(), ws_b,
                                        _lib.stream()), 'norm_reduce_rows')
    r = red.result(what + ' reduced stats')
    LT.assert_bit_equal(r[0], s1, what + ' reduced sums', 'flat')
    LT.assert_bit_equal(r[1], s2, what + ' reduced sums of squares', 'flat')
  return routes


def run_dgrad(c, dt):
  """se3ds_conv2d_dgrad / _dgrad_acc with c['epi']: none | scale | row_a | bias | bias_relu;
  c['acc']: integer addend; c['row_scale']: dy row scale."""
  L, T = _L(), _DT[dt]
  n, h, w, cin, cout, s = c['n'], c['h'], c['w'], c['cin'], c['cout'], c.get('stride', 1)
  kh, kw = khw(c)
  ho, wo, pt, pl = geom(c)
  dy, kern = LT.ternary((n, ho, wo, cout), _seed(c, 11)), LT.ternary((kh, kw, cin, cout), _seed(c, 2))
  epi = c.get('epi', 'none')
  scale = LT.pow2_scale(_seed(c, 4)) if epi in ('scale', 'row_a') else None
  row_a = LT.pow2_rows(n * h * w, _seed(c, 6)) if epi == 'row_a' else None
  bias = LT.bias_ints(cin, _seed(c, 5)) if epi.startswith('bias') else None
  act, alpha = (1, 0.0) if epi == 'bias_relu' else (0, 0.0)
  rs = LT.pow2_rows(n * ho * wo, _seed(c, 8)) if c.get('row_scale') else None
  addend = LT.prior_grad((n, h, w, cin), _seed(c, 9)) if c.get('acc') else None
  dxe, pre, q = _memo('dgrad', c, lambda: LT.conv2d_dgrad(dy, kern, (n, h, w, cin), s, pt, pl,
                                                          c.get('wrap', 0), rs, scale, bias, row_a, act,
                                                          alpha, addend))
  what = f'dgrad {dt} {c}'
  exp = _expected_stored(dxe, pre, q, dt, what)
  _, wn = LT.weight_operands(kern, T)
  out = Guarded((n, h, w, cin), T, fill=addend)   # the addend may be dx itself
  ddy, dwn = dev(dy, T), dev(wn, T)
  drs, ds, db, da = dev(rs), dev(scale), dev(bias), dev(row_a)
  args = [p(ddy), p(dwn), out.ptr(), _lib.dtype_code(ddy), n, h, w, cin, ho, wo, cout, kh, kw, s, pt, pl,
          c.get('wrap', 0), p(drs), p(ds), p(db), p(da), act, alpha]
  if addend is not None:
    _lib.check(L.se3ds_conv2d_dgrad_acc(*args, out.ptr(), _lib.stream()), what)
  else:
    _lib.check(L.se3ds_conv2d_dgrad(*args, _lib.stream()), what)
  routes = last_routes(1)
  LT.assert_bit_equal(out.result(what), exp, what)
  return routes


def run_dgrad_bn(c, dt='bf16'):
  """se3ds_conv2d_dgrad_bnstats with integer means, power-of-two rstd, ternary bn_x and a ReLU
  mask: dx, dz = dx_stored * act'(y) and dz * xhat are all integers (times a power of two), so the
  per-tile sums are exact in fp32 and the reduced statistics have one legal value.  dx is compared
  bit for bit; the statistics rows are summed in float64 on the host (exact) and compared with `==`."""
  L, T = _L(), torch.bfloat16
  n, h, w, cin, cout, k = c['n'], c['h'], c['w'], c['cin'], c['cout'], c['k']
  ho, wo, pt, pl = geom(c)
  rows = L.se3ds_conv2d_dgrad_bnstats_rows(_lib.BF16, n, h, w, cin, cout, k, k, 1, 0)
  what = f'dgrad_bnstats {c}'
  assert rows > 0, f'{what}: no fused path'
  dy, kern = LT.ternary((n, ho, wo, cout), _seed(c, 11)), LT.ternary((k, k, cin, cout), _seed(c, 2))
  addend = LT.prior_grad((n, h, w, cin), _seed(c, 9)) if c.get('acc') else None
  bn_x = LT.ternary((n, h, w, cin), _seed(c, 12))
  mean = LT.integers((cin,), _seed(c, 13), -2, 2)
  rstd = LT.choice((cin,), _seed(c, 14), (0.5, 1.0, 2.0))
  bits = torch.randint(0, 2, (n * h * w * cin,), generator=torch.Generator().manual_seed(_seed(c, 15)))
  dxe, pre, q = LT.conv2d_dgrad(dy, kern, (n, h, w, cin), 1, pt, pl, 0, addend=addend)
  _note_visibility(pre, q, what)
  exp = LT.rne_bf16(dxe)
  dz = exp * bits.view(n, h, w, cin).float()             # ReLU: act'(y) = (y > 0)
  xhat = (bn_x - mean) * rstd
  e1 = dz.double().reshape(-1, cin).sum(0)
  e2 = (dz * xhat).double().reshape(-1, cin).sum(0)
  assert float((dz * xhat).abs().double().reshape(-1, cin).sum(0).max()) < LT.LIMIT
  packed = torch.from_numpy(np.packbits(bits.numpy().astype(np.uint8), bitorder='little'))
  out = Guarded((n, h, w, cin), T, fill=addend)
  st = Guarded((rows, 2, cin), torch.float32)
  ddy, dwn = dev(dy, T), dev(LT.weight_operands(kern, T)[1], T)
  dbx, dmask, dmean, drstd = dev(bn_x, T), packed.to(DEV), dev(mean), dev(rstd)
  _lib.check(L.se3ds_conv2d_dgrad_bnstats(
      p(ddy), p(dwn), out.ptr(), _lib.BF16, n, h, w, cin, ho, wo, cout, k, k, 1, pt, pl, 0, None, None,
      out.ptr() if addend is not None else None, p(dbx), p(dmask), p(dmean), p(drstd), 1, 0.0, st.ptr(),
      _lib.stream()), what)
  routes = last_routes(1)
  LT.assert_bit_equal(out.result(what), exp, what)
  got = st.result(what + ' stats').double().sum(0)
  LT.assert_bit_equal(got[0].float(), e1.float(), what + ' sum dz', 'flat')
  LT.assert_bit_equal(got[1].float(), e2.float(), what + ' sum dz * xhat', 'flat')
  return routes


def _wgrad_inputs(c, dt):
  n, h, w, cin, cout, k = c['n'], c['h'], c['w'], c['cin'], c['cout'], c['k']
  ho, wo, pt, pl = geom(c)
  x, dy = LT.ternary((n, h, w, cin), _seed(c, 1)), LT.ternary((n, ho, wo, cout), _seed(c, 11))
  mask, mbin = _mask_args(c, n, h, w, _seed(c, 3))
  rs = LT.pow2_rows(n * ho * wo, _seed(c, 8)) if c.get('row_scale') else None
  return x, dy, mask, mbin, rs


def run_wgrad(c, dt, launches=2):
  """se3ds_conv2d_wgrad: c['mask'], c['row_scale'], c['out_scale'], c['acc'] (accumulate = 1 onto an
  integer prior).  Returns the routes of the main kernel and of the split reduction."""
  L, T = _L(), _DT[dt]
  n, h, w, cin, cout, s = c['n'], c['h'], c['w'], c['cin'], c['cout'], c.get('stride', 1)
  kh, kw = khw(c)
  ho, wo, pt, pl = geom(c)
  x, dy, mask, mbin, rs = _wgrad_inputs(c, dt)
  osc = LT.pow2_scale(_seed(c, 16)) if c.get('out_scale') else None
  prior = LT.prior_grad((kh, kw, cin, cout), _seed(c, 17)) if c.get('acc') else None
  exp = _memo('wgrad', c, lambda: LT.conv2d_wgrad(x, dy, (kh, kw, cin, cout), s, pt, pl, c.get('wrap', 0),
                                                  mask, rs, osc, prior))
  what = f'wgrad {dt} {c}'
  out = Guarded((kh, kw, cin, cout), torch.float32, fill=prior)
  wsb = L.se3ds_conv2d_wgrad_workspace_bytes(n, ho, wo, cin, cout, kh, kw)
  ws = Guarded((wsb // 4 + 1,), torch.float32)
  dx, ddy, dm, drs, dos = dev(x, T), dev(dy, T), dev(mask), dev(rs), dev(osc)
  _lib.check(L.se3ds_conv2d_wgrad(p(dx), p(ddy), out.ptr(), _lib.dtype_code(dx), n, h, w, cin, ho, wo,
                                  cout, kh, kw, s, pt, pl, c.get('wrap', 0), p(dm), mbin, p(drs), p(dos),
                                  int(prior is not None), ws.ptr(), wsb, _lib.stream()), what)
  routes = last_routes(launches)
  LT.assert_bit_equal(out.result(what), exp, what, 'hwio')
  torch.cuda.synchronize()
  assert bool(torch.isnan(ws.flat[:ws.g]).all()) and bool(torch.isnan(ws.flat[-ws.g:]).all()), (
      f'{what}: workspace guard band overwritten')
  return routes


def run_swapped(c, dt, launches):
  L, T = _L(), _DT[dt]
  n, h, w, cin, cout, k, pad = c['n'], c['h'], c['w'], c['cin'], c['cout'], c['k'], c['pad']
  x, dy = LT.ternary((n, h, w, cin), _seed(c, 1)), LT.ternary((n, h, w, cout), _seed(c, 11))
  prior = LT.prior_grad((k, k, cin, cout), _seed(c, 17)) if c.get('acc') else None
  exp = LT.conv2d_wgrad_swapped(x, dy, k, pad, prior)
  what = f'wgrad_swapped {dt} {c}'
  out = Guarded((k, k, cin, cout), torch.float32, fill=prior)
  wsb = L.se3ds_conv2d_wgrad_swapped_workspace_bytes(n, h, w, cin, cout, k)
  ws = Guarded((wsb // 4 + 1,), torch.float32)
  dx, ddy = dev(x, T), dev(dy, T)
  _lib.check(L.se3ds_conv2d_wgrad_swapped(p(dx), p(ddy), out.ptr(), _lib.dtype_code(dx), n, h, w, cin,
                                          cout, k, pad, int(prior is not None), ws.ptr(), wsb,
                                          _lib.stream()), what)
  routes = last_routes(launches)
  LT.assert_bit_equal(out.result(what), exp, what, 'hwio')
  torch.cuda.synchronize()
  assert bool(torch.isnan(ws.flat[:ws.g]).all()) and bool(torch.isnan(ws.flat[-ws.g:]).all()), (
      f'{what}: workspace guard band overwritten')
  return routes


def run_convt(c, dt):
  L, T = _L(), _DT[dt]
  n, h, w, cin, cout = c['n'], c['h'], c['w'], c['cin'], c['cout']
  x, kern = LT.ternary((n, h, w, cin), _seed(c, 1)), LT.ternary((2, 2, cout, cin), _seed(c, 2))
  bias = LT.bias_ints(cout, _seed(c, 5)) if c.get('epi') == 'bias' else None
  y = LT.conv_transpose2x2(x, kern, bias)
  what = f'conv_transpose2x2 {dt} {c}'
  exp = _expected_stored(y, y, 1.0, dt, what)
  out = Guarded((n, 2 * h, 2 * w, cout), T)
  dx, dk, db = dev(x, T), dev(kern, T), dev(bias)
  _lib.check(L.se3ds_conv_transpose2x2_fwd(p(dx), p(dk), out.ptr(), _lib.dtype_code(dx), n, h, w, cin,
                                           cout, p(db), _lib.stream()), what)
  routes = last_routes(2)
  LT.assert_bit_equal(out.result(what), exp, what)
  return routes


def run_prep(c, dt):
  """se3ds_weight_prep: wt [cout][K], wn [K][cout] of an fp32 master (ternary: exact in bf16)."""
  L, T = _L(), _DT[dt]
  k, cout = c['K'], c['cout']
  w = LT.ternary((1, 1, k, cout), c['K'] * 131 + cout)
  wt_e, wn_e = LT.weight_operands(w)
  wt, wn = Guarded((cout, k), T), Guarded((k, cout), T)
  dw = dev(w)
  _lib.check(L.se3ds_weight_prep(p(dw), k, cout, _lib.dtype_code(wt.view), wt.ptr(), wn.ptr(),
                                 _lib.stream()), f'weight_prep {c}')
  routes = last_routes(1)
  LT.assert_bit_equal(wt.result('wt'), wt_e, f'weight_prep {dt} {c} wt', 'flat')
  LT.assert_bit_equal(wn.result('wn'), wn_e, f'weight_prep {dt} {c} wn', 'flat')
  return routes


# ---------------------------------------------------------------------------------------------
# the route table: route name -> (runner, case, dtype, environment, launches checked)
# Routes the default dispatch takes carry no environment, at a shape where the cost model picks
# them; only the 128-channel macro tile and the 32x32x16 MFMA variants are forced-only and use the
# existing switches (the 32x32x16 forms of the 256-channel tiles on small maps also force the width).

M32 = {'SE3DS_HALO_M16': '0'}
BIG = {'SE3DS_BIG_TILE': '1'}
H256 = {'SE3DS_HALO_TILE': '256'}
_r3 = dict(k=3, stride=1, padding='VALID', pad=1)

ROUTES = {
    # thin layers (default dispatch)
    'thin_s2_dgrad': ('dgrad', C(3, 128, 4, 2, 'VALID', 2, 1, 70, 130), 'bf16', {}),
    'thin_cin_fwd': ('fwd', C(5, 128, 7, 2, 'VALID', 3, 2, 32, 64, mask='binary', epi='partial_bias'), 'bf16', {}),
    'thin_cout_dgrad': ('dgrad', C(128, 3, 3, 1, 'VALID', 1, 2, 12, 64, epi='bias'), 'bf16', {}),
    'thin_cout_fwd': ('fwd', C(128, 1, 3, 1, 'VALID', 1, 2, 9, 37, epi='bias'), 'bf16', {}),
    # halo-resident 3x3: 256 channels where the grid fills the chip, 128 otherwise
    'halo256_fwd_m16': ('fwd', C(64, 1024, 3, 1, 'VALID', 1, 1, 61, 250, epi='bias_relu'), 'bf16', {}),
    'halo256_dgrad_m16': ('dgrad', C(1024, 64, 3, 1, 'VALID', 1, 1, 61, 250), 'bf16', {}),
    'halo256_dgrad_bn_m16': ('dgrad_bn', C(256, 64, 3, 1, 'VALID', 1, 3, 61, 250, acc=1), 'bf16', {}),
    'halo256_fwd_m32': ('fwd', C(64, 256, 3, 1, 'VALID', 1, 2, 16, 32, epi='scale'), 'bf16', dict(M32, **H256)),
    'halo256_dgrad_m32': ('dgrad', C(256, 64, 3, 1, 'VALID', 1, 3, 11, 23, epi='row_a'), 'bf16', dict(M32, **H256)),
    'halo256_dgrad_bn_m32': ('dgrad_bn', C(256, 64, 3, 1, 'VALID', 1, 2, 9, 17), 'bf16', dict(M32, **H256)),
    'halo128_fwd_m16': ('fwd', C(192, 128, 3, 1, 'VALID', 1, 1, 20, 70, epi='bias_leaky'), 'bf16', {}),
    'halo128_dgrad_m16': ('dgrad', C(128, 192, 3, 1, 'VALID', 1, 1, 20, 70, acc=1), 'bf16', {}),
    'halo128_dgrad_bn_m16': ('dgrad_bn', C(128, 64, 3, 1, 'SAME', 0, 2, 8, 32), 'bf16', {}),
    'halo128_fwd_m32': ('fwd', C(64, 128, 3, 1, 'SAME', 0, 2, 8, 32), 'bf16', M32),
    'halo128_dgrad_m32': ('dgrad', C(128, 64, 3, 1, 'VALID', 1, 3, 11, 23), 'bf16', M32),
    'halo128_dgrad_bn_m32': ('dgrad_bn', C(128, 128, 3, 1, 'VALID', 1, 1, 20, 70, acc=1), 'bf16', M32),
    # 256-pixel macro tile: the cost model takes the 256-channel form for a full last round
    'big256_fwd_m16': ('fwd', C(64, 256, 1, 1, 'SAME', 0, 1, 128, 512, epi='bias'), 'bf16', {}),
    'big256_dgrad_m16': ('dgrad', C(256, 64, 1, 1, 'SAME', 0, 1, 128, 512), 'bf16', {}),
    'big256_dgrad_bn_m16': ('dgrad_bn', C(256, 64, 1, 1, 'SAME', 0, 1, 128, 509, acc=1), 'bf16', {}),
    'big256_fwd_m32': ('fwd', C(128, 256, 4, 2, 'VALID', 2, 2, 18, 34, epi='bias'), 'bf16', dict(M32, **BIG)),
    'big256_dgrad_m32': ('dgrad', C(256, 128, 4, 2, 'VALID', 2, 2, 18, 34), 'bf16', dict(M32, **BIG)),
    'big256_dgrad_bn_m32': ('dgrad_bn', C(256, 64, 1, 1, 'SAME', 0, 2, 9, 17), 'bf16', dict(M32, **BIG)),
    'big128_fwd_m16': ('fwd', C(64, 128, 3, 2, 'VALID', 1, 2, 16, 32, mask='binary', epi='partial_bias'), 'bf16', BIG),
    'big128_dgrad_m16': ('dgrad', C(128, 64, 3, 2, 'VALID', 1, 2, 17, 33), 'bf16', BIG),
    'big128_dgrad_bn_m16': ('dgrad_bn', C(128, 64, 1, 1, 'SAME', 0, 3, 11, 23), 'bf16', BIG),
    'big128_fwd_m32': ('fwd', C(64, 128, 1, 1, 'SAME', 0, 3, 11, 23, epi='scale'), 'bf16', dict(M32, **BIG)),
    'big128_dgrad_m32': ('dgrad', C(128, 64, 4, 2, 'VALID', 2, 2, 18, 34), 'bf16', dict(M32, **BIG)),
    'big128_dgrad_bn_m32': ('dgrad_bn', C(128, 64, 1, 1, 'SAME', 0, 1, 20, 70, acc=1), 'bf16', dict(M32, **BIG)),
    # 128 x 128 LDS-DMA kernels
    'glds_f32_fwd': ('fwd', C(32, 64, 3, 1, 'VALID', 1, 2, 16, 32, epi='bias'), 'f32', {}),
    'glds_f32_dgrad': ('dgrad', C(64, 32, 4, 2, 'VALID', 2, 2, 18, 34), 'f32', {}),
    'glds_bf16_fwd_m16': ('fwd', C(64, 128, 1, 1, 'SAME', 0, 2, 9, 17, epi='bias'), 'bf16', {}),
    'glds_bf16_dgrad_m16': ('dgrad', C(128, 64, 4, 2, 'VALID', 2, 2, 18, 34), 'bf16', {}),
    'glds_bf16_dgrad_bn_m16': ('dgrad_bn', C(128, 64, 1, 1, 'SAME', 0, 3, 11, 23, acc=1), 'bf16', {}),
    'glds_bf16_fwd_m32': ('fwd', C(64, 160, 3, 1, 'VALID', 1, 2, 8, 16, epi='bias'), 'bf16', {}),
    'glds_bf16_dgrad_m32': ('dgrad', C(48, 64, 1, 1, 'SAME', 0, 1, 8, 16), 'bf16', {}),
    'glds_bf16_dgrad_bn_m32': ('dgrad_bn', C(128, 64, 1, 1, 'SAME', 0, 2, 9, 17), 'bf16', M32),
    # scalar-gather kernels (ragged reduction channels, non-binary masks)
    'igemm_f32_fwd': ('fwd', C(5, 16, 7, 2, 'VALID', 3, 2, 32, 64, mask='plain', epi='partial_bias'), 'f32', {}),
    'igemm_f32_dgrad': ('dgrad', C(16, 5, 3, 1, 'VALID', 1, 2, 9, 17, row_scale=1), 'f32', {}),
    'igemm_bf16_fwd': ('fwd', C(48, 32, 1, 1, 'SAME', 0, 1, 8, 16, epi='partial'), 'bf16', {}),
    'igemm_bf16_dgrad': ('dgrad', C(32, 48, 3, 2, 'VALID', 1, 2, 16, 32, row_scale=1, epi='row_a'), 'bf16', {}),
    # weight gradients: (main kernel, split reduction)
    'wgrad_taps3_m16': ('wgrad', C(64, 128, 3, 1, 'VALID', 1, 3, 11, 23, mask='binary'), 'bf16', {}),
    'wgrad_taps3_m32': ('wgrad', C(192, 128, 3, 1, 'VALID', 1, 1, 20, 70), 'bf16', M32),
    'wgrad_taps_wrap': ('wgrad', C(128, 128, 3, 1, 'VALID', 1, 1, 16, 32, wrap=1, pad_t=1, pad_l=1), 'bf16', {}),
    'thin_cin_wgrad': ('wgrad', C(5, 128, 7, 2, 'VALID', 3, 2, 32, 64, mask='binary', row_scale=1), 'bf16', {}),
    'wgrad_glds_f32': ('wgrad', C(32, 64, 3, 1, 'VALID', 1, 2, 16, 32), 'f32', {}),
    'wgrad_glds_bf16': ('wgrad', C(128, 256, 4, 2, 'VALID', 2, 2, 18, 34, acc=1), 'bf16', {}),
    'wgrad_f32': ('wgrad', C(5, 16, 7, 2, 'VALID', 3, 2, 32, 64, mask='plain', row_scale=1, out_scale=1), 'f32', {}),
    'wgrad_bf16': ('wgrad', C(32, 32, 3, 2, 'VALID', 1, 2, 16, 32, mask='binary', row_scale=1, acc=1), 'bf16', {}),
    'wgrad_reduce_vec': ('wgrad', C(64, 160, 3, 1, 'VALID', 1, 2, 8, 16, out_scale=1), 'bf16', {}),
    'wgrad_reduce_scalar': ('wgrad', C(5, 3, 3, 1, 'VALID', 1, 2, 9, 17, acc=1), 'f32', {}),
    'wgrad_reduce_multi': ('reduce_multi', None, 'bf16', {}),
    # swapped weight gradient of the thin heads
    'thin_cout_wgrad_t2': ('swapped', C(32, 3, 3, 1, 'VALID', 1, 2, 17, 40), 'bf16', {}),
    'thin_cout_wgrad_t3': ('swapped', C(64, 3, 3, 1, 'VALID', 1, 2, 12, 20, acc=1), 'bf16', {}),
    'thin_cout_wgrad_t4': ('swapped', C(96, 2, 3, 1, 'VALID', 1, 1, 20, 70), 'bf16', {}),
    'thin_cout_wgrad_t5': ('swapped', C(128, 1, 3, 1, 'VALID', 1, 2, 9, 37), 'bf16', {}),
    'pad_channels8': ('swapped', C(192, 3, 3, 1, 'VALID', 1, 1, 20, 70), 'bf16', {}),
    'wgrad_taps_thin': ('swapped', C(64, 8, 3, 1, 'VALID', 1, 2, 12, 20, acc=1), 'bf16', {}),
    'wgrad_swap_fixup': ('swapped', C(48, 3, 3, 1, 'VALID', 1, 2, 12, 20, acc=1), 'f32', {}),
    # operand copies
    'weight_prep_f32': ('prep', dict(K=45, cout=3), 'f32', {}),
    'weight_prep_bf16': ('prep', dict(K=45, cout=3), 'bf16', {}),
    'weight_prep_vec': ('prep', dict(K=9 * 48, cout=160), 'bf16', {}),
    'weight_prep_multi': ('prep_multi', None, 'bf16', {}),
}

# the exact launches of the multi-launch entry points, oldest first ('R': the split reduction,
# vec or scalar); every other route case is one launch.  The ring is read back exactly this deep, so
# a launch of an earlier case can never stand in for one of this case.
_R = ('wgrad_reduce_vec', 'wgrad_reduce_scalar')
_SWAPPED = {
    'thin_cout_wgrad_t2': ['thin_cout_wgrad_t2', 'R'], 'thin_cout_wgrad_t3': ['thin_cout_wgrad_t3', 'R'],
    'thin_cout_wgrad_t4': ['thin_cout_wgrad_t4', 'R'], 'thin_cout_wgrad_t5': ['thin_cout_wgrad_t5', 'R'],
    'pad_channels8': ['pad_channels8', 'wgrad_taps_thin', 'R'],
    'wgrad_taps_thin': ['pad_channels8', 'wgrad_taps_thin', 'R'],
    'wgrad_swap_fixup': ['wgrad_f32', 'R', 'wgrad_swap_fixup'],
}
_WGRAD_OF_REDUCE = {'wgrad_reduce_vec': 'wgrad_glds_bf16', 'wgrad_reduce_scalar': 'wgrad_f32'}


def _expected_launches(name, kind):
  if kind == 'wgrad':
    return [_WGRAD_OF_REDUCE[name], name] if name in _WGRAD_OF_REDUCE else [name, 'R']
  if kind == 'swapped':
    return _SWAPPED[name]
  return [name]


def _same_launches(got, want):
  return len(got) == len(want) and all(g in _R if w == 'R' else g == w for g, w in zip(got, want))


def _setenv(monkeypatch, env):
  for k in ('SE3DS_HALO_M16', 'SE3DS_BIG_TILE', 'SE3DS_HALO_TILE', 'SE3DS_NO_THIN'):
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)


def _reduce_multi_case():
  """se3ds_conv2d_wgrad_partial over three layers + ONE se3ds_wgrad_reduce_multi launch: bit-equal
  to the lattice reference (hence to the per-layer call, which the route cases hold to the same)."""
  L = _L()
  layers = [C(64, 128, 3, 1, 'VALID', 1, 3, 11, 23), C(128, 256, 4, 2, 'VALID', 2, 2, 18, 34),
            C(5, 128, 7, 2, 'VALID', 3, 2, 32, 64)]
  tile = L.se3ds_wgrad_reduce_tile()
  rows, outs, exps, keep, first = [], [], [], [], 0
  for c in layers:
    n, h, w, cin, cout, k, s = c['n'], c['h'], c['w'], c['cin'], c['cout'], c['k'], c['stride']
    ho, wo, pt, pl = geom(c)
    x, dy, _, _, _ = _wgrad_inputs(c, 'bf16')
    exps.append(LT.conv2d_wgrad(x, dy, (k, k, cin, cout), s, pt, pl))
    out = Guarded((k, k, cin, cout), torch.float32)
    wsb = L.se3ds_conv2d_wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dx, ddy = dev(x, torch.bfloat16), dev(dy, torch.bfloat16)
    row = (ctypes.c_int64 * 5)()
    _lib.check(L.se3ds_conv2d_wgrad_partial(p(dx), p(ddy), out.ptr(), _lib.BF16, n, h, w, cin, ho, wo,
                                            cout, k, k, s, pt, pl, 0, None, 0, None, ws.data_ptr(), wsb,
                                            row, _lib.stream()), 'wgrad_partial')
    assert row[4] == 1, 'aligned layer: the reduction must have been deferred'
    main = last_routes(1)[0]
    assert not main.startswith('wgrad_reduce'), main    # nothing launched after the main kernel
    rows.append([row[0], row[1], row[2], row[3], first])
    first += -(-row[2] // tile)
    outs.append(out)
    keep += [ws, dx, ddy]
  table = torch.tensor(rows, dtype=torch.int64).to(DEV)
  _lib.check(L.se3ds_wgrad_reduce_multi(table.data_ptr(), len(rows), first, _lib.stream()), 'reduce_multi')
  routes = last_routes(1)
  for c, out, exp in zip(layers, outs, exps):
    LT.assert_bit_equal(out.result(f'reduce_multi {c}'), exp, f'wgrad_partial + reduce_multi {c}', 'hwio')
  return routes


def _prep_multi_case():
  """se3ds_weight_prep_multi over layers whose K and cout are no multiples of 64 (k % 8 == 0,
  cout % 4 == 0): every wt / wn buffer sits between NaN guard words that must stay untouched."""
  L = _L()
  shapes = [(72, 4), (9 * 48, 160), (200, 36), (64, 64), (8, 132)]
  rows, bufs, keep, first = [], [], [], 0
  for i, (k, cout) in enumerate(shapes):
    w = LT.ternary((1, 1, k, cout), 977 * i + k)
    dw = dev(w)
    wt, wn = Guarded((cout, k), torch.bfloat16), Guarded((k, cout), torch.bfloat16)
    rows.append([dw.data_ptr(), k, cout, wt.ptr(), wn.ptr(), first])
    first += -(-k // 64) * -(-cout // 64)
    bufs.append((w, wt, wn))
    keep.append(dw)
  table = torch.tensor(rows, dtype=torch.int64).to(DEV)
  _lib.check(L.se3ds_weight_prep_multi(table.data_ptr(), len(rows), first, _lib.stream()), 'weight_prep_multi')
  routes = last_routes(1)
  for (k, cout), (w, wt, wn) in zip(shapes, bufs):
    wt_e, wn_e = LT.weight_operands(w)
    LT.assert_bit_equal(wt.result('wt'), wt_e, f'weight_prep_multi K {k} cout {cout} wt', 'flat')
    LT.assert_bit_equal(wn.result('wn'), wn_e, f'weight_prep_multi K {k} cout {cout} wn', 'flat')
  return routes


def _run(kind, case, dt, name=None):
  if kind == 'fwd':
    return run_fwd(case, dt)
  if kind == 'dgrad':
    return run_dgrad(case, dt)
  if kind == 'dgrad_bn':
    return run_dgrad_bn(case, dt)
  if kind == 'wgrad':
    return run_wgrad(case, dt)
  if kind == 'swapped':
    return run_swapped(case, dt, len(_SWAPPED[name]))
  if kind == 'prep':
    return run_prep(case, dt)
  if kind == 'reduce_multi':
    return _reduce_multi_case()
  if kind == 'prep_multi':
    return _prep_multi_case()
  raise ValueError(kind)


@pytest.mark.parametrize('name', sorted(ROUTES))
def test_route_is_reached_and_bit_exact(name, monkeypatch):
  kind, case, dt, env = ROUTES[name]
  _setenv(monkeypatch, env)
  print(f'route {name}: {kind} {dt} {case} {env}', flush=True)
  routes = _run(kind, case, dt, name)
  want = _expected_launches(name, kind)
  assert _same_launches(routes, want), f'{name}: the launches were {routes}, expected {want}'


def test_route_table_names_every_route():
  names = route_names()
  assert len(names) == len(set(names)) and len(names) >= 60
  assert sorted(ROUTES) == sorted(names), (sorted(set(names) - set(ROUTES)), sorted(set(ROUTES) - set(names)))
  assert _L().se3ds_debug_conv_route_name(-1) is None


# ---------------------------------------------------------------------------------------------
# shapes: ragged tiles, small channel counts, paddings, strides, masks, through the DEFAULT dispatch
# (the lists of tests/test_nets_gpu.py CONV_CASES / BIG_TILE_CASES / THIN_CASES / THIN_CIN_CASES plus
# the edges named in the issue); forward + data gradient + weight gradient each

SHAPES = [
    C(32, 64, 3, 1, 'VALID', 1, 2, 16, 32, epi='bias'),
    C(32, 64, 3, 1, 'VALID', 1, 1, 16, 32, wrap=1, pad_t=1, pad_l=1),
    C(64, 160, 3, 1, 'VALID', 1, 2, 8, 16, epi='scale'),
    C(32, 32, 4, 2, 'VALID', 2, 2, 18, 34, epi='bias_relu'),
    C(64, 32, 1, 1, 'SAME', 0, 2, 9, 17, epi='bias'),
    C(5, 16, 7, 2, 'VALID', 3, 2, 32, 64, mask='binary', epi='partial_bias'),
    C(32, 32, 3, 2, 'VALID', 1, 2, 16, 32, mask='binary', epi='partial_bias', row_scale=1),
    C(32, 128, 1, 2, 'SAME', 0, 2, 16, 32, mask='binary', epi='partial'),
    C(48, 32, 1, 1, 'SAME', 0, 1, 8, 16),
    C(4, 16, 4, 2, 'VALID', 2, 2, 32, 64, epi='bias'),
    C(64, 1, 4, 1, 'SAME', 0, 2, 10, 18, epi='bias'),
    C(8, 8, 3, 1, 'VALID', 1, 1, 12, 24),
    C(64, 3, 3, 1, 'VALID', 1, 2, 12, 20, epi='bias'),
    C(32, 1, 3, 1, 'VALID', 1, 2, 20, 36, epi='bias'),
    C(64, 256, 3, 1, 'VALID', 1, 2, 16, 32, epi='bias'),
    C(128, 128, 3, 1, 'VALID', 1, 1, 16, 32, wrap=1, pad_t=1, pad_l=1),
    C(256, 256, 1, 1, 'SAME', 0, 2, 9, 17, epi='bias'),
    C(128, 256, 4, 2, 'VALID', 2, 2, 18, 34, epi='bias'),
    C(64, 128, 3, 2, 'VALID', 1, 2, 16, 32, mask='binary', epi='partial_bias'),
    C(128, 128, 3, 1, 'VALID', 1, 2, 16, 32, mask='binary', epi='partial_bias'),
    C(512, 256, 3, 1, 'VALID', 1, 3, 11, 23, epi='bias'),
    C(192, 128, 3, 1, 'VALID', 1, 1, 20, 70, epi='bias'),
    C(64, 128, 3, 1, 'SAME', 0, 2, 8, 32),
    C(64, 128, 3, 1, 'VALID', 1, 3, 128, 256, epi='bias'),
    C(128, 256, 3, 1, 'VALID', 1, 3, 128, 256, epi='bias_leaky'),
    C(128, 3, 3, 1, 'VALID', 1, 2, 12, 64, epi='bias'),
    C(128, 1, 3, 1, 'VALID', 1, 2, 9, 37, epi='bias'),
    C(64, 3, 3, 1, 'VALID', 1, 1, 16, 32, wrap=1, pad_t=1, pad_l=1),
    C(256, 4, 3, 1, 'SAME', 0, 1, 7, 45, epi='bias'),
    C(96, 2, 3, 1, 'VALID', 1, 1, 20, 70),
    C(5, 128, 7, 2, 'VALID', 3, 2, 32, 64, mask='binary', epi='partial_bias'),
    C(4, 128, 4, 2, 'VALID', 2, 2, 34, 66, epi='bias'),
    C(4, 256, 3, 1, 'VALID', 1, 1, 12, 40, wrap=1, pad_t=1, pad_l=1),
    C(8, 128, 3, 2, 'VALID', 1, 3, 19, 45, epi='bias'),
    C(3, 128, 4, 2, 'VALID', 2, 1, 70, 130),
    C(4, 128, 4, 2, 'VALID', 0, 2, 20, 36, epi='bias'),
    # edges: one pixel row, n = 1, odd sizes under stride 2 (both parities / one parity empty),
    # asymmetric explicit padding 0..3, ragged cin / cout, one and several K steps
    C(64, 128, 3, 1, 'SAME', 0, 1, 1, 45, epi='bias'),
    C(128, 64, 4, 2, 'VALID', 2, 1, 33, 65, epi='bias'),
    C(64, 48, 3, 2, 'VALID', 1, 1, 1, 9),
    C(96, 16, 3, 1, 'VALID', 0, 2, 9, 17, pad_t=0, pad_l=3, epi='scale'),
    C(192, 160, 3, 1, 'VALID', 1, 1, 9, 17, pad_t=2, pad_l=0),
    C(48, 48, 5, 1, 'SAME', 0, 1, 11, 23, pad_t=3, pad_l=1, epi='bias'),
    C(5, 2, 3, 1, 'SAME', 0, 2, 9, 17, mask='plain', epi='partial_bias'),
    C(4, 4, 1, 1, 'SAME', 0, 1, 20, 70, epi='bias'),
    C(32, 4, 1, 1, 'SAME', 0, 3, 128, 256),
]


def _three(c, dt):
  run_fwd(c, dt)
  d = {k: v for k, v in c.items() if k not in ('epi', 'mask')}
  epi = c.get('epi', 'none')
  d['epi'] = 'row_a' if c.get('mask') else (epi if epi in ('scale', 'bias', 'bias_relu') else 'none')
  run_dgrad(d, dt)
  run_wgrad({k: v for k, v in c.items() if k != 'epi'}, dt)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('i', range(len(SHAPES)))
def test_shapes_default_dispatch(i, dt, monkeypatch):
  _setenv(monkeypatch, {})
  _three(SHAPES[i], dt)


@pytest.mark.parametrize('i', [5, 6, 18, 19, 30])
def test_binary_mask_promise_changes_no_bit(i, monkeypatch):
  """in_mask_binary = 0 / 1 on the same binary mask (with a fully masked band) route to different
  kernels; both are held to the same expected bits, forward and weight gradient."""
  _setenv(monkeypatch, {})
  for m in ('binary', 'plain'):
    c = dict(SHAPES[i], mask=m)
    run_fwd(c, 'bf16')
    run_wgrad({k: v for k, v in c.items() if k != 'epi'}, 'bf16')


@pytest.mark.parametrize('c', [
    C(64, 128, 3, 1, 'VALID', 1, 2, 16, 32, epi='bias'),           # halo, 128 channels
    C(64, 1024, 3, 1, 'VALID', 1, 1, 61, 250, epi='bias_relu'),    # halo, 256 channels
    C(64, 256, 1, 1, 'SAME', 0, 1, 128, 512),                      # 256-pixel macro tile
    C(128, 128, 4, 2, 'VALID', 2, 2, 18, 34, mask='binary', epi='partial_bias'),   # 128 x 128
], ids=lambda c: f"{c['cin']}-{c['cout']}-k{c['k']}s{c['stride']}")
def test_fwd_stats_columns(c, monkeypatch):
  _setenv(monkeypatch, {})
  run_fwd(c, 'bf16', stats=True)


@pytest.mark.parametrize('c', [C(32, 64, 1, 1, 'SAME', 0, 2, 9, 17, epi='bias'),
                               C(128, 48, 1, 1, 'SAME', 0, 1, 20, 70),
                               C(64, 4, 1, 1, 'SAME', 0, 3, 11, 23, epi='bias')],
                         ids=lambda c: f"{c['cin']}-{c['cout']}")
@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_conv_transpose2x2(c, dt, monkeypatch):
  _setenv(monkeypatch, {})
  routes = run_convt(c, dt)
  assert routes[0] == routes[1] and routes[0] is not None, routes


# ---------------------------------------------------------------------------------------------
# production shapes (tests/test_prod_shapes_gpu.py PROD_CONVS) at the smallest listed batch,
# default dispatch, bf16 and fp32: forward, data gradient, weight gradient bit-exact

def _prod_case(row):
  name, kind, cin, cout, k, stride, padding, pad, bias, use_mask, h, w, batches, _ = row
  c = C(cin, cout, k, stride, padding, pad, min(batches), h, w)
  if use_mask:
    c['mask'] = 'binary'
  c['epi'] = ('partial_bias' if bias else 'partial') if kind.startswith('partial') else (
      'bias' if bias else ('scale' if kind == 'spectral' else 'none'))
  return c


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('row', PROD_CONVS, ids=[r[0].replace(' ', '_') for r in PROD_CONVS])
def test_production_shape(row, dt, monkeypatch):
  _setenv(monkeypatch, {})
  c = _prod_case(row)
  print(f'production shape {row[0]}: {c}', flush=True)
  _three(c, dt)


# ---------------------------------------------------------------------------------------------
# the Python-side routing (se3ds_amd/hipops/nn.py): nn.conv2d / nn.conv_transpose2d on plain layers,
# forward + backward, with the weight gradients' split reductions run per layer (ctx.wgrad_defer =
# None: what SE3DS_DEFER_WGRAD_REDUCE=0 selects in the trainer) and deferred into ONE
# se3ds_wgrad_reduce_multi launch (nn._wgrad, reduce_or_defer, flush_wgrad_reduces), and the 2x2
# transposed conv through se3ds_conv_transpose2x2_fwd and through the parity-class data gradient
# (SE3DS_CONVT_2X2 = nn._CONVT_2X2).  Same references, same `==`.

from se3ds_amd.hipops import nn  # noqa: E402

# name, cin, cout, k, stride, padding, pad, n, h, w
NN_LAYERS = [
    # (first: its backward runs last, so its launches are still in the route ring afterwards)
    ('e', 5, 3, 3, 2, 'VALID', 1, 2, 9, 17),          # 135 elements: no 16-byte reduction, never deferred
    ('a', 64, 128, 3, 1, 'VALID', 1, 3, 11, 23),      # tap-fused weight gradient, several splits
    ('b', 128, 256, 4, 2, 'VALID', 2, 2, 18, 34),     # LDS-DMA weight gradient, parity classes
    ('c', 5, 128, 7, 2, 'VALID', 3, 2, 32, 64),       # thin-cin weight gradient: one slab per workgroup
    ('d', 48, 32, 1, 1, 'SAME', 0, 1, 8, 16),         # ragged reduction channels
]


def _count_flushed_rows(monkeypatch):
  """Records how many rows each batched reduction (nn._reduce_rows) is given, then runs it."""
  seen, real = [], nn._reduce_rows

  def counting(ctx, rows):
    seen.append(len(rows))
    return real(ctx, rows)
  monkeypatch.setattr(nn, '_reduce_rows', counting)
  return seen


def _launch_log(count):
  return [r for r in last_routes(count) if r is not None]


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('defer', [False, True], ids=['reduce_per_layer', 'reduce_deferred'])
def test_nn_conv2d_weight_gradient_reductions(defer, dt, monkeypatch):
  """Five plain layers in one parameter store.  The gradient arena is filled with NaN first: a
  layer whose reduction is dropped keeps NaN, one reduced twice or into the wrong place differs by
  an integer.  Deferred: no reduction may launch before the flush (except the ragged layer's own,
  which the 16-byte kernel cannot take), then exactly one wgrad_reduce_multi over four rows (the
  flush at the end of ctx.backward())."""
  _setenv(monkeypatch, {})
  T = _DT[dt]
  store = nn.ParamStore()
  layers = {name: nn.ConvLayer(store, name, cin, cout, k, s, padding, True, 'plain')
            for name, cin, cout, k, s, padding, pad, n, h, w in NN_LAYERS}
  store.finalize(DEV, torch.Generator().manual_seed(3))
  cases, load = {}, {}
  for name, cin, cout, k, s, padding, pad, n, h, w in NN_LAYERS:
    c = C(cin, cout, k, s, padding, pad, n, h, w, epi='bias')
    cases[name] = c
    load[name + '/kernel'] = LT.ternary((k, k, cin, cout), _seed(c, 2)).numpy()
    load[name + '/bias'] = LT.bias_ints(cout, _seed(c, 5)).numpy()
  store.load_dict(load)
  store.grad.fill_(float('nan'))
  ctx = nn.Ctx(DEV, T, training=False, record=True)
  ctx.wgrad_defer = [] if defer else None
  xs, ys, exp = {}, {}, {}
  for name, cin, cout, k, s, padding, pad, n, h, w in NN_LAYERS:
    c = cases[name]
    ho, wo, pt, pl = geom(c)
    x, dy = LT.ternary((n, h, w, cin), _seed(c, 1)), LT.ternary((n, ho, wo, cout), _seed(c, 11))
    kern, bias = torch.from_numpy(load[name + '/kernel']), torch.from_numpy(load[name + '/bias'])
    y, pre, q = LT.conv2d_fwd(x, kern, ho, wo, s, pt, pl, 0, None, None, bias)
    dxe, dpre, dq = LT.conv2d_dgrad(dy, kern, (n, h, w, cin), s, pt, pl)
    exp[name] = (_expected_stored(y, pre, q, dt, f'nn fwd {name}'),
                 _expected_stored(dxe, dpre, dq, dt, f'nn dgrad {name}'),
                 LT.conv2d_wgrad(x, dy, (k, k, cin, cout), s, pt, pl), dy.reshape(-1, cout).sum(0))
    xs[name] = nn.Var(dev(x, T), requires_grad=True)
    ys[name] = nn.conv2d(ctx, xs[name], layers[name], pad=pad)
    ys[name].grad = dev(dy, T)
  flushed = _count_flushed_rows(monkeypatch)
  ctx.backward()
  if defer:
    # layers a..d deferred their reduction and ctx.backward() flushed the four rows as ONE launch at
    # its end; e ran its own (scalar) reduction; no per-layer 16-byte reduction ran
    assert flushed == [4] and ctx.wgrad_defer == [], (flushed, ctx.wgrad_defer)
    log = _launch_log(8)
    assert log[-1] == 'wgrad_reduce_multi' and log.count('wgrad_reduce_multi') == 1 and \
        log.count('wgrad_reduce_scalar') == 1 and 'wgrad_reduce_vec' not in log, log
    nn.flush_wgrad_reduces(ctx)                       # nothing left: no second launch
    assert flushed == [4] and last_routes(2)[0] != 'wgrad_reduce_multi'
  else:
    log = _launch_log(8)
    assert flushed == [] and 'wgrad_reduce_multi' not in log and log.count('wgrad_reduce_vec') >= 1, log
  torch.cuda.synchronize()
  for name, cin, cout, k, s, padding, pad, n, h, w in NN_LAYERS:
    ye, dxe, dwe, dbe = exp[name]
    what = f'nn.conv2d {name} {dt} defer={defer}'
    LT.assert_bit_equal(ys[name].data.float().cpu(), ye, what + ' y')
    LT.assert_bit_equal(xs[name].grad.float().cpu(), dxe, what + ' dx')
    LT.assert_bit_equal(store.grad_views[name + '/kernel'].cpu(), dwe, what + ' dW', 'hwio')
    LT.assert_bit_equal(store.grad_views[name + '/bias'].cpu(), dbe, what + ' db', 'flat')


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('defer', [False, True], ids=['reduce_per_layer', 'reduce_deferred'])
@pytest.mark.parametrize('two_by_two', [True, False], ids=['convt2x2', 'parity_dgrad'])
def test_nn_conv_transpose2d(two_by_two, defer, dt, monkeypatch):
  """Keras Conv2DTranspose k2 s2 through nn.conv_transpose2d, forward + backward: the pitched 1x1
  form (se3ds_conv_transpose2x2_fwd: two launches of one forward route) and, with nn._CONVT_2X2 off,
  the parity-class data-gradient kernel (one launch of a dgrad route)."""
  _setenv(monkeypatch, {})
  monkeypatch.setattr(nn, '_CONVT_2X2', two_by_two)
  T = _DT[dt]
  cin, cout, n, h, w = 64, 48, 2, 9, 17
  c = C(cin, cout, 2, 2, 'SAME', 0, n, h, w)
  store = nn.ParamStore()
  layer = nn.ConvLayer(store, 't', cin, cout, 2, 2, 'SAME', True, 'plain', transpose=True)
  store.finalize(DEV, torch.Generator().manual_seed(4))
  kern, bias = LT.ternary((2, 2, cout, cin), _seed(c, 2)), LT.bias_ints(cout, _seed(c, 5))
  store.load_dict({'t/kernel': kern.numpy(), 't/bias': bias.numpy()})
  store.grad.fill_(float('nan'))
  x, dy = LT.ternary((n, h, w, cin), _seed(c, 1)), LT.ternary((n, 2 * h, 2 * w, cout), _seed(c, 11))
  y = LT.conv_transpose2x2(x, kern, bias)
  # backward = the associated forward conv (2h, 2w, cout) -> (h, w, cin), kernel HWIO = (2, 2, cout, cin)
  dxa = LT.conv_acc(dy, kern, h, w, 2, 0, 0)
  dwe = LT.conv2d_wgrad(dy, x, (2, 2, cout, cin), 2, 0, 0)
  ctx = nn.Ctx(DEV, T, training=False, record=True)
  ctx.wgrad_defer = [] if defer else None
  xv = nn.Var(dev(x, T), requires_grad=True)
  out = nn.conv_transpose2d(ctx, xv, layer)
  fwd = last_routes(2)
  if two_by_two:
    assert fwd[0] == fwd[1] and '_fwd' in fwd[1], fwd
  else:
    assert '_dgrad' in fwd[1], fwd
  out.grad = dev(dy, T)
  flushed = _count_flushed_rows(monkeypatch)
  ctx.backward()
  log = _launch_log(4)
  if defer:   # the layer's row went into the one batched launch at the end of the backward pass
    assert flushed == [1] and ctx.wgrad_defer == [], (flushed, ctx.wgrad_defer)
    assert log[-1] == 'wgrad_reduce_multi' and not any(r in _R for r in log), log
  else:
    assert flushed == [] and any(r in _R for r in log) and 'wgrad_reduce_multi' not in log, log
  what = f'nn.conv_transpose2d {dt} 2x2={two_by_two} defer={defer}'
  LT.assert_bit_equal(out.data.float().cpu(), _expected_stored(y, y, 1.0, dt, what), what + ' y')
  LT.assert_bit_equal(xv.grad.float().cpu(), _expected_stored(dxa, dxa, 1.0, dt, what), what + ' dx')
  LT.assert_bit_equal(store.grad_views['t/kernel'].cpu(), dwe, what + ' dW', 'hwio')
  LT.assert_bit_equal(store.grad_views['t/bias'].cpu(), dy.reshape(-1, cout).sum(0), what + ' db', 'flat')
