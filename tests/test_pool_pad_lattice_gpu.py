"""Bit-exact lattice tests of the pooling, pad, copy and small pointwise kernels of
se3ds_amd/csrc/pointwise.hip, straight through the C ABI.  References: tests/_lattice.py (NumPy
float64, pinned without a GPU by tests/test_lattice_cpu.py, which also builds every case below).

Compared with LT.assert_bit_equal, every element: maxpool2x2 forward and backward (inputs are
integers in [-2, 2] with runs of zeros and some -0.0, so ties for the maximum -- whole-window ties
included -- are frequent and the "first maximum in row-major window order" rule decides),
avgpool3s2 forward and backward on the lattice 36 * {-3..3} (36 = lcm(4, 6, 9): every quotient is
an integer) plus one plain-integer forward case (one correctly rounded division), upsample2x,
pad2d (CONSTANT / REFLECT / SYMMETRIC, wrap_w), copy_channels (all four dtype pairs, unaligned
offsets, fp32 -> bf16 ties), row_scale, add, act_bwd, fill, and `um` of mask_window.
mask_window's ratio / ru / bu: equal to the documented formula where cnt = 0, elsewhere
|kernel - float64| <= K * 2^-24 * magnitude, K = LT.K_RATIO / K_BU counted roundings; the share
of elements equal to the formula evaluated with one fp32 rounding per operation is printed.

Measured on an MI355X: 100 % (12672 of 12672) of mask_window's ratio / ru / bu equal the formula
evaluated with one fp32 rounding per operation, the largest bound ratio is 0.78; the module takes
well under a second of wall time.
"""
import numpy as np
import pytest
import torch

from se3ds_amd import _lib
import se3ds_amd.hipops  # noqa: F401  registers the signatures
import _lattice as LT

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32, BF16 = _lib.F32, _lib.BF16
N = 2
POOL_HW = ((1, 1), (2, 2), (5, 7), (6, 8), (1, 9))
POOL_C = (8, 16, 12)          # bf16: 8 and 16 take the vec8 backward, 12 the scalar one
LENGTHS = (1, 7, 256 + 5, 256 * 3 + 5, 256 * 3 + 8, 256 * 17 + 5)



def _L():
  return _lib.lib()


def dev(a, bf16=False):
  if a is None:
    return None
  t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)
  return t.bfloat16() if bf16 else t


def blank(shape, bf16=False):
  return torch.full(tuple(shape), float('nan'), device=DEV,
                    dtype=torch.bfloat16 if bf16 else torch.float32)


def host(t):
  return t.float().cpu().numpy()


def p(t):
  return _lib.ptr(t)


def code(bf16):
  return BF16 if bf16 else F32


def ok(rc, what):
  assert rc == 0, f'{what}: rc {rc} {_L().se3ds_last_error().decode()}'


def pool_cases():
  return [dict(h=h, w=w, c=c, bf16=bf16) for bf16 in (False, True) for (h, w) in POOL_HW for c in POOL_C]


# ---------------------------------------------------------------------------------------------
def build_maxpool(k, seed=0):
  h, w, c = k['h'], k['w'], k['c']
  x = LT.tie_ints((N, h, w, c), 100 + seed)
  neg = (x == 0) & (LT.rng(101 + seed).random(x.shape) < 0.3)
  x[neg] = -0.0
  y = LT.maxpool2x2_fwd(x)
  dy = LT.small_ints(y.shape, 102 + seed, 1, 3) * LT.rng(103 + seed).choice((-1.0, 1.0), y.shape)
  dx, share = LT.maxpool2x2_bwd(dy, x)
  return dict(x=x, dy=dy), dict(y=LT.f32(y), dx=LT.f32(dx), tie_share=share)


def test_maxpool2x2():
  for i, k in enumerate(pool_cases()):
    h, w, c, bf16 = k['h'], k['w'], k['c'], k['bf16']
    inp, exp = build_maxpool(k, i)
    x, dy = dev(inp['x'], bf16), dev(inp['dy'], bf16)
    y = blank(exp['y'].shape, bf16)
    ok(_L().se3ds_maxpool2x2_fwd(p(x), code(bf16), N, h, w, c, p(y), _lib.stream()), f'maxpool fwd {k}')
    LT.assert_bit_equal(host(y), exp['y'], f'maxpool2x2_fwd {k}')
    dx = blank((N, h, w, c), bf16)
    ok(_L().se3ds_maxpool2x2_bwd(p(dy), p(x), p(y), code(bf16), N, h, w, c, p(dx), _lib.stream()),
       f'maxpool bwd {k}')
    LT.assert_bit_equal(host(dx), exp['dx'], f'maxpool2x2_bwd {k} (ties in {exp["tie_share"]:.2f} of windows)')


def build_avgpool(k, seed=0):
  h, w, c, bf16 = k['h'], k['w'], k['c'], k['bf16']
  x = 36.0 * LT.small_ints((N, h, w, c), 200 + seed, -3, 3)
  y = LT.avgpool3s2_fwd(x, bf16)
  dy = 36.0 * LT.small_ints(y.shape, 201 + seed, -3, 3)
  xi = LT.small_ints((N, h, w, c), 202 + seed, -8, 8)
  return dict(x=x, dy=dy, xi=xi), dict(y=y, dx=LT.avgpool3s2_bwd(dy, h, w, bf16),
                                       yi=LT.avgpool3s2_fwd(xi, bf16, lattice36=False))


def test_avgpool3s2():
  for i, k in enumerate(pool_cases()):
    h, w, c, bf16 = k['h'], k['w'], k['c'], k['bf16']
    inp, exp = build_avgpool(k, i)
    for xin, e, name in ((inp['x'], exp['y'], '36-lattice'), (inp['xi'], exp['yi'], 'plain integers')):
      y, xd = blank(e.shape, bf16), dev(xin, bf16)
      ok(_L().se3ds_avgpool3s2_fwd(p(xd), code(bf16), N, h, w, c, p(y), _lib.stream()),
         f'avgpool fwd {k}')
      LT.assert_bit_equal(host(y), e, f'avgpool3s2_fwd {name} {k}')
    dx, dyd = blank((N, h, w, c), bf16), dev(inp['dy'], bf16)
    ok(_L().se3ds_avgpool3s2_bwd(p(dyd), code(bf16), N, h, w, c, p(dx), _lib.stream()),
       f'avgpool bwd {k}')
    LT.assert_bit_equal(host(dx), exp['dx'], f'avgpool3s2_bwd {k}')


def build_upsample(k, seed=0):
  h, w, c = k['h'], k['w'], k['c']
  x = LT.small_ints((N, h, w, c), 300 + seed, -4, 4)
  dy = LT.small_ints((N, 2 * h, 2 * w, c), 301 + seed, -2, 2)
  return dict(x=x, dy=dy), dict(y=LT.f32(LT.upsample2x_fwd(x)), dx=LT.upsample2x_bwd(dy, k['bf16']))


def test_upsample2x():
  for i, k in enumerate(pool_cases()):
    h, w, c, bf16 = k['h'], k['w'], k['c'], k['bf16']
    inp, exp = build_upsample(k, i)
    y, dx = blank((N, 2 * h, 2 * w, c), bf16), blank((N, h, w, c), bf16)
    xd, dyd = dev(inp['x'], bf16), dev(inp['dy'], bf16)
    ok(_L().se3ds_upsample2x_fwd(p(xd), code(bf16), N, h, w, c, p(y), _lib.stream()), f'up {k}')
    ok(_L().se3ds_upsample2x_bwd(p(dyd), code(bf16), N, h, w, c, p(dx), _lib.stream()), f'up {k}')
    LT.assert_bit_equal(host(y), exp['y'], f'upsample2x_fwd {k}')
    LT.assert_bit_equal(host(dx), exp['dx'], f'upsample2x_bwd {k}')


# ---------------------------------------------------------------------------------------------
PAD_VALUE = 1.5


def pad_cases():
  return [dict(h=h, w=w, c=c, pad=pad, mode=mode, wrap=wrap, bf16=bf16)
          for bf16 in (False, True) for (h, w, c) in ((4, 5, 3), (5, 4, 8)) for pad in (1, 3)
          for mode in (0, 1, 2) for wrap in (0, 1)]


def build_pad(k, seed=0):
  x = LT.small_ints((N, k['h'], k['w'], k['c']), 400 + seed, -4, 4)
  assert k['pad'] < min(k['h'], k['w'])          # REFLECT reads index pad, wrap_w index w - pad
  return dict(x=x), dict(y=LT.f32(LT.pad2d(x, k['pad'], k['mode'], k['wrap'], PAD_VALUE)))


def test_pad2d():
  for i, k in enumerate(pad_cases()):
    inp, exp = build_pad(k, i)
    y, xd = blank(exp['y'].shape, k['bf16']), dev(inp['x'], k['bf16'])
    ok(_L().se3ds_pad2d(p(xd), code(k['bf16']), N, k['h'], k['w'], k['c'], k['pad'],
                        k['mode'], k['wrap'], PAD_VALUE, p(y), _lib.stream()), f'pad2d {k}')
    LT.assert_bit_equal(host(y), exp['y'], f'pad2d {k}')


def copy_cases():
  return [dict(sb=sb, db=db, ncopy=n, rows=37, src_c=13, src_c0=3, dst_c=11, dst_c0=2)
          for sb in (False, True) for db in (False, True) for n in (1, 3, 8)]


def build_copy(k, seed=0):
  # fp32 sources carry multiples of 1 / 256 up to 4: the conversion to bf16 rounds, ties included
  src = LT.small_ints((k['rows'], k['src_c']), 500 + seed, -1024, 1024) / 256.0
  src = LT.rne_np(src, k['sb']).astype(np.float64)
  dst = LT.small_ints((k['rows'], k['dst_c']), 501 + seed, 5, 9)
  return dict(src=src, dst=dst), dict(dst=LT.f32(LT.copy_channels(src, k['src_c0'], dst, k['dst_c0'],
                                                                   k['ncopy'], k['db'])))


def test_copy_channels():
  for i, k in enumerate(copy_cases()):
    inp, exp = build_copy(k, i)
    src, dst = dev(inp['src'], k['sb']), dev(inp['dst'], k['db'])
    ok(_L().se3ds_copy_channels(p(src), code(k['sb']), k['src_c'], k['src_c0'], p(dst), code(k['db']), k['dst_c'],
                                k['dst_c0'], k['ncopy'], k['rows'], _lib.stream()), f'copy_channels {k}')
    LT.assert_bit_equal(host(dst), exp['dst'], f'copy_channels {k}', 'flat')
  assert _L().se3ds_copy_channels(p(src), F32, 13, 10, p(dst), F32, 11, 2, 8, 37, _lib.stream()) == -1


def build_pointwise(n, bf16, seed=0):
  a, b = LT.small_ints((n,), 600 + seed, -4, 4, 0.3), LT.small_ints((n,), 601 + seed, -4, 4)
  out = dict(add=LT.add(a, b, bf16))
  for act in (0, 1, 2):
    out[f'act{act}'] = LT.act_bwd(b, a, act, 0.5, bf16)
  return dict(a=a, b=b), out


def test_add_act_bwd_fill():
  for bf16 in (False, True):
    for i, n in enumerate(LENGTHS):
      inp, exp = build_pointwise(n, bf16, i)
      a, b = dev(inp['a'], bf16), dev(inp['b'], bf16)
      o = blank((n,), bf16)
      ok(_L().se3ds_add(p(a), p(b), code(bf16), n, p(o), _lib.stream()), f'add {n}')
      LT.assert_bit_equal(host(o), exp['add'], f'add n {n} bf16 {bf16}', 'flat')
      for act in (0, 1, 2):
        o = blank((n,), bf16)
        ok(_L().se3ds_act_bwd(p(b), p(a), code(bf16), n, act, 0.5, p(o), _lib.stream()), f'act_bwd {n}')
        LT.assert_bit_equal(host(o), exp[f'act{act}'], f'act_bwd n {n} act {act} bf16 {bf16}', 'flat')
      o = dev(np.full(n + 8, 7.0), bf16)
      ok(_L().se3ds_fill(p(o), code(bf16), n, PAD_VALUE, _lib.stream()), f'fill {n}')
      LT.assert_bit_equal(host(o), np.r_[np.full(n, PAD_VALUE), np.full(8, 7.0)], f'fill n {n} bf16 {bf16}', 'flat')


def row_scale_cases():
  return [dict(rows=rows, c=c, bf16=bf16) for bf16 in (False, True) for rows in (1, 7, 261) for c in (1, 8, 12, 773)]


def build_row_scale(k, seed=0):
  x = LT.small_ints((k['rows'], k['c']), 700 + seed, -4, 4)
  s = LT.signed_pow2((k['rows'],), 701 + seed)
  s[0] = 0.5
  return dict(x=x, s=s), dict(y=LT.row_scale(x, s, k['bf16']))


def test_row_scale():
  for i, k in enumerate(row_scale_cases()):
    inp, exp = build_row_scale(k, i)
    y, xd, sd = blank((k['rows'], k['c']), k['bf16']), dev(inp['x'], k['bf16']), dev(inp['s'])
    ok(_L().se3ds_row_scale(p(xd), code(k['bf16']), k['rows'], k['c'], p(sd),
                            p(y), _lib.stream()), f'row_scale {k}')
    LT.assert_bit_equal(host(y), exp['y'], f'row_scale {k}', 'flat')


# ---------------------------------------------------------------------------------------------
MW_H, MW_W = 24, 12


def mask_cases():
  return [dict(k=kk, stride=s, wrap=wrap) for (kk, s) in ((1, 1), (3, 1), (3, 2), (4, 2), (7, 2)) for wrap in (0, 1)]


def build_mask(k, seed=0):
  m = (LT.rng(800 + seed).random((N, MW_H, MW_W)) > 0.3).astype(np.float64)
  m[:, 8:16] = 0.0                      # an all-zero band: windows with cnt = 0
  m[:, 16:] = 1.0                       # a hole-free region: full windows
  ho, pt = LT.out_size(MW_H, k['k'], k['stride'], 'SAME')
  wo, pl = LT.out_size(MW_W, k['k'], k['stride'], 'SAME')
  assert k['k'] - 1 <= MW_W              # the circular W index wraps at most once
  exp = LT.mask_window(m, ho, wo, k['k'], k['k'], k['stride'], pt, pl, k['wrap'])
  assert (exp['cnt'] == 0).any() and (exp['cnt'] == k['k'] ** 2).any()
  return dict(mask=m, ho=ho, wo=wo, pt=pt, pl=pl), exp


def test_mask_window():
  same = total = 0
  worst = 0.0
  for i, k in enumerate(mask_cases()):
    inp, exp = build_mask(k, i)
    ho, wo = inp['ho'], inp['wo']
    m = dev(inp['mask'])
    for with_b in (False, True):
      o = {n: blank((N, ho, wo)) for n in ('ratio', 'um', 'ru', 'bu')}
      ok(_L().se3ds_mask_window(p(m), N, MW_H, MW_W, ho, wo, k['k'], k['k'], k['stride'], inp['pt'], inp['pl'],
                                k['wrap'], p(o['ratio']), p(o['um']), p(o['ru']) if with_b else None,
                                p(o['bu']) if with_b else None, _lib.stream()), f'mask_window {k}')
      got = {n: host(t) for n, t in o.items()}
      LT.assert_bit_equal(got['um'], exp['um'], f'mask_window um {k}', 'flat')
      names = (('ratio', LT.K_RATIO, 'ratio'),) + ((('ru', LT.K_RATIO, 'ratio'), ('bu', LT.K_BU, 'bu')) if with_b else ())
      zero = exp['cnt'] == 0
      for name, kk, mag in names:
        assert np.array_equal(got[name][zero], LT.f32(exp[name])[zero]), f'mask_window {name} {k}: cnt = 0'
        ratio = LT.bound_ratio(got[name], exp[name], kk, exp['mag_' + mag])
        worst = max(worst, ratio)
        assert ratio <= 1.0, f'mask_window {name} {k}: {ratio:.3f} x the {kk}-rounding bound'
      same += int((got['ratio'] == exp['ratio32']).sum())
      total += got['ratio'].size
      if with_b:
        same += int((got['bu'] == exp['bu32']).sum()) + int((got['ru'] == exp['ratio32']).sum())
        total += 2 * got['bu'].size
  print(f'mask_window: {same} / {total} = {100.0 * same / total:.2f} % of ratio / ru / bu equal the formula '
        f'with one fp32 rounding per operation; largest bound ratio {worst:.3f}')


# ---------------------------------------------------------------------------------------------
def build_all():
  """Builds every case of this module and runs the references' preconditions (no GPU).  Returns
  (number of cases, share of max-pool windows with a tie for the maximum)."""
  n = 0
  shares = []
  for i, k in enumerate(pool_cases()):
    shares.append(build_maxpool(k, i)[1]['tie_share'] if k['h'] * k['w'] > 1 else None)
    build_avgpool(k, i)
    build_upsample(k, i)
    n += 3
  for table, fn in ((pad_cases(), build_pad), (copy_cases(), build_copy), (row_scale_cases(), build_row_scale),
                    (mask_cases(), build_mask)):
    for i, k in enumerate(table):
      fn(k, i)
      n += 1
  for bf16 in (False, True):
    for i, ln in enumerate(LENGTHS):
      build_pointwise(ln, bf16, i)
      n += 1
  shares = [s for s in shares if s is not None]
  return n, float(np.mean(shares)), float(np.min(shares))
