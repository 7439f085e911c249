"""Bit-exact lattice tests of the Inception-v3 evaluator (se3ds_amd/utils/inception_utils.py,
se3ds_amd/csrc/inception.hip), straight through the C ABI with the runners of
tests/test_conv_lattice_gpu.py.  References: tests/_lattice.py and plain NumPy float64 / int64;
tests/test_lattice_cpu.py builds every case below (build_all) without a GPU.

Convolutions: every distinct (cin, cout, kh, kw, stride, padding) of iu.conv_specs() and the dense
layer, with the real channel counts, the evaluator's geometry ('same': pad (kh-1)//2, (kw-1)//2;
'valid': 0) and its epilogue (bias + ReLU; the dense layer bias only), n = 2, ternary operands,
integer bias, NaN guard bands, `==` on every element, bf16 and fp32.  Maps: the evaluator's own where
it is at most 35 (35, 17, 8), 23 x 19 for the stem; every kh != kw spec also on 17 x 13.  The
non-square specs (and three of them through the data and weight gradients, which no caller uses
with kh != kw yet) are the only bit-exact cases anywhere whose kernel is not square.  The route of
every launch is recorded and the last test prints the (spec, dtype, route) table.

The glue: InceptionV3._prep's operand against LT.weight_operands, the channel concatenations of
every block layout through _Device._dense against torch.cat, the two pooling kernels, the global
average pool and the feature moments with `==`; the softmax with `==` where the result is
determined (constant rows, one-hot rows) and within 8 x the error of a plain fp32 NumPy
restatement elsewhere (the device expf is not specified to the bit).

Measured on an MI355X (default dispatch), forward routes of the kh != kw classes: bf16 128 -> 128
glds_bf16_fwd_m16, 128 -> 192 and 192 -> 192 glds_bf16_fwd_m32 (ragged channel tile), every cin 160
layer igemm_bf16_fwd, 384 -> 384 1x3 / 3x1 glds_bf16_fwd_m16, the synthetic cin 24 / 40 layers
igemm_bf16_fwd; fp32 every evaluator layer glds_f32_fwd, the synthetic ones igemm_f32_fwd; 448 ->
384 3x3 at 8x8 halo128_fwd_m16 (bf16).  Backward: dgrad glds_bf16_dgrad_m16 (128 1x7, 384 1x3),
igemm_bf16_dgrad (160 7x1), glds_f32_dgrad in fp32; wgrad wgrad_glds_bf16 / wgrad_glds_f32 +
wgrad_reduce_vec.  Every case was bit-equal on the first run: no kernel or entry point changed.
Softmax: the fp32 restatement's error against float64 is 7.3e-9 .. 2.0e-7 (0 for c = 1), the
kernel's largest error 2.8e-7, the largest kernel / floor ratio 7.46 (1 x 65, fp32, +-80: floor
1.1e-8) against the bound of 8; bf16 inputs 3.73.  The module (94 tests) takes 2.9 s of wall time,
the slowest test 0.8 s.
"""
import types

import numpy as np
import pytest
import torch

from se3ds_amd import _lib
import se3ds_amd.hipops  # noqa: F401  registers the conv / copy signatures
from se3ds_amd.utils import inception_utils as iu
import _lattice as LT
import test_conv_lattice_gpu as CL

pytestmark = pytest.mark.gpu
DEV = CL.DEV
_DT = CL._DT
DTS = ('bf16', 'f32')
STEM_MAP, NONSQUARE_MAP = (23, 19), (17, 13)
DENSE_SPEC = (iu.POOL_DIM, iu.NUM_CLASSES, 1, 1, 1, 'valid')


def _L():
  return _lib.lib()


# ---------------------------------------------------------------------------------------------
# convolution cases, derived from the evaluator's own architecture function

class _Maps(iu._Specs):
  """iu._Specs that also records the (h, w) every conv reads."""

  def __init__(self):
    super().__init__()
    self.maps = []

  def conv_bn(self, x, cout, kh, kw, stride=1, padding='same'):
    self.maps.append((x[0], x[1]))
    return super().conv_bn(x, cout, kh, kw, stride, padding)


def traced_specs():
  """{spec: [maps it runs at]} in order of first use; the specs are iu.conv_specs()."""
  t = _Maps()
  iu._architecture(t, (iu.INPUT_SIZE, iu.INPUT_SIZE, 3))
  assert t.convs == iu.conv_specs()
  out = {}
  for spec, hw in zip(t.convs, t.maps):
    out.setdefault(spec, [])
    if hw not in out[spec]:
      out[spec].append(hw)
  return out


def device_geometry(spec, h, w):
  """(ho, wo, pad_t, pad_l) as _Device.conv_bn computes them."""
  cin, cout, kh, kw, stride, padding = spec
  if padding == 'valid':
    return (h - kh) // stride + 1, (w - kw) // stride + 1, 0, 0
  assert stride == 1
  return h, w, (kh - 1) // 2, (kw - 1) // 2


def conv_case(spec, h, w, n=2, epi='bias_relu'):
  cin, cout, kh, kw, stride, padding = spec
  c = CL.C(cin, cout, kh, stride, 'SAME' if padding == 'same' else 'VALID', 0, n, h, w, epi=epi)
  if kh != kw:
    c['kh'], c['kw'] = kh, kw
  assert CL.geom(c) == device_geometry(spec, h, w), (spec, h, w)
  return c


def _conv_cases():
  """[(spec, case)]: every distinct spec at the smallest maps that keep its edge behaviour, the
  non-square ones also on a non-square map, the dense layer with n in {1, 5}."""
  out = []
  for spec, maps in traced_specs().items():
    sizes = []
    for h, w in maps:
      hw = (h, w) if max(h, w) <= 35 else STEM_MAP
      if hw not in sizes:
        sizes.append(hw)
    if spec[2] != spec[3]:
      sizes.append(NONSQUARE_MAP)
    out += [(spec, conv_case(spec, h, w)) for h, w in sizes]
  out += [(DENSE_SPEC, conv_case(DENSE_SPEC, 1, 1, n, 'bias')) for n in (1, 5)]
  return out


# the register-staged (scalar-gather) routes: the evaluator has no non-square fp32 spec with
# cin % 32 != 0 and only cin = 160 leaves the LDS-DMA kernels in bf16
SYNTHETIC = [(24, 48, 1, 7, 1, 'same'), (40, 48, 1, 7, 1, 'same')]
CONV_CASES = _conv_cases() + [(s, conv_case(s, *NONSQUARE_MAP)) for s in SYNTHETIC]

BACKWARD = [conv_case((128, 128, 1, 7, 1, 'same'), 17, 13, epi='none'),
            conv_case((160, 160, 7, 1, 1, 'same'), 17, 13, epi='none'),
            conv_case((384, 384, 1, 3, 1, 'same'), 8, 8, epi='none')]

ROUTE_LOG = []     # (spec, (h, w, n), dtype, route) of every forward launch of this module


def _id(sc):
  (cin, cout, kh, kw, s, pad), c = sc
  return f"{cin}-{cout}-{kh}x{kw}s{s}{pad[0]}-{c['h']}x{c['w']}n{c['n']}"


def build_conv(c):
  """The forward reference of a case with run_fwd's own seeds (no GPU): -> invisible bf16 share."""
  n, h, w, cin, cout, s = c['n'], c['h'], c['w'], c['cin'], c['cout'], c.get('stride', 1)
  kh, kw = CL.khw(c)
  ho, wo, pt, pl = CL.geom(c)
  x, kern = LT.ternary((n, h, w, cin), CL._seed(c, 1)), LT.ternary((kh, kw, cin, cout), CL._seed(c, 2))
  bias = LT.bias_ints(cout, CL._seed(c, 5))
  y, pre, q = LT.conv2d_fwd(x, kern, ho, wo, s, pt, pl, 0, None, None, bias, None, None,
                            1 if c['epi'] == 'bias_relu' else 0, 0.0)
  LT.assert_exact_range(y, f'fwd {c}', 0.25)
  return LT.assert_visible(pre, f'fwd {c}', q)


def build_backward(c):
  n, h, w, cin, cout = c['n'], c['h'], c['w'], c['cin'], c['cout']
  kh, kw = CL.khw(c)
  ho, wo, pt, pl = CL.geom(c)
  kern = LT.ternary((kh, kw, cin, cout), CL._seed(c, 2))
  x, dy = LT.ternary((n, h, w, cin), CL._seed(c, 1)), LT.ternary((n, ho, wo, cout), CL._seed(c, 11))
  _, pre, q = LT.conv2d_dgrad(dy, kern, (n, h, w, cin), 1, pt, pl)
  LT.conv2d_wgrad(x, dy, (kh, kw, cin, cout), 1, pt, pl)
  return LT.assert_visible(pre, f'dgrad {c}', q)


def _run_conv(sc):
  spec, c = sc
  for dt in DTS:      # (the two runs share one reference)
    routes = CL.run_fwd(c, dt)
    rid = _L().se3ds_debug_last_conv_route()
    name = _L().se3ds_debug_conv_route_name(rid).decode()
    assert routes == [name], (routes, name)
    ROUTE_LOG.append((spec, (c['h'], c['w'], c['n']), dt, name))


@pytest.mark.parametrize('sc', CONV_CASES, ids=_id)
def test_evaluator_conv_is_bit_exact(sc, monkeypatch):
  CL._setenv(monkeypatch, {})
  _run_conv(sc)


def test_every_spec_has_a_case():
  have = {s for s, _ in CONV_CASES}
  missing = [s for s in list(dict.fromkeys(iu.conv_specs())) + [DENSE_SPEC] if s not in have]
  assert not missing, missing
  for spec, c in CONV_CASES:
    if spec[2] != spec[3] and spec not in SYNTHETIC:
      assert any(s == spec and (k['h'], k['w']) == NONSQUARE_MAP for s, k in CONV_CASES), spec
  assert {c['n'] for s, c in CONV_CASES if s == DENSE_SPEC} == {1, 5}


@pytest.mark.parametrize('shape', [(1, 7, 128, 128), (7, 1, 160, 192)], ids=['1x7', '7x1'])
@pytest.mark.parametrize('dt', DTS)
def test_prep_operand_is_the_runners_k_order(shape, dt):
  """InceptionV3._prep (se3ds_weight_prep) lays the HWIO kernel out as wt [cout][(kh, kw, cin)]:
  the K order the lattice runners feed the convolution with."""
  w = LT.ternary(shape, 7 * shape[0] + shape[1])
  m = types.SimpleNamespace(dtype=_DT[dt], device=torch.device(DEV),
                            code=_lib.BF16 if dt == 'bf16' else _lib.F32)
  wt = iu.InceptionV3._prep(m, w.to(DEV).contiguous())
  torch.cuda.synchronize()
  assert wt.dtype == _DT[dt] and tuple(wt.shape) == (shape[3], shape[0] * shape[1] * shape[2])
  LT.assert_bit_equal(wt.float().cpu(), LT.weight_operands(w, _DT[dt])[0].float(), f'_prep {shape} {dt}', 'flat')
  kh, kw, cin, _ = shape      # (ky, kx, ci) -> k = (ky * kw + kx) * cin + ci, spelled out once
  ky, kx, ci, co = kh - 1, kw - 1, 5, 3
  assert float(wt[co, (ky * kw + kx) * cin + ci]) == float(w[ky, kx, ci, co])


@pytest.mark.parametrize('c', BACKWARD, ids=lambda c: f"{c['cin']}-{c.get('kh')}x{c.get('kw')}")
@pytest.mark.parametrize('dt', DTS)
def test_nonsquare_backward_is_bit_exact(c, dt, monkeypatch):
  CL._setenv(monkeypatch, {})
  d = CL.run_dgrad(c, dt)
  wg = CL.run_wgrad({k: v for k, v in c.items() if k != 'epi'}, dt)
  assert '_dgrad' in d[0] and wg[0].startswith('wgrad') and wg[1] in CL._R, (d, wg)
  print(f"non-square backward {c['cin']} {CL.khw(c)} {dt}: dgrad {d[0]}, wgrad {wg[0]} + {wg[1]}")


# ---------------------------------------------------------------------------------------------
# concatenation glue: _Cat flattening, se3ds_copy_channels and se3ds_inception_maxpool3s2 offsets

LAYOUTS = [[64, 64, 96, 32], [64, 64, 96, 64], [384, 96, 'pool288'], [192, 192, 192, 192],
           [320, 192, 'pool768'], [320, [384, 384], [384, 384], 192]]
CAT_N = 2


def _flat(layout):
  return [q for p in layout for q in (_flat(p) if isinstance(p, list) else [p])]


def _maxpool3s2_np(x):
  n, h, w, c = x.shape
  oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
  y = np.empty((n, oh, ow, c))
  for oy in range(oh):
    for ox in range(ow):
      y[:, oy, ox] = x[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].reshape(n, 9, c).max(axis=1)
  return y


def build_cat(layout, seed=0):
  """-> (host parts in layout order [(kind, array)], expected (n, 3, 3, ctot)).  Values are distinct
  small integers (exact in bf16): a part's element depends on the part, the channel and the pixel."""
  parts, c0 = [], 0
  for i, p in enumerate(_flat(layout)):
    pool = isinstance(p, str)
    c = int(p[4:]) if pool else p
    hw = 7 if pool else 3
    idx = np.arange(CAT_N * hw * hw * c, dtype=np.int64).reshape(CAT_N, hw, hw, c)
    a = ((idx * 7 + (c0 + i) * 13 + seed) % 251 - 125).astype(np.float64)
    parts.append(('pool' if pool else 'copy', a))
    c0 += c
  exp = np.concatenate([_maxpool3s2_np(a) if k == 'pool' else a for k, a in parts], axis=3)
  LT.assert_np_lattice(exp, 'concat', 1.0, 125.0)
  return parts, exp


def _nest(layout, flat_parts):
  """Rebuilds the evaluator's objects: tensors, pending _MaxPool, nested _Cat."""
  it = iter(flat_parts)

  def make(p):
    if isinstance(p, list):
      return iu._Cat([make(q) for q in p])
    return next(it)
  return iu._Cat([make(p) for p in layout])


@pytest.mark.parametrize('layout', LAYOUTS, ids=lambda l: '-'.join(str(p) for p in _flat(l)))
@pytest.mark.parametrize('dt', DTS)
def test_concat_glue(layout, dt):
  parts, exp = build_cat(layout)
  m = types.SimpleNamespace(dtype=_DT[dt], device=torch.device(DEV),
                            code=_lib.BF16 if dt == 'bf16' else _lib.F32)
  d = iu._Device(m)
  objs = []
  for kind, a in parts:
    t = torch.from_numpy(a).to(_DT[dt]).to(DEV).contiguous()
    objs.append(iu._MaxPool(t) if kind == 'pool' else t)
  cat = _nest(layout, objs)
  assert all(not isinstance(p, iu._Cat) for p in cat.parts) and len(cat.parts) == len(parts)
  y = d._dense(cat)
  torch.cuda.synchronize()
  assert tuple(y.shape) == exp.shape and y.dtype == _DT[dt]
  LT.assert_bit_equal(y.float().cpu().numpy(), LT.f32(exp), f'concat {layout} {dt}')
  want = torch.cat([torch.from_numpy(_maxpool3s2_np(a) if k == 'pool' else a) for k, a in parts], dim=3)
  assert torch.equal(y.double().cpu(), want)
  assert d._dense(cat) is y            # built once


# ---------------------------------------------------------------------------------------------
# pools

POOL_N, SENTINEL = 2, 7.0
AVG_HW = ((1, 1), (1, 5), (2, 2), (3, 3), (8, 8), (17, 13))
MAX_HW = ((3, 3), (4, 4), (7, 9), (17, 17))
POOL_C = (1, 12, 24)


def _slice_of(c):
  """(y_c, y_c0): the layer fills [y_c0, y_c0 + c) of pixel rows of y_c channels."""
  return c + 9, 5


def build_avgpool(h, w, c, seed):
  x = 36.0 * LT.small_ints((POOL_N, h, w, c), 900 + seed, -3, 3)
  LT.assert_lattice36(x, 'x')
  y = np.empty_like(x)
  for oy in range(h):
    for ox in range(w):
      win = x[:, max(oy - 1, 0):oy + 2, max(ox - 1, 0):ox + 2]
      y[:, oy, ox] = win.sum(axis=(1, 2)) / (win.shape[1] * win.shape[2])   # in-bounds taps only
  LT.assert_np_lattice(y, 'avgpool3s1', 1.0, 255.0)     # integers below 256: exact in bf16
  return x, y


def build_maxpool(h, w, c, seed):
  x = LT.tie_ints((POOL_N, h, w, c), 950 + seed)
  x[(x == 0) & (LT.rng(951 + seed).random(x.shape) < 0.3)] = -0.0
  y = _maxpool3s2_np(x)
  ties = float(np.mean([(x[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].reshape(POOL_N, 9, c) ==
                         y[:, oy:oy + 1, ox].reshape(POOL_N, 1, c)).sum(1) > 1
                        for oy in range(y.shape[1]) for ox in range(y.shape[2])]))
  if h % 2 == 0:      # 'valid': the last row / column of an even map is never read
    x[:, h - 1] = np.nan
  if w % 2 == 0:
    x[:, :, w - 1] = np.nan
  return x, y, ties


def _sliced(shape_hw, c, dt):
  """A guarded (n, h, w, y_c) buffer: sentinel outside the slice, NaN inside it."""
  yc, c0 = _slice_of(c)
  g = CL.Guarded((POOL_N,) + tuple(shape_hw) + (yc,), _DT[dt])
  g.view.fill_(SENTINEL)
  g.view[..., c0:c0 + c] = float('nan')
  return g, yc, c0


def _check_slice(g, exp, c, c0, what):
  torch.cuda.synchronize()
  assert bool(torch.isnan(g.flat[:g.g]).all()) and bool(torch.isnan(g.flat[-g.g:]).all()), f'{what}: guard band'
  out = g.view.float().cpu().numpy()
  LT.assert_bit_equal(out[..., c0:c0 + c], LT.f32(exp), what)
  rest = np.delete(out, np.s_[c0:c0 + c], axis=3)
  assert np.all(rest == SENTINEL), f'{what}: channels outside the slice were written'


@pytest.mark.parametrize('dt', DTS)
def test_avgpool3s1_is_exact(dt):
  i = 0
  for h, w in AVG_HW:
    for c in POOL_C:
      x, exp = build_avgpool(h, w, c, i)
      i += 1
      xd = torch.from_numpy(x).to(_DT[dt]).to(DEV).contiguous()
      g, yc, c0 = _sliced((h, w), c, dt)
      _lib.check(_L().se3ds_inception_avgpool3s1(xd.data_ptr(), _lib.dtype_code(xd), POOL_N, h, w, c, g.ptr(),
                                                 yc, c0, _lib.stream()), 'avgpool3s1')
      _check_slice(g, exp, c, c0, f'avgpool3s1 {h}x{w} c {c} {dt}')


@pytest.mark.parametrize('dt', DTS)
def test_maxpool3s2_is_exact(dt):
  i = 0
  for h, w in MAX_HW:
    for c in POOL_C:
      x, exp, _ = build_maxpool(h, w, c, i)
      i += 1
      xd = torch.from_numpy(x).to(_DT[dt]).to(DEV).contiguous()
      g, yc, c0 = _sliced(exp.shape[1:3], c, dt)
      _lib.check(_L().se3ds_inception_maxpool3s2(xd.data_ptr(), _lib.dtype_code(xd), POOL_N, h, w, c, g.ptr(),
                                                 yc, c0, _lib.stream()), 'maxpool3s2')
      _check_slice(g, exp, c, c0, f'maxpool3s2 {h}x{w} c {c} {dt}')


GAP_N, GAP_C = 3, (1, 100, 2048)


def build_gap(hw, c, seed):
  """hw 64: integers in [-4, 4]; hw 49: multiples of 49 -- sum and quotient are exact either way."""
  x = LT.small_ints((GAP_N, hw, c), 980 + seed, -4, 4) * (49.0 if hw == 49 else 1.0)
  assert hw in (49, 64) and np.abs(x).max() <= 256
  s = LT.assert_exact_colsum(x, 'global_avg_pool', 1.0)
  return x, LT.exact32(s / hw, 'mean')


@pytest.mark.parametrize('dt', DTS)
def test_global_avg_pool_is_exact(dt):
  for i, (hw, c) in enumerate((hw, c) for hw in (64, 49) for c in GAP_C):
    x, exp = build_gap(hw, c, i)
    xd = torch.from_numpy(x).to(_DT[dt]).to(DEV).contiguous()
    g = CL.Guarded((GAP_N, c), torch.float32)
    _lib.check(_L().se3ds_global_avg_pool(xd.data_ptr(), _lib.dtype_code(xd), GAP_N, hw, c, g.ptr(),
                                          _lib.stream()), 'global_avg_pool')
    LT.assert_bit_equal(g.result(f'gap {hw} {c}').numpy(), LT.f32(exp), f'global_avg_pool hw {hw} c {c} {dt}', 'flat')


# ---------------------------------------------------------------------------------------------
# softmax

SM_ROWS, SM_C = (1, 4, 5, 9), (1, 63, 64, 65, 1000)
SOFTMAX_STATS = []     # (rows, c, dtype, scale, fp32 floor, kernel error)


def softmax_ref(z, dtype=np.float64):
  """tf.nn.softmax: exp(z - max) / sum; dtype=np.float32 is the plain fp32 restatement."""
  z = np.asarray(z, dtype=dtype)
  e = np.exp(z - z.max(axis=1, keepdims=True))
  return e / e.sum(axis=1, keepdims=True, dtype=dtype)


def softmax_inputs(rows, c, dt, scale, seed):
  """Random logits (bf16 runs: rounded to bf16 first, so every evaluation sees the same values)."""
  z = LT.f32(LT.rng(seed).standard_normal((rows, c)) * 4)
  m = np.abs(z).max()
  if scale:
    z = LT.f32(z * (scale / m))      # reaches +-scale: exp overflows without the max subtraction
  return LT.rne_np(z, dt == 'bf16')


def _softmax(z, dt):
  rows, c = z.shape
  zd = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(_DT[dt]).to(DEV)
  g = CL.Guarded((rows, c), torch.float32)
  _lib.check(_L().se3ds_softmax_rows(zd.data_ptr(), _lib.dtype_code(zd), rows, c, g.ptr(), _lib.stream()),
             'softmax_rows')
  return g.result(f'softmax {rows} x {c} {dt}').numpy()


@pytest.mark.parametrize('dt', DTS)
def test_softmax_exact_rows(dt):
  for rows in SM_ROWS:
    for c in SM_C:
      for v in (0.0, 3.0, -80.0):      # constant rows: fp32(1 / c) in every element
        got = _softmax(np.full((rows, c), v), dt)
        LT.assert_bit_equal(got, np.full((rows, c), np.float32(1.0) / np.float32(c)), f'constant {v} {rows}x{c}', 'flat')
      z = np.full((rows, c), -200.0)   # exp(-200) = 0 in fp32: exactly one-hot
      hot = [(7 * r + c - 1) % c for r in range(rows)]
      z[np.arange(rows), hot] = 0.0
      exp = np.zeros((rows, c), np.float32)
      exp[np.arange(rows), hot] = 1.0
      LT.assert_bit_equal(_softmax(z, dt), exp, f'one-hot {rows}x{c} {dt}', 'flat')


@pytest.mark.parametrize('dt', DTS)
def test_softmax_random_rows(dt):
  for rows in SM_ROWS:
    for c in SM_C:
      for scale in (0, 80):
        z = softmax_inputs(rows, c, dt, scale, 31 * rows + c + scale)
        ref = softmax_ref(z)
        floor = LT.scaled_err(softmax_ref(z, np.float32), ref)
        got = _softmax(z, dt)
        err = LT.scaled_err(got, ref)
        SOFTMAX_STATS.append((rows, c, dt, scale, floor, err))
        print(f'softmax {rows} x {c} {dt} scale {scale}: fp32 floor {floor:.2e}, kernel {err:.2e}', flush=True)
        assert np.all(np.isfinite(got)) and np.all(got >= 0)
        assert err <= 8 * floor, (rows, c, dt, scale, err, floor)
        dev = np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max()
        assert dev <= c * 2.0 ** -23, (rows, c, dt, scale, dev)
  fl = [s[4] for s in SOFTMAX_STATS if s[2] == dt and s[4] > 0]
  ratio = max(s[5] / s[4] for s in SOFTMAX_STATS if s[2] == dt and s[4] > 0)
  print(f'softmax {dt}: fp32 floor {min(fl):.2e} .. {max(fl):.2e}, largest kernel / floor {ratio:.2f}')


# ---------------------------------------------------------------------------------------------
# feature moments: integer rows, every product and sum exact in binary64

MOM_ROWS, MOM_C = (1, 31, 32, 33, 100), (1, 63, 64, 65, 130)
MOM_SENTINEL = -12345.0


def build_moments(rows, c, seed):
  """Two batches of integer rows and the int64 moments after the first and after both."""
  xs = [LT.rng(1000 + seed + k).integers(-8, 9, (rows, c)) for k in (0, 1)]
  states, s, g = [], np.zeros(c, np.int64), np.zeros((c, c), np.int64)
  for x in xs:
    s, g = s + x.sum(0), g + x.T @ x
    assert np.abs(g).max() < 2 ** 53
    states.append((s.copy(), g.copy()))
  tile = np.arange(c) // 64
  lower = tile[:, None] > tile[None, :]      # the strictly lower 64 x 64 tiles: never touched
  return xs, states, lower


def test_feature_moments_are_exact():
  L = _L()
  for i, (rows, c) in enumerate((r, c) for r in MOM_ROWS for c in MOM_C):
    xs, states, lower = build_moments(rows, c, 7 * i)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    s = torch.zeros(c, dtype=torch.float64, device=DEV)
    g = torch.zeros((c, c), dtype=torch.float64, device=DEV)
    g[torch.from_numpy(lower).to(DEV)] = MOM_SENTINEL
    for k, x in enumerate(xs):
      xd = torch.from_numpy(x.astype(np.float32)).to(DEV).contiguous()
      _lib.check(L.se3ds_feature_moments_accumulate(xd.data_ptr(), rows, c, count.data_ptr(), s.data_ptr(),
                                                    g.data_ptr(), _lib.stream()), 'feature_moments')
      torch.cuda.synchronize()
      what = f'moments rows {rows} c {c} call {k}'
      es, eg = states[k]
      assert int(count.cpu()[0]) == (k + 1) * rows, what
      assert np.array_equal(s.cpu().numpy(), es.astype(np.float64)), what + ' sum'
      gh = g.cpu().numpy()
      assert np.array_equal(gh[~lower], eg.astype(np.float64)[~lower]), what + ' gram'
      assert np.all(gh[lower] == MOM_SENTINEL), what + ' strictly lower tiles written'
    before = (count.clone(), s.clone(), g.clone())
    assert L.se3ds_feature_moments_accumulate(xd.data_ptr(), 0, c, count.data_ptr(), s.data_ptr(),
                                              g.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (count, s, g))), f'rows = 0 changed the moments (c {c})'


# ---------------------------------------------------------------------------------------------
def build_all(verbose=True):
  """Builds every case of this module and runs the references' preconditions (no GPU).  Returns
  (number of cases, largest share of bf16 elements a unit error could hide in)."""
  n, worst = 0, 0.0
  test_every_spec_has_a_case()
  for spec, c in CONV_CASES:
    s = build_conv(c)
    if verbose:
      print(f'invisible share {100 * s:.4f} % in {_id((spec, c))}')
    worst, n = max(worst, s), n + 1
  for c in BACKWARD:
    s = build_backward(c)
    if verbose:
      print(f"invisible share {100 * s:.4f} % in dgrad {c['cin']} {CL.khw(c)}")
    worst, n = max(worst, s), n + 1
  for layout in LAYOUTS:
    build_cat(layout)
    n += 1
  i = 0
  for h, w in AVG_HW:
    for c in POOL_C:
      build_avgpool(h, w, c, i)
      i, n = i + 1, n + 1
  i, ties = 0, []
  for h, w in MAX_HW:
    for c in POOL_C:
      ties.append(build_maxpool(h, w, c, i)[2])
      i, n = i + 1, n + 1
  if verbose:
    print(f'3x3/s2 max-pool windows with a tie for the maximum: mean {np.mean(ties):.3f}')
  assert np.mean(ties) >= 0.25, ties
  for i, (hw, c) in enumerate((hw, c) for hw in (64, 49) for c in GAP_C):
    build_gap(hw, c, i)
    n += 1
  for i, (rows, c) in enumerate((r, c) for r in MOM_ROWS for c in MOM_C):
    build_moments(rows, c, 7 * i)
    n += 1
  return n, worst


# ---------------------------------------------------------------------------------------------
def test_route_table_covers_every_spec(monkeypatch):
  """Last: prints the (spec, dtype, route) table of this run and pins the families (cases that
  did not run in this session, because this test was selected alone, run here)."""
  CL._setenv(monkeypatch, {})
  seen = {(s, hwn) for s, hwn, _, _ in ROUTE_LOG}
  for sc in CONV_CASES:
    if (sc[0], (sc[1]['h'], sc[1]['w'], sc[1]['n'])) not in seen:
      _run_conv(sc)
  for spec, hwn, dt, route in ROUTE_LOG:
    print(f'route {spec} @ {hwn} {dt}: {route}')
  for dt in DTS:
    ran = {s for s, _, d, _ in ROUTE_LOG if d == dt}
    wanted = set(iu.conv_specs()) | {DENSE_SPEC}
    assert wanted <= ran, (dt, sorted(wanted - ran))
    nonsq = {r for s, _, d, r in ROUTE_LOG if d == dt and s[2] != s[3]}
    assert any(r.startswith('glds_') for r in nonsq), (dt, nonsq)     # LDS-DMA
    assert any(r.startswith('igemm_') for r in nonsq), (dt, nonsq)    # register-staged
    print(f'non-square routes {dt}: {sorted(nonsq)}')
