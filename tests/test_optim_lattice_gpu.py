"""Bit-exact lattice tests of the kernels that run after the backward pass: the multi-tensor
squared norm / clip / Adam / EMA and the spectral power iteration and fix-up of
se3ds_amd/csrc/optim.hip, the loss and head kernels of pointwise.hip -- driven through the host
classes that feed them (nn.ParamStore.chunk_tables, nn.SpectralGroup, gan_manager.AdamState) on a
synthetic store: no model, no activations.  References: tests/_lattice.py (NumPy float64, pinned
without a GPU by tests/test_lattice_cpu.py).

Everything is compared with LT.assert_bit_equal, every element of every tensor, alignment gaps
included, except
  * Adam / EMA outputs: |kernel - float64| <= K * 2^-24 * (largest float64 intermediate of that
    element), K = LT.K_M / K_V / K_P / K_E roundings counted from the documented formulas;
  * power iteration and the rgb head: 8 x the error of a plain fp32 NumPy restatement against
    float64 on the same inputs (printed per case).
The last test prints the (kernel, path-class) table the module reached and asserts that it holds
every class the shape table was built for; it relies on pytest's in-file order.
"""
import types

import numpy as np
import pytest
import torch

from se3ds_amd import _lib
import se3ds_amd.hipops  # noqa: F401  registers the signatures
from se3ds_amd.hipops import nn
from se3ds_amd.trainers.gan_manager import AdamState
import _lattice as LT
from test_prod_shapes_gpu import PROD_CONVS

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CHUNK, BLOCK = 65536, 256          # ParamStore.chunk_tables' default, the kernels' workgroup
LR, B1, B2, EPS = 1e-4, 0.5, 0.999, 1e-7      # configs/highres
OMD = float(np.float32(1.0 - 0.999))
CLIP = 5.0


def _L():
  return _lib.lib()


# ---------------------------------------------------------------------------------------------
# shape table

def _harvest():
  """(kh, kw, cin, cout) of the effective spectral kernels of the configs/highres generator and
  discriminator, widest first, read from their un-finalised stores (nothing is allocated: the
  models' _finish -- finalize + SpectralGroup -- is held back while they are constructed)."""
  import os
  from se3ds_amd import gin_lite
  from se3ds_amd.models import image_models as IM
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  saved = gin_lite.operative_bindings()      # whatever another test module has configured
  gin_lite.clear_config()
  gin_lite.parse_config_files_and_bindings([os.path.join(root, 'configs', 'highres', 'highres.gin')], [])
  orig = IM._Model._finish
  IM._Model._finish = lambda self, device, seed, dtype: None
  try:
    models = (IM.ResNetGenerator(image_size=512, device='cpu'),
              IM.SNMultiScaleDiscriminator(image_size=512, device='cpu'))
  finally:
    IM._Model._finish = orig
    gin_lite.clear_config()
    gin_lite._BINDINGS.update(saved)
  out = []
  for mdl in models:
    assert mdl.store.theta is None
    shapes = {s[0]: s[1] for s in mdl.store._specs}
    found = {shapes[l.name + '/kernel'] for l in IM._conv_layers_of(mdl) if l.kind == 'spectral'}
    out.append(sorted(found, key=lambda s: -int(np.prod(s))))
  return out


_GEN, _DIS = _harvest()
assert _GEN[0] == (3, 3, 1024, 1024) and _DIS[0][:2] == (4, 4), (_GEN[:2], _DIS[:1])
assert {(r[4], r[4], r[2], r[3]) for r in PROD_CONVS if r[1] == 'spectral'} >= {_GEN[0], _DIS[0]}

S, P = 'spectral', 'plain'
# (segment, kind, shape): spectral and plain tensors alternate; segments 'a' and 'b' start on a
# plain tensor and end on a spectral one, 'c' starts on a spectral one (tensor_base != 0) and ends
# on a plain one; spectral tensors sit behind the alignment gaps of plain ones.
OPT_TENSORS = [
    ('a', P, (1,)),
    ('a', S, _GEN[0]),                 # widest generator kernel, Cout 1024: dq == 0, 144 chunks
    ('a', P, (3,)),
    ('a', S, (1, 1, 512, 2048)),       # Cout 2048
    ('a', P, (64,)),
    ('a', S, (3, 3, 128, 3)),          # rgb head: Cout % 4 != 0
    ('a', P, (65535,)),
    ('a', S, (3, 3, 128, 1)),          # depth head / discriminator logits: Cout 1
    ('b', P, (4,)),
    ('b', S, _DIS[0]),                 # widest discriminator kernel, 4 x 4
    ('b', P, (65536,)),
    ('b', S, (1, 1, 512, 256)),        # Cout 256: dq == 1, dr == 0
    ('b', P, (65537,)),
    ('b', S, (1, 1, 33, 64)),          # K 33: ceil(33 / 32) * 31 >= 33, empty slabs; K < 256
    ('c', S, _GEN[1]),                 # second widest generator kernel
    ('c', P, (2 * 65536 + 5,)),
    ('c', S, (3, 3, 3, 1)),            # K 27 < 256, Cout 1, 27 elements: scalar tail
    ('c', P, (4096,)),
    ('c', P, (1024,)),
]
assert sum(int(np.prod(s)) for _, _, s in OPT_TENSORS) < 40e6

REACHED = {}


def reach(kernel, cls, detail):
  REACHED.setdefault((kernel, cls), str(detail))


class Bed:
  """The synthetic store, its spectral group and optimiser, and host-side layout."""

  def __init__(self):
    self.store = nn.ParamStore()
    self.layers, self.names, self.kinds = [], [], []
    for i, (seg, kind, shape) in enumerate(OPT_TENSORS):
      base = f'{seg}/t{i:02d}'
      if kind == S:
        kh, kw, cin, cout = shape
        assert kh == kw
        self.layers.append(nn.ConvLayer(self.store, base, cin, cout, kh, use_bias=False, kind='spectral'))
        self.names.append(base + '/kernel')
      else:
        self.names.append(self.store.add(base + '/w', shape, nn.zeros_init))
      self.kinds.append(kind)
    self.store.finalize(DEV)
    assert self.store.trainable_names == self.names
    self.spectral = nn.SpectralGroup(self.layers, DEV)
    self.opt = AdamState(self, LR, B1, B2, EPS)
    self.off = {n: self.store._off_tr[n][:2] for n in self.names}
    self.numel = self.store.theta.numel()
    self.segs = self.store.segments(['a', 'b', 'c'])
    self.layer_of = {l.name + '/kernel': l for l in self.layers}
    self.KC = {n: (int(np.prod(s[:3])), s[3]) for n, (_, k, s) in zip(self.names, OPT_TENSORS) if k == S}
    # chunk tables against an independent statement of the layout
    chunks = self.opt.chunks.cpu().numpy()
    want = [(t, o + s, min(CHUNK, n - s)) for t, name in enumerate(self.names)
            for o, n in [self.off[name]] for s in range(0, n, CHUNK)]
    assert chunks.tolist() == [list(w) for w in want]
    tcs = self.opt.tensor_chunk_start.cpu().numpy()
    assert tcs.tolist() == list(np.cumsum([0] + [-(-self.off[n][1] // CHUNK) for n in self.names]))
    o = 0
    for n in self.names:
      assert self.off[n][0] == o and o % 4 == 0
      o = (o + self.off[n][1] + 3) // 4 * 4

  # host <-> arena
  def arena(self, per_tensor):
    a = np.zeros(self.numel, np.float64)
    for n, x in per_tensor.items():
      o, k = self.off[n]
      a[o:o + k] = np.asarray(x, np.float64).reshape(-1)
    return a

  def real(self):
    m = np.zeros(self.numel, bool)
    for n in self.names:
      o, k = self.off[n]
      m[o:o + k] = True
    return m

  def put(self, dst, host):
    dst.copy_(torch.from_numpy(np.asarray(host, np.float64).astype(np.float32)).to(DEV))

  def get(self, t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()

  def tensor_range(self, seg):
    return self.segs[seg][:2]


@pytest.fixture(scope='module')
def bed():
  return Bed()


@pytest.fixture(scope='module')
def lat(bed):
  """Lattice state of the whole store, made once: plain gradients with power-of-four squared
  norms; per spectral layer G, W, v, uhat, inv with the fixed gradient and its reductions."""
  r = types.SimpleNamespace(g={}, w={}, sn={}, fixed={}, red={})
  invs, dots = (0.5, 1.0, 2.0), (1, -3, 2, -1, 5)
  for i, n in enumerate(bed.names):
    o, k = bed.off[n]
    if bed.kinds[i] == P:
      r.g[n] = LT.pow4_gradient(k, 100 + i, scale=(1.0, 2.0, 0.5)[i % 3])
      continue
    K, C = bed.KC[n]
    inv, dot = invs[i % 3], dots[i % 5]
    if K * C > 4e6:
      inv, dot = (0.5, 1.0)[i % 2], (1, -1)[i % 2]     # room for sum f^2 below 2^24 quanta
    for density in (2.0 / 3.0, 0.4, 0.25, 0.12, 0.05):
      c = LT.sn_case(K, C, 200 + i, inv, dot, density)
      fixed, red = LT.sn_fixup(**c)
      if red['sq'] / red['quantum'] ** 2 < LT.LIMIT:
        break
    LT.assert_reduction(red['sq'] / red['quantum'] ** 2 + 1, f'{n}: sum f^2')
    assert red['dot'] == dot
    print(f'{n}: K {K} C {C} inv {inv} <G,W> {dot} density {density} sum f^2 {red["sq"]}')
    r.g[n], r.w[n], r.sn[n], r.fixed[n], r.red[n] = c['G'], c['W'], c, fixed, red
  r.G = bed.arena(r.g)
  r.W = bed.arena(r.w)
  # expected arenas
  r.F = bed.arena({n: r.fixed.get(n, r.g[n]) for n in bed.names})
  r.sq_fixed = [r.red[n]['sq'] if n in r.red else LT.sqnorm(r.g[n], 0.5) for n in bed.names]
  r.sq_raw = [r.red[n]['gg'] if n in r.red else LT.sqnorm(r.g[n], 0.5) for n in bed.names]
  r.clip_fixed = bed.arena({n: LT.clip_by_norm(r.fixed.get(n, r.g[n]), CLIP, r.sq_fixed[t])
                            for t, n in enumerate(bed.names)})
  r.clip_raw = bed.arena({n: LT.clip_by_norm(r.g[n], CLIP, r.sq_raw[t]) for t, n in enumerate(bed.names)})
  return r


def load_spectral(bed, lat):
  """Gradient arena := G, kernels := W, and the spectral table rows (v, uhat, sig) as the test
  owns them.  sig = (sigma, 1 / sigma)."""
  bed.put(bed.store.grad, lat.G)
  bed.put(bed.store.theta, lat.W)
  for n, c in lat.sn.items():
    sn = bed.layer_of[n].sn
    bed.put(sn['v'], c['v'])
    bed.put(sn['uhat'], c['uhat'])
    bed.put(sn['sig'], [1.0 / c['inv'], c['inv']])
    sn['vpart'].fill_(float('nan'))     # every slot the kernels read must have been written


def mark_clip(bed, t0, t1, fused_sn, kernel='clip_kernel'):
  """Path classes of a clip launch over tensors [t0, t1), computed from the layout."""
  if t0 > 0 and fused_sn:
    reach('se3ds_multi_sqnorm_sn', f'tensor_base != 0, segment starts on a {bed.kinds[t0]} tensor',
          f'tensors [{t0}, {t1})')
  for t in range(t0, t1):
    n = bed.names[t]
    k = bed.off[n][1]
    if kernel == 'clip_adam_kernel' and k % 4:
      reach(kernel, 'scalar tail (len % 4 != 0)', f'{n}: {k} elements')
    if bed.kinds[t] == S and fused_sn:
      K, C = bed.KC[n]
      if kernel == 'clip_kernel':
        if BLOCK // C == 0:
          reach(kernel, 'dq == 0 (Cout > 256)', f'{n}: Cout {C}')
        if C == 1:
          reach(kernel, 'Cout == 1', n)
        if C % 4:
          reach(kernel, 'Cout % 4 != 0', f'{n}: Cout {C}')
      else:
        reach(kernel, 'uhat as float4' if C % 4 == 0 else 'C & 3 fallback', f'{n}: Cout {C}')
      if k > CHUNK:
        reach(kernel, 'chunk from the middle of a tensor', f'{n}: {-(-k // CHUNK)} chunks')
    else:
      reach(kernel, 'plain tensor', n)


def mark_dots(bed, names):
  for n in names:
    K, C = bed.KC[n]
    reach('sn_dots_kernel', 'vector' if C % 4 == 0 else 'scalar branch (Cout % 4 != 0)', f'{n}: Cout {C}')
    if K < 256:
      reach('sn_dots_kernel', 'K < 256 (waves without a row)', f'{n}: K {K}')


def dots(bed, seg=None):
  bed.spectral.backward_fixup(prefix=seg, dots_only=True)
  mark_dots(bed, [n for n in bed.KC if seg is None or n.startswith(seg + '/')])


def check_arena(got, want, what):
  LT.assert_bit_equal(got, LT.f32(want), what, layout='flat')


# ---------------------------------------------------------------------------------------------
# squared norm and clip of plain tensors

@pytest.fixture(scope='module')
def plain(bed):
  """Every tensor of the store as a plain one: power-of-four squared norms 4^j * scale^2."""
  scale = (1.0, 2.0, 4.0)
  g = {n: LT.pow4_gradient(bed.off[n][1], 300 + i, scale=scale[i % 3]) for i, n in enumerate(bed.names)}
  sq = [LT.sqnorm(g[n], scale[i % 3]) for i, n in enumerate(bed.names)]
  assert all(LT.is_pow4(s) for s in sq) and min(sq) >= 1 and max(sq) < 2.0 ** 40
  return types.SimpleNamespace(g=g, sq=sq, G=bed.arena(g))


@pytest.mark.parametrize('clip', [0.5, 5.0, 2.0 ** 21], ids=['active', 'mixed', 'inactive'])
@pytest.mark.parametrize('segments', [False, True], ids=['arena', 'segments'])
def test_sqnorm_and_clip_plain(bed, plain, clip, segments):
  norms = np.sqrt(plain.sq)
  assert {'active': (norms > clip).all(), 'inactive': (norms < clip).all(),
          'mixed': (norms > clip).any() and (norms < clip).any()}[
              'active' if clip == 0.5 else 'mixed' if clip == 5.0 else 'inactive']
  bed.put(bed.store.grad, plain.G)
  bed.opt.sqnorm.fill_(float('nan'))
  if segments:
    for seg in ('c', 'b', 'a'):
      t0, t1 = bed.tensor_range(seg)
      bed.opt.clip_segment(t0, t1, clip)
      mark_clip(bed, t0, t1, False)
    mean = bed.opt.mean_clipped_norm(clip)
  else:
    mean = bed.opt.clip_gradients(clip)
    mark_clip(bed, 0, len(bed.names), False)
  LT.assert_bit_equal(bed.get(bed.opt.sqnorm), LT.f32(plain.sq), 'sqnorm', layout='flat')
  want = bed.arena({n: LT.clip_by_norm(plain.g[n], clip, plain.sq[t]) for t, n in enumerate(bed.names)})
  # power-of-four norms: the expectation IS tf.clip_by_norm in float64, rounded once
  ref = bed.arena({n: (plain.g[n] * clip) / max(norms[t], clip) for t, n in enumerate(bed.names)})
  assert np.array_equal(LT.f32(want), LT.f32(ref))
  check_arena(bed.get(bed.store.grad), want, f'clipped arena, clip {clip}')
  LT.assert_bit_equal(bed.get(mean), [LT.mean_clipped_norm(plain.sq, clip)], 'mean clipped norm', layout='flat')


def test_zero_gradient_has_norm_zero_and_no_nan(bed):
  bed.store.grad.zero_()
  bed.opt.sqnorm.fill_(float('nan'))
  mean = bed.opt.clip_gradients(CLIP)
  assert not bed.get(bed.opt.sqnorm).any()
  g = bed.get(bed.store.grad)
  assert not np.isnan(g).any() and not g.any()
  LT.assert_bit_equal(bed.get(mean), [LT.mean_clipped_norm([0.0] * len(bed.names), CLIP)], 'mean', layout='flat')
  LT.assert_bit_equal(bed.get(bed.opt.mean_clipped_norm(CLIP)), [np.float32(0)], 'mean', layout='flat')


# ---------------------------------------------------------------------------------------------
# spectral fix-up: three routes, one reference

def test_spectral_route_a_fixup_then_clip(bed, lat):
  load_spectral(bed, lat)
  bed.spectral.backward_fixup()
  for n in bed.KC:
    reach('sn_fix_kernel', 'separate fix-up', n)
  check_arena(bed.get(bed.store.grad), lat.F, 'gradient arena after backward_fixup')
  bed.opt.sqnorm.fill_(float('nan'))
  bed.opt.clip_gradients(CLIP)
  LT.assert_bit_equal(bed.get(bed.opt.sqnorm), LT.f32(lat.sq_fixed), 'sqnorm of the fixed arena', layout='flat')
  check_arena(bed.get(bed.store.grad), lat.clip_fixed, 'fixed arena after the clip')
  check_arena(bed.get(bed.store.theta), lat.W, 'weights')


@pytest.mark.parametrize('segments', [False, True], ids=['route_b_arena', 'route_c_segments'])
def test_spectral_fused_fixup_clip(bed, lat, segments):
  load_spectral(bed, lat)
  bed.opt.sqnorm.fill_(float('nan'))
  if segments:
    for seg in ('c', 'b', 'a'):
      t0, t1 = bed.tensor_range(seg)
      dots(bed, seg)
      bed.opt.clip_segment(t0, t1, CLIP, fused_sn=True)
      mark_clip(bed, t0, t1, True)
  else:
    dots(bed)
    bed.opt.clip_gradients(CLIP, fused_sn=True)
    mark_clip(bed, 0, len(bed.names), True)
  # closed form: exact integers (in quanta), at most one rounding to fp32
  LT.assert_bit_equal(bed.get(bed.opt.sqnorm), LT.f32(lat.sq_fixed), 'closed-form sqnorm', layout='flat')
  for n, red in lat.red.items():
    vp = bed.get(bed.layer_of[n].sn['vpart']).astype(np.float64)
    rb = (_L().se3ds_spectral_vpart_len() - 2) // 3
    got = [vp[0:rb].sum(), vp[rb:2 * rb].sum(), vp[2 * rb:3 * rb].sum(), vp[3 * rb], vp[3 * rb + 1]]
    assert got == [red['dot'], red['gg'], red['gvu'], red['nv'], red['nu']], (n, got, red)
  check_arena(bed.get(bed.store.grad), lat.clip_fixed, 'fused fix-up + clip')


# ---------------------------------------------------------------------------------------------
# fused clip + Adam + EMA

@pytest.fixture(scope='module')
def slots(bed):
  """Non-zero fp32 optimiser state; gaps stay 0."""
  r = LT.rng(77)
  def per(fn):
    return LT.f32(bed.arena({n: fn(bed.off[n][1]) for n in bed.names})).astype(np.float64)
  p = per(lambda k: r.standard_normal(k) * 0.05)
  return types.SimpleNamespace(
      p=p, m=per(lambda k: r.standard_normal(k) * 0.1), v=per(lambda k: r.random(k) * 0.02),
      e=LT.f32(p + per(lambda k: r.standard_normal(k) * 0.01)).astype(np.float64))


def check_update(bed, got, ref, mags, what):
  """got / ref: dicts p, m, v (, e).  Prints and returns the worst ratios to the bounds."""
  real = bed.real()
  ratios = {}
  for key, k in (('m', LT.K_M), ('v', LT.K_V), ('p', LT.K_P), ('e', LT.K_P + LT.K_E)):
    if key not in got:
      continue
    assert not got[key][~real].any(), f'{what}: {key} written in an alignment gap'
    ratios[key] = LT.bound_ratio(got[key][real], ref[key][real], k, mags[key][real])
  print(f'{what}: kernel / bound: ' + ' '.join(f'{k}={x:.3f}' for k, x in ratios.items()), flush=True)
  assert max(ratios.values()) <= 1.0, (what, ratios)
  return ratios


FUSED = [  # fused_sn, ema, per segment, step
    (True, True, True, 1), (False, False, False, 2), (True, False, False, 1000),
    (False, True, True, 1000), (True, True, False, 2), (False, False, True, 1)]


@pytest.mark.parametrize('fused_sn,with_ema,segments,step', FUSED)
def test_fused_clip_adam_ema(bed, lat, slots, fused_sn, with_ema, segments, step):
  """clip_apply against the float64 chain clip -> Adam -> EMA.  Worst ratio to the bound
  K * 2^-24 * (largest intermediate): fp32 NumPy on the CPU m 0.20, v 0.20, p 0.07, e 0.06
  (tests/test_lattice_cpu.py::test_adam_and_ema_references); the kernels on an MI355X m 0.25,
  v 0.20, p 0.07, e 0.06 in all six cases (printed per case)."""
  load_spectral(bed, lat)
  # the kernels of the spectral tensors ARE the lattice W (the dots read them); the rest random
  sp = np.zeros(bed.numel, bool)
  for n in bed.KC:
    o, k = bed.off[n]
    sp[o:o + k] = True
  p0 = np.where(sp, lat.W, slots.p)
  bed.put(bed.store.theta, p0)
  bed.put(bed.opt.m, slots.m)
  bed.put(bed.opt.v, slots.v)
  ema_t = torch.empty_like(bed.store.theta) if with_ema else None
  if with_ema:
    bed.put(ema_t, slots.e)
  bed.opt.sqnorm.fill_(float('nan'))
  bed.opt.iterations = step - 1
  bed.opt.begin_step()
  for seg in (('c', 'b', 'a') if segments else (None,)):
    t0, t1 = bed.tensor_range(seg) if seg else (0, len(bed.names))
    if fused_sn:
      dots(bed, seg)
    assert bed.opt.clip_apply(t0, t1, CLIP, fused_sn=fused_sn, ema_theta=ema_t, one_minus_decay=OMD)
    mark_clip(bed, t0, t1, fused_sn, 'clip_adam_kernel')
    reach('clip_adam_kernel', 'with EMA' if with_ema else 'without EMA', f'tensors [{t0}, {t1})')
  bed.opt.end_step()
  check_arena(bed.get(bed.store.grad), lat.G, 'gradient arena after clip_apply (must be unchanged)')
  LT.assert_bit_equal(bed.get(bed.opt.sqnorm), LT.f32(lat.sq_fixed if fused_sn else lat.sq_raw), 'sqnorm', layout='flat')
  gc = LT.f32(lat.clip_fixed if fused_sn else lat.clip_raw).astype(np.float64)
  p2, m2, v2, mag = LT.adam_keras(p0, gc, slots.m, slots.v, LR, B1, B2, step, EPS)
  got = dict(p=bed.get(bed.store.theta), m=bed.get(bed.opt.m), v=bed.get(bed.opt.v))
  ref, mags = dict(p=p2, m=m2, v=v2), dict(mag)
  if with_ema:
    ref['e'], mage = LT.ema(slots.e, p2, OMD)
    mags['e'] = np.maximum(mage, mag['p'])
    got['e'] = bed.get(ema_t)
  check_update(bed, got, ref, mags, f'clip_apply fused_sn={fused_sn} ema={with_ema} segments={segments} step={step}')


def test_apply_segment_and_multi_ema_at_an_odd_offset(bed, lat, slots):
  """The separate Adam (+ EMA) pass and se3ds_multi_ema on elements [e0, e1) with e0 not a multiple
  of the block size (nor of 4): same references, same bounds; nothing outside the range moves.
  Worst ratios on an MI355X: m 0.25, v 0.20, p 0.07, e 0.06; se3ds_multi_ema alone 0.33."""
  e0 = bed.segs['b'][2] + 1
  e1 = bed.numel - 3
  assert e0 % BLOCK and e0 % 4 and (e1 - e0) % BLOCK
  g = LT.f32(lat.clip_raw).astype(np.float64)
  for with_ema in (True, False):
    bed.put(bed.store.grad, g)
    bed.put(bed.store.theta, slots.p)
    bed.put(bed.opt.m, slots.m)
    bed.put(bed.opt.v, slots.v)
    ema_t = torch.empty_like(bed.store.theta)
    bed.put(ema_t, slots.e)
    bed.opt.iterations = 6
    bed.opt.begin_step()
    bed.opt.apply_segment(e0, e1, ema_t if with_ema else None, OMD)
    bed.opt.end_step()
    p2, m2, v2, mag = LT.adam_keras(slots.p, g, slots.m, slots.v, LR, B1, B2, 7, EPS)
    e2, mage = LT.ema(slots.e, p2, OMD)
    got = dict(p=bed.get(bed.store.theta), m=bed.get(bed.opt.m), v=bed.get(bed.opt.v), e=bed.get(ema_t))
    start = dict(p=slots.p, m=slots.m, v=slots.v, e=slots.e)
    ref = dict(p=p2, m=m2, v=v2, e=e2 if with_ema else slots.e)
    mags = dict(mag, e=np.maximum(mage, mag['p']))
    sl = slice(e0, e1)
    for key, k in (('m', LT.K_M), ('v', LT.K_V), ('p', LT.K_P), ('e', LT.K_P + LT.K_E)):
      for part in (slice(0, e0), slice(e1, None)):
        LT.assert_bit_equal(got[key][part], LT.f32(start[key][part]), f'{key} outside [e0, e1)', layout='flat')
      ratio = LT.bound_ratio(got[key][sl], ref[key][sl], k, mags[key][sl])
      print(f'apply_segment ema={with_ema} {key}: kernel / bound {ratio:.3f}', flush=True)
      assert ratio <= 1.0, (key, ratio)
    reach('adam_ema_kernel' if with_ema else 'adam_kernel', 'e0 % 256 != 0', f'[{e0}, {e1})')
  # se3ds_multi_ema alone: fp32 inputs ema, theta
  ema_t = torch.empty_like(bed.store.theta)
  bed.put(ema_t, slots.e)
  bed.put(bed.store.theta, slots.p)
  _lib.check(_L().se3ds_multi_ema(ema_t.data_ptr() + 4 * e0, bed.store.theta.data_ptr() + 4 * e0, e1 - e0,
                                  OMD, _lib.stream()), 'se3ds_multi_ema')
  e2, mage = LT.ema(slots.e, slots.p, OMD)
  got = bed.get(ema_t)
  for part in (slice(0, e0), slice(e1, None)):
    LT.assert_bit_equal(got[part], LT.f32(slots.e[part]), 'ema outside [e0, e1)', layout='flat')
  ratio = LT.bound_ratio(got[e0:e1], e2[e0:e1], LT.K_E, mage[e0:e1])
  print(f'se3ds_multi_ema: kernel / bound {ratio:.3f}', flush=True)
  assert ratio <= 1.0
  reach('ema_kernel', 'e0 % 256 != 0', f'[{e0}, {e1})')


# ---------------------------------------------------------------------------------------------
# power iteration

@pytest.mark.parametrize('training', [0, 1])
def test_power_iteration(bed, training):
  """v, uhat, u, sig against float64 at every spectral shape of the table.  Tolerance per shape:
  8 x the largest scaled error (max |x - ref| / max |ref| over v, uhat, sigma, 1 / sigma) of the
  fp32 NumPy restatement LT.power_iteration(dtype=float32) on the same W and u.  Floors measured
  on these inputs: 1.9e-8 (K 27, Cout 1, training 1) ... 9.4e-7 (K 9216, Cout 1024); the kernels
  on an MI355X stay below 2.7e-7 everywhere, worst kernel / floor 1.24 (training 0) and 6.84
  (training 1, the K 27 layer with the smallest floor).  Both figures are printed per layer."""
  r = LT.rng(5 + training)
  Ws, us = {}, {}
  for n, (K, C) in bed.KC.items():
    Ws[n] = LT.f32(r.standard_normal((K, C)) * 0.05).astype(np.float64)
    us[n] = LT.f32(r.standard_normal(C)).astype(np.float64)
    bed.put(bed.store.views[n], Ws[n].reshape(bed.store.views[n].shape))
    l = bed.layer_of[n]
    bed.put(l.store[l.name + '/u'], us[n].reshape(1, C))
    for key in ('v', 'uhat', 'sig', 'part', 'vpart'):
      l.sn[key].fill_(float('nan'))
  bed.spectral.power_iteration(training)
  rows = _L().se3ds_spectral_part_rows()
  worst = 0.0
  for n, (K, C) in bed.KC.items():
    l = bed.layer_of[n]
    ref = LT.power_iteration(Ws[n], us[n])
    r32 = LT.power_iteration(Ws[n], us[n], np.float32)
    keys = ('v', 'uhat', 'sigma', 'inv')
    floor = max(LT.scaled_err(r32[k], ref[k]) for k in keys)
    sig = bed.get(l.sn['sig'])
    got = dict(v=bed.get(l.sn['v']), uhat=bed.get(l.sn['uhat']), sigma=sig[0], inv=sig[1])
    errs = {k: LT.scaled_err(got[k], ref[k]) for k in keys}
    u_now = bed.get(l.store[l.name + '/u']).reshape(-1)
    print(f'power iteration {n} K {K} C {C} training {training}: fp32 floor {floor:.2e}, kernel '
          + ' '.join(f'{k}={e:.2e}' for k, e in errs.items()), flush=True)
    assert floor > 0
    for k, e in errs.items():
      assert e <= 8 * floor, (n, k, e, floor)
    worst = max(worst, max(errs.values()) / floor)
    if training:
      LT.assert_bit_equal(u_now, got['uhat'], f'{n}: u := uhat', layout='flat')
    else:
      LT.assert_bit_equal(u_now, LT.f32(us[n]), f'{n}: u unchanged', layout='flat')
    if K < 256:
      reach('sn_v_kernel', 'K < 256 (waves without a row)', f'{n}: K {K}')
    if -(-K // rows) * (rows - 1) >= K:
      reach('sn_u_kernel', 'empty slabs', f'{n}: K {K}, {rows} slabs of {-(-K // rows)}')
    reach('sn_finish_kernel', f'training {training}', n)
  print(f'power iteration training {training}: worst kernel / floor {worst:.2f}')


# ---------------------------------------------------------------------------------------------
# loss and head kernels (C ABI)

SIZES = [(1, 1, 1), (3, 8191, 3), (2, 512 * 1024, 3), (8, 512 * 1024, 1)]


def d32(a):
  return torch.from_numpy(np.asarray(a, np.float64).astype(np.float32)).to(DEV)


def host(t):
  torch.cuda.synchronize()
  return t.float().cpu().numpy()


def _pair(n, p, c, mode, seed):
  vals = LT.COARSE_DEPTHS if mode == 4 else (0.0, 1.0) if mode == 3 else LT.DEPTH_VALUES
  a = LT.pick((n, p, c), seed, vals)
  b = LT.pick((n, p, c), seed + 1, (0.0, 0.5, 1.0) if mode == 3 else vals)
  if a.size > 8:
    a.reshape(-1)[-3:] = b.reshape(-1)[-3:]
  return a, b


@pytest.mark.parametrize('size', SIZES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_sample_sum(mode, size):
  n, p, c = size
  a, b = _pair(n, p, c, mode, 10 * mode + n)
  masks = [None, LT.pick((n, p), 3, (0.0, 1.0))] if mode == 1 else [None]
  ws = torch.full((n * 256,), float('nan'), device=DEV)
  for m in masks:
    out = torch.full((n,), float('nan'), device=DEV)
    ta, tb, tm = d32(a), d32(b), None if m is None else d32(m)
    _lib.check(_L().se3ds_sample_sum(ta.data_ptr(), tb.data_ptr(), _lib.ptr(tm), n, p, c, mode,
                                     out.data_ptr(), ws.data_ptr(), _lib.stream()), 'se3ds_sample_sum')
    LT.assert_bit_equal(host(out), LT.sample_sum(a, b, m, mode), f'sample_sum mode {mode} {size}', layout='flat')
  chunks = -(-p * c // (BLOCK * 8))
  reach('sample_sum_kernel', 'chunk count capped at 256' if chunks > 256 else 'chunk count <= 256',
        f'P*C {p * c}: {chunks} chunks wanted')
  reach('sample_sum_kernel', f'mode {mode}', size)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_l1_grad(mode, size):
  n, p, c = size
  a, b = _pair(n, p, c, 0, 50 + mode + n)
  if a.size == 1:
    b = a.copy() if mode else np.full_like(a, 0.5)
    a = b.copy()
  m, m2 = LT.pick((n, p), 5, (0.0, 1.0)), LT.pick((n, p), 6, (0.0, 0.5, 1.0))
  coef = np.array([2.0 ** (i % 5 - 3) for i in range(n)])
  ta, tb, tc = d32(a), d32(b), d32(coef)
  tm, tm2 = (d32(m), d32(m2)) if mode in (1, 3) else (None, None)
  out = torch.full((n, p, c), float('nan'), device=DEV)
  _lib.check(_L().se3ds_l1_grad(ta.data_ptr(), tb.data_ptr(), _lib.ptr(tm), _lib.ptr(tm2), tc.data_ptr(),
                                n, p, c, mode, out.data_ptr(), _lib.stream()), 'se3ds_l1_grad')
  LT.assert_bit_equal(host(out), LT.l1_grad(a, b, m, m2, coef, mode), f'l1_grad mode {mode} {size}', layout='flat')
  reach('l1_grad_kernel', f'mode {mode}', size)


def test_recip_clamp():
  sums = np.array([0.0, 0.25, 0.5, 1.0, 1.5, 3.0, 8191.0, 24573.0, 1572864.0] + list(range(2, 300)))
  for scale in (1.0, 100.0, 10.0 / 3.0):
    out = torch.full((sums.size,), float('nan'), device=DEV)
    _lib.check(_L().se3ds_recip_clamp(d32(sums).data_ptr(), sums.size, scale, out.data_ptr(), _lib.stream()),
               'se3ds_recip_clamp')
    LT.assert_bit_equal(host(out), LT.recip_clamp(sums, scale), f'recip_clamp scale {scale}', layout='flat')
  reach('recip_clamp_kernel', 'sums below, at and above 1', sums.size)


@pytest.mark.parametrize('half', [1, 255, 256, 257, 8 * 30 * 62])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_hinge(dt, half):
  x = LT.pick((2 * half,), half, LT.LOGIT_VALUES)
  if half == 1:
    x = np.array([-1.0, 1.0])
  else:
    x[half:half + min(9, half)] = LT.LOGIT_VALUES[:min(9, half)]
    x[half - 1], x[-1] = -1.0, 1.0
  cd, cg = 0.5 / 4, 0.25
  sums, dd, dg = LT.hinge(x, cd, cg)
  LT.assert_on_lattice(torch.from_numpy(x), 'logits', 0.25, 2.0)   # exact in bf16
  logits = d32(x).to(dt)
  for seeds in ('both', 'd only', 'none'):
    out = torch.full((2,), float('nan'), device=DEV)
    td = torch.full((2 * half,), float('nan'), device=DEV, dtype=dt) if seeds != 'none' else None
    tg = torch.full((2 * half,), float('nan'), device=DEV, dtype=dt) if seeds == 'both' else None
    _lib.check(_L().se3ds_hinge(logits.data_ptr(), _lib.dtype_code(logits), half, cd, cg, out.data_ptr(),
                                _lib.ptr(td), _lib.ptr(tg), _lib.stream()), 'se3ds_hinge')
    LT.assert_bit_equal(host(out), sums, f'hinge sums {dt} half {half} seeds {seeds}', layout='flat')
    if td is not None:
      LT.assert_bit_equal(host(td), dd, 'dlog_d', layout='flat')
    if tg is not None:
      LT.assert_bit_equal(host(tg), dg, 'dlog_g', layout='flat')
  reach('hinge_kernel', 'bf16 logits' if dt == torch.bfloat16 else 'f32 logits', f'half {half}')


@pytest.mark.parametrize('n', [1, 3 * 8191 + 1, (1 << 20) + 3])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_depth_head_is_bit_exact(dt, n):
  x = LT.pick((n,), n, (0.0, 1.0, -0.5, 0.25, 1.5, 0.75, -2.0, 3.0))
  if n == 1:
    x[:] = 1.0
  dy = LT.pick((n,), n + 1, (0.5, -2.0, 1.0, 0.125))
  tx = d32(x).to(dt)
  y = torch.full((n,), float('nan'), device=DEV)
  _lib.check(_L().se3ds_head_fwd(tx.data_ptr(), _lib.dtype_code(tx), n, 1, y.data_ptr(), _lib.stream()), 'head_fwd')
  LT.assert_bit_equal(host(y), LT.f32(LT.head_fwd(x, 1)), f'depth head {dt}', layout='flat')
  dx = torch.full((n,), float('nan'), device=DEV, dtype=dt)
  _lib.check(_L().se3ds_head_bwd(d32(dy).data_ptr(), y.data_ptr(), tx.data_ptr(), _lib.dtype_code(tx), n, 1,
                                 dx.data_ptr(), _lib.stream()), 'head_bwd')
  LT.assert_bit_equal(host(dx), LT.f32(LT.head_bwd(dy, None, x, 1)), f'depth head backward {dt}', layout='flat')
  reach('head kernels', f'depth {str(dt)[6:]}', n)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_rgb_head_against_float64_tanh(dt):
  """(tanh(x) + 1) / 2 and its backward against float64; tolerance 8 x the scaled error of the
  fp32 NumPy restatement on the same x (floors measured here: forward 6.0e-8 on fp32 x and 5.7e-8
  on bf16 x, backward 4.5e-8; the kernels on an MI355X: 5.3e-8, 4.7e-8 and 3.0e-8; all printed).
  The backward runs on fp32 x only: its bf16 store would dominate."""
  n = 3 * 8191 + 1
  x = LT.f32(LT.rng(9).standard_normal(n) * 2)
  x[:4] = (0.0, 10.0, -10.0, 1e-3)
  tx = torch.from_numpy(x).to(DEV).to(dt)
  x = tx.float().cpu().numpy()
  y = torch.full((n,), float('nan'), device=DEV)
  _lib.check(_L().se3ds_head_fwd(tx.data_ptr(), _lib.dtype_code(tx), n, 0, y.data_ptr(), _lib.stream()), 'head_fwd')
  ref, r32 = LT.head_fwd(x, 0), LT.head_fwd(x, 0, np.float32)
  floor, err = LT.scaled_err(r32, ref), LT.scaled_err(host(y), ref)
  print(f'rgb head {dt}: fp32 floor {floor:.2e}, kernel {err:.2e}', flush=True)
  assert 0 < floor and err <= 8 * floor
  if dt == torch.float32:
    dy = LT.pick((n,), 3, (0.5, -2.0, 1.0, 0.125))
    yk = host(y)
    dx = torch.full((n,), float('nan'), device=DEV)
    _lib.check(_L().se3ds_head_bwd(d32(dy).data_ptr(), y.data_ptr(), tx.data_ptr(), 0, n, 0, dx.data_ptr(),
                                   _lib.stream()), 'head_bwd')
    ref, r32 = LT.head_bwd(dy, yk, None, 0), LT.head_bwd(dy, yk, None, 0, np.float32)
    floor, err = LT.scaled_err(r32, ref), LT.scaled_err(host(dx), ref)
    print(f'rgb head backward: fp32 floor {floor:.2e}, kernel {err:.2e}', flush=True)
    assert 0 < floor and err <= 8 * floor
  reach('head kernels', f'rgb {str(dt)[6:]}', n)


def test_bad_shapes_and_dtypes_return_their_codes():
  L = _L()
  t = torch.zeros(1024, device=DEV)
  p, s = t.data_ptr(), _lib.stream()
  BADSHAPE, BADDTYPE, WORKSPACE = -1, -2, -3
  assert L.se3ds_sample_sum(p, p, None, 0, 4, 1, 0, p, p, s) == BADSHAPE
  assert L.se3ds_sample_sum(p, p, None, 1, 0, 1, 0, p, p, s) == BADSHAPE
  assert L.se3ds_sample_sum(p, p, None, 1, 4, 0, 0, p, p, s) == BADSHAPE
  assert L.se3ds_sample_sum(p, p, None, 1, 4, 1, 0, p, None, s) == WORKSPACE
  assert L.se3ds_l1_grad(p, p, None, None, p, 0, 4, 1, 0, p, s) == BADSHAPE
  assert L.se3ds_l1_grad(p, p, None, None, p, 1, 0, 1, 0, p, s) == BADSHAPE
  assert L.se3ds_hinge(p, _lib.F32, 0, 1.0, 1.0, p, None, None, s) == BADSHAPE
  for bad in (_lib.I32, _lib.U8, 17):
    assert L.se3ds_hinge(p, bad, 4, 1.0, 1.0, p, None, None, s) == BADDTYPE
    assert L.se3ds_head_fwd(p, bad, 4, 1, p, s) == BADDTYPE
    assert L.se3ds_head_bwd(p, p, p, bad, 4, 1, p, s) == BADDTYPE
  torch.cuda.synchronize()
  assert not host(t).any()


# ---------------------------------------------------------------------------------------------
# coverage table

REQUIRED = [
    ('clip_kernel', 'dq == 0 (Cout > 256)'), ('clip_kernel', 'Cout == 1'), ('clip_kernel', 'Cout % 4 != 0'),
    ('clip_kernel', 'chunk from the middle of a tensor'), ('clip_kernel', 'plain tensor'),
    ('clip_adam_kernel', 'uhat as float4'), ('clip_adam_kernel', 'scalar tail (len % 4 != 0)'),
    ('clip_adam_kernel', 'C & 3 fallback'), ('clip_adam_kernel', 'chunk from the middle of a tensor'),
    ('clip_adam_kernel', 'with EMA'), ('clip_adam_kernel', 'without EMA'),
    ('sn_dots_kernel', 'scalar branch (Cout % 4 != 0)'), ('sn_dots_kernel', 'vector'),
    ('sn_dots_kernel', 'K < 256 (waves without a row)'), ('sn_v_kernel', 'K < 256 (waves without a row)'),
    ('sn_u_kernel', 'empty slabs'),
    ('se3ds_multi_sqnorm_sn', 'tensor_base != 0, segment starts on a plain tensor'),
    ('se3ds_multi_sqnorm_sn', 'tensor_base != 0, segment starts on a spectral tensor'),
    ('sample_sum_kernel', 'chunk count capped at 256'), ('hinge_kernel', 'bf16 logits'),
]


def test_coverage_table():
  for (kernel, cls), detail in sorted(REACHED.items()):
    print(f'reached {kernel:24s} {cls:36s} {detail}')
  missing = [r for r in REQUIRED if r not in REACHED]
  assert not missing, missing
