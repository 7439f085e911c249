"""GPU parity tests: HIP network kernels (through the C ABI) vs the PyTorch-CPU oracle.

Tolerances (north_star: "generator activations and grads within 1e-3 rel fp32"):
  fp32 path  : max |a-b| <= 1e-3 * max|b| per tensor (most tensors are ~1e-5)
  bf16 path  : 1e-2 * max|b| (bf16 has 8 mantissa bits; operands are rounded to bf16, the
               accumulation is fp32; the suite also passes at 6e-3 -- SE3DS_TEST_BF16_TOL overrides).
               The per-output-type bars (fp32-stored outputs of the bf16 path 1e-4, bf16-stored
               6e-3) are in test_prod_shapes_gpu.py, on bf16-representable inputs.
"""
import os

import numpy as np
import pytest
import torch

from oracle import nets_torch as O
from se3ds_amd import _lib
from se3ds_amd import gin_lite
from se3ds_amd.hipops import nn
from se3ds_amd.models import image_models
from se3ds_amd.models import layers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def rel_err(a, b):
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-12))


def tol(dtype):
  return 1e-3 if dtype == torch.float32 else float(os.environ.get('SE3DS_TEST_BF16_TOL', '1e-2'))


def to_dev(x, dtype):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)


def _mk_layer(kind, cin, cout, k, stride, padding, bias, seed, transpose=False):
  store = nn.ParamStore()
  layer = nn.ConvLayer(store, 'c', cin, cout, k, stride, padding, bias, kind, transpose=transpose)
  store.finalize(DEV, torch.Generator().manual_seed(seed))
  if bias:
    store['c/bias'].copy_(torch.randn(cout, generator=torch.Generator().manual_seed(seed + 1)).to(DEV) * 0.1)
  sg = nn.SpectralGroup([layer], torch.device(DEV))
  return store, layer, sg


CONV_CASES = [
    # kind, cin, cout, k, stride, padding, pad, wrap, bias, mask, n, h, w
    ('plain', 32, 64, 3, 1, 'VALID', 1, False, True, False, 2, 16, 32),
    ('plain', 32, 64, 3, 1, 'VALID', 1, True, False, False, 1, 16, 32),
    ('spectral', 64, 160, 3, 1, 'VALID', 1, False, True, False, 2, 8, 16),
    ('spectral', 32, 32, 4, 2, 'VALID', 2, False, True, False, 2, 18, 34),
    ('spectral', 64, 32, 1, 1, 'SAME', 0, False, True, False, 2, 9, 17),
    ('partial', 5, 16, 7, 2, 'VALID', 3, False, True, True, 2, 32, 64),
    ('partial_spectral', 32, 32, 3, 2, 'VALID', 1, False, True, True, 2, 16, 32),
    ('partial_spectral', 32, 128, 1, 2, 'SAME', 0, False, False, True, 2, 16, 32),
    ('partial_spectral', 48, 32, 1, 1, 'SAME', 0, False, False, False, 1, 8, 16),
    ('plain', 4, 16, 4, 2, 'VALID', 2, False, True, False, 2, 32, 64),
    ('plain', 64, 1, 4, 1, 'SAME', 0, False, True, False, 2, 10, 18),
    ('plain', 8, 8, 3, 1, 'VALID', 1, False, False, False, 1, 12, 24),
    ('spectral', 64, 3, 3, 1, 'VALID', 1, False, True, False, 2, 12, 20),   # thin Cout: swapped wgrad
    ('plain', 32, 1, 3, 1, 'VALID', 1, False, True, False, 2, 20, 36),
]


# shapes the 256-pixel macro-tile kernels accept (bf16, Cout % 128 == 0 and/or Cin % 128 == 0 for
# the data gradient, reduction channels % 64 == 0); run with SE3DS_BIG_TILE=1 so that the cost
# model cannot route these small problems back to the 128 x 128 kernel
BIG_TILE_CASES = [
    ('spectral', 64, 256, 3, 1, 'VALID', 1, False, True, False, 2, 16, 32),
    ('plain', 128, 128, 3, 1, 'VALID', 1, True, False, False, 1, 16, 32),      # circular width
    ('spectral', 256, 256, 1, 1, 'SAME', 0, False, True, False, 2, 9, 17),     # ragged pixel tiles
    ('spectral', 128, 256, 4, 2, 'VALID', 2, False, True, False, 2, 18, 34),   # parity classes
    ('partial_spectral', 64, 128, 3, 2, 'VALID', 1, False, True, True, 2, 16, 32),
    ('partial_spectral', 128, 128, 3, 1, 'VALID', 1, False, True, True, 2, 16, 32),
    ('plain', 512, 256, 3, 1, 'VALID', 1, False, True, False, 3, 11, 23),      # several taps x K steps
    ('spectral', 192, 128, 3, 1, 'VALID', 1, False, True, False, 1, 20, 70),   # 3 slabs, ragged tiles
    ('plain', 64, 128, 3, 1, 'SAME', 0, False, False, False, 2, 8, 32),        # one slab, SAME pad
    # more than 256 work items: the persistent halo kernel takes several items per workgroup
    ('plain', 64, 128, 3, 1, 'VALID', 1, False, True, False, 3, 128, 256),
    ('spectral', 128, 256, 3, 1, 'VALID', 1, False, True, False, 3, 128, 256),
    ('plain', 128, 128, 3, 1, 'VALID', 1, False, True, False, 3, 128, 256),    # two slabs per item
]


# the generator's heads: 3x3 onto <= 4 channels (thin_cout_fwd_kernel; thin weight gradients)
THIN_CASES = [
    ('spectral', 128, 3, 3, 1, 'VALID', 1, False, True, False, 2, 12, 64),
    ('spectral', 128, 1, 3, 1, 'VALID', 1, False, True, False, 2, 9, 37),     # ragged tiles
    ('plain', 64, 3, 3, 1, 'VALID', 1, True, False, False, 1, 16, 32),        # circular width
    ('plain', 256, 4, 3, 1, 'SAME', 0, False, True, False, 1, 7, 45),         # SAME padding, 4 rows
    # the weight-gradient kernel's other instantiations: 9 * Cin / 32 column tiles dealt to 8 waves
    # = 2 per wave (Cin 32), 4 (Cin 96: also the only channel count whose patch fetch takes the
    # generic, non-power-of-two indexing)
    ('spectral', 32, 3, 3, 1, 'VALID', 1, False, True, False, 2, 17, 40),
    ('plain', 96, 2, 3, 1, 'VALID', 1, False, False, False, 1, 20, 70),
]


@pytest.mark.parametrize('case', THIN_CASES)
def test_conv_thin_cout(case):
  _run_conv_case(case, torch.bfloat16)


# first layers: <= 8 input channels onto a multiple of 128 (thin_cin_fwd_kernel)
THIN_CIN_CASES = [
    ('partial', 5, 128, 7, 2, 'VALID', 3, False, True, True, 2, 32, 64),      # generator conv1
    ('plain', 4, 128, 4, 2, 'VALID', 2, False, True, False, 2, 34, 66),       # discriminator conv1
    ('plain', 4, 256, 3, 1, 'VALID', 1, True, False, False, 1, 12, 40),       # two channel groups, wrap
    ('spectral', 8, 128, 3, 2, 'VALID', 1, False, True, False, 3, 19, 45),    # ragged tiles
    ('plain', 3, 128, 4, 2, 'VALID', 2, False, False, False, 1, 70, 130),     # stride-2 thin data gradient, 2 x 3 tiles
    ('spectral', 4, 128, 4, 2, 'VALID', 0, False, True, False, 2, 20, 36),    # no padding
]


@pytest.mark.parametrize('case', THIN_CIN_CASES)
def test_conv_thin_cin(case):
  _run_conv_case(case, torch.bfloat16)


@pytest.mark.parametrize('case', THIN_CASES[:2] + THIN_CIN_CASES[:2] + THIN_CIN_CASES[4:5])
def test_conv_thin_layers_through_the_general_kernels(case, monkeypatch):
  """SE3DS_NO_THIN=1: heads and stems through the general implicit-GEMM kernels (the routing of
  round 1) against the same oracle and tolerance -- the switch that separates a thin-kernel fault
  from a model fault keeps working."""
  monkeypatch.setenv('SE3DS_NO_THIN', '1')
  _run_conv_case(case, torch.bfloat16)


@pytest.mark.parametrize('halo', ['0', '1'])
@pytest.mark.parametrize('case', BIG_TILE_CASES)
def test_conv_macro_tile_fwd_bwd(case, halo, monkeypatch):
  """halo=1: stride-1 3x3 cases run the halo-resident kernel; halo=0: the generic macro tile."""
  monkeypatch.setenv('SE3DS_BIG_TILE', '1')
  monkeypatch.setenv('SE3DS_HALO_TILE', halo)
  _run_conv_case(case, torch.bfloat16)


@pytest.mark.parametrize('big', ['0', '1'])
@pytest.mark.parametrize('case', BIG_TILE_CASES)
def test_conv_lds_dma_kernels_mfma_32x32x16(case, big, monkeypatch):
  """SE3DS_HALO_M16=0: the 256-pixel macro tile (big=1) and the 128 x 128 tile (big=0) with the
  32x32x16 MFMA shape (the default since round 4 is 16x16x32, which every other test runs)."""
  monkeypatch.setenv('SE3DS_BIG_TILE', big)
  monkeypatch.setenv('SE3DS_HALO_TILE', '0')
  monkeypatch.setenv('SE3DS_HALO_M16', '0')
  _run_conv_case(case, torch.bfloat16)


@pytest.mark.parametrize('case', [c for c in BIG_TILE_CASES if c[2] % 128 == 0 and c[3] == 3 and c[4] == 1] + [
    ('partial_spectral', 128, 256, 3, 1, 'VALID', 1, False, True, True, 2, 24, 40),   # gather mask, ragged tiles
    ('plain', 256, 512, 3, 1, 'VALID', 1, True, False, False, 1, 16, 64),            # circular width, 2 channel tiles
])
@pytest.mark.parametrize('m16', ['0', '1'])
def test_conv_halo_mfma_shapes(case, m16, monkeypatch):
  """The 8-wave halo kernels with v_mfma_f32_16x16x32_bf16 (SE3DS_HALO_M16=1, the default: other
  fragment and accumulator layouts, own epilogue parking) and with 32x32x16 (=0); forward, data
  gradient and the fused statistics."""
  monkeypatch.setenv('SE3DS_BIG_TILE', '1')
  monkeypatch.setenv('SE3DS_HALO_TILE', '1')
  monkeypatch.setenv('SE3DS_HALO_M16', m16)
  _run_conv_case(case, torch.bfloat16)


@pytest.mark.parametrize('k,cin,cout', [(3, 128, 128), (2, 64, 256)])
def test_conv_transpose_macro_tile(k, cin, cout, monkeypatch):
  monkeypatch.setenv('SE3DS_BIG_TILE', '1')
  test_conv_transpose_fwd_bwd(k, cin, cout, True, torch.bfloat16)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('case', CONV_CASES)
def test_conv_fwd_bwd(case, dtype):
  _run_conv_case(case, dtype)


def _run_conv_case(case, dtype):
  kind, cin, cout, k, stride, padding, pad, wrap, bias, use_mask, n, h, w = case
  store, layer, sg = _mk_layer(kind, cin, cout, k, stride, padding, bias, 7)
  gen = torch.Generator().manual_seed(11)
  x = torch.randn((n, h, w, cin), generator=gen)
  mask = (torch.rand((n, h, w, 1), generator=gen) > 0.4).float() if use_mask else None
  if dtype == torch.bfloat16:   # compare against the oracle on bf16-representable inputs
    x = x.bfloat16().float()
  # ---- oracle
  p = {kk: v.detach().cpu().clone() for kk, v in store.views.items()}
  if dtype == torch.bfloat16:
    p['c/kernel'] = p['c/kernel'].bfloat16().float()
  xo = x.clone().requires_grad_(True)
  ko = p['c/kernel'].clone().requires_grad_(True)
  p['c/kernel'] = ko
  if bias:
    p['c/bias'] = p['c/bias'].clone().requires_grad_(True)
  net = O.Net(p, training=not wrap)
  xin = O.pad_layer(xo, pad, circular_pad=wrap, training=not wrap) if pad else xo
  if kind.startswith('partial'):
    m_in = None
    if mask is not None:
      m_in = O.pad_layer(mask, pad, circular_pad=wrap, training=not wrap) if pad else mask
    yo, umo = net.partial_conv(xin, m_in, 'c', stride, padding, spectral=kind == 'partial_spectral')
  elif kind == 'spectral':
    yo = net.spectral_conv(xin, 'c', stride, padding)
  else:
    yo = net.conv2d(xin, 'c', stride, padding)
  gy = torch.randn(yo.shape, generator=gen)
  if dtype == torch.bfloat16:
    gy = gy.bfloat16().float()
  yo.backward(gy)
  # ---- HIP
  ctx = nn.Ctx(DEV, dtype, training=not wrap, record=True)
  if dtype == torch.bfloat16:
    store.load_dict({'c/kernel': p['c/kernel'].detach().numpy()})
  sg.power_iteration(training=False)
  xv = nn.Var(to_dev(x.numpy(), dtype), requires_grad=True)
  mdev = to_dev(mask.numpy()[..., 0], torch.float32) if mask is not None else None
  res = nn.conv2d(ctx, xv, layer, pad=pad, wrap=wrap, mask=mdev)
  if kind.startswith('partial'):
    yv, um = res
    np.testing.assert_array_equal(um.cpu().numpy(), umo.detach().numpy()[..., 0])
  else:
    yv = res
  t = tol(dtype)
  assert rel_err(yv.data.float().cpu().numpy(), yo.detach().numpy()) < t
  yv.grad = to_dev(gy.numpy(), dtype)
  ctx.backward()
  sg.backward_fixup()
  assert rel_err(xv.grad.float().cpu().numpy(), xo.grad.numpy()) < t
  assert rel_err(store.grad_views['c/kernel'].cpu().numpy(), ko.grad.numpy()) < t
  if bias:
    assert rel_err(store.grad_views['c/bias'].cpu().numpy(), p['c/bias'].grad.numpy()) < t


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('k,cin,cout,bias', [(3, 64, 32, False), (2, 32, 32, False), (2, 32, 48, True),
                                             (3, 8, 4, False), (2, 4, 4, True)])
def test_conv_transpose_fwd_bwd(k, cin, cout, bias, dtype):
  store, layer, _ = _mk_layer('plain', cin, cout, k, 2, 'SAME', bias, 21, transpose=True)
  gen = torch.Generator().manual_seed(5)
  n, h, w = 2, 6, 10
  x = torch.randn((n, h, w, cin), generator=gen)
  kern = store['c/kernel'].cpu().clone()
  if dtype == torch.bfloat16:
    x = x.bfloat16().float()
    kern = kern.bfloat16().float()
    store.load_dict({'c/kernel': kern.numpy()})
  xo = x.clone().requires_grad_(True)
  ko = kern.clone().requires_grad_(True)
  bo = store['c/bias'].cpu().clone().requires_grad_(True) if bias else None
  yo = O.keras_conv2d_transpose(xo, ko, bo, 2)
  gy = torch.randn(yo.shape, generator=gen)
  if dtype == torch.bfloat16:
    gy = gy.bfloat16().float()
  yo.backward(gy)
  ctx = nn.Ctx(DEV, dtype, training=True, record=True)
  xv = nn.Var(to_dev(x.numpy(), dtype), requires_grad=True)
  yv = nn.conv_transpose2d(ctx, xv, layer)
  t = tol(dtype)
  assert tuple(yv.data.shape) == (n, 2 * h, 2 * w, cout)
  assert rel_err(yv.data.float().cpu().numpy(), yo.detach().numpy()) < t
  yv.grad = to_dev(gy.numpy(), dtype)
  ctx.backward()
  assert rel_err(xv.grad.float().cpu().numpy(), xo.grad.numpy()) < t
  assert rel_err(store.grad_views['c/kernel'].cpu().numpy(), ko.grad.numpy()) < t
  if bias:
    assert rel_err(store.grad_views['c/bias'].cpu().numpy(), bo.grad.numpy()) < t


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('kind,c,act,with_res,training', [
    ('batch', 32, nn.ACT_RELU, True, True), ('batch', 4, nn.ACT_NONE, False, True),
    ('batch', 64, nn.ACT_LRELU, False, False), ('instance', 32, nn.ACT_LRELU, False, True),
    ('instance', 6, nn.ACT_LRELU, False, True)])
def test_norm_fwd_bwd(kind, c, act, with_res, training, dtype):
  store = nn.ParamStore()
  layer = nn.NormLayer(store, 'n', c, kind)
  store.finalize(DEV, None)
  gen = torch.Generator().manual_seed(3)
  store.load_dict({'n/gamma': (torch.rand(c, generator=gen) + 0.5).numpy(),
                   'n/beta': (torch.randn(c, generator=gen) * 0.2).numpy()})
  if kind == 'batch':
    store.load_dict({'n/moving_mean': (torch.randn(c, generator=gen) * 0.1).numpy(),
                     'n/moving_variance': (torch.rand(c, generator=gen) + 0.5).numpy()})
  n, h, w = 3, 9, 14
  x = torch.randn((n, h, w, c), generator=gen) * 1.5 + 0.3
  r = torch.randn((n, h, w, c), generator=gen)
  gy = torch.randn((n, h, w, c), generator=gen)
  if dtype == torch.bfloat16:
    x, r, gy = x.bfloat16().float(), r.bfloat16().float(), gy.bfloat16().float()
  alpha = 0.2
  p = {k: v.cpu().clone() for k, v in store.views.items()}
  p['n/gamma'].requires_grad_(True)
  p['n/beta'].requires_grad_(True)
  xo, ro = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
  net = O.Net(p, training=training)
  yo = net.sync_bn(xo, 'n') if kind == 'batch' else net.instance_norm(xo, 'n')
  if with_res:
    yo = yo + ro
  if act == nn.ACT_RELU:
    yo = torch.relu(yo)
  elif act == nn.ACT_LRELU:
    yo = O.leaky_relu(yo, alpha)
  yo.backward(gy)
  ctx = nn.Ctx(DEV, dtype, training=training, record=True)
  xv = nn.Var(to_dev(x.numpy(), dtype))
  rv = nn.Var(to_dev(r.numpy(), dtype)) if with_res else None
  yv = nn.norm_act(ctx, xv, layer, act=act, alpha=alpha, res=rv)
  t = tol(dtype)
  assert rel_err(yv.data.float().cpu().numpy(), yo.detach().numpy()) < t
  if kind == 'batch' and training:
    for nm in ('moving_mean', 'moving_variance'):
      assert rel_err(store['n/' + nm].cpu().numpy(), net.updates['n/' + nm].numpy()) < 1e-5
  yv.grad = to_dev(gy.numpy(), dtype)
  ctx.backward()
  assert rel_err(xv.grad.float().cpu().numpy(), xo.grad.numpy()) < 2 * t
  assert rel_err(store.grad_views['n/gamma'].cpu().numpy(), p['n/gamma'].grad.numpy()) < 2 * t
  assert rel_err(store.grad_views['n/beta'].cpu().numpy(), p['n/beta'].grad.numpy()) < 2 * t
  if with_res:
    assert rel_err(rv.grad.float().cpu().numpy(), ro.grad.numpy()) < t


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pools_and_upsample(dtype):
  gen = torch.Generator().manual_seed(9)
  for (h, w) in ((8, 12), (9, 13)):
    x = torch.randn((2, h, w, 8), generator=gen)
    if dtype == torch.bfloat16:
      x = x.bfloat16().float()
    for name, fn_o, fn_g in (('max', O.max_pool_same, nn.maxpool2x2),
                             ('avg', O.avg_pool3s2_same, nn.avgpool3s2),
                             ('up', lambda t: t.repeat_interleave(2, 1).repeat_interleave(2, 2),
                              nn.upsample2x)):
      xo = x.clone().requires_grad_(True)
      yo = fn_o(xo)
      gy = torch.randn(yo.shape, generator=gen)
      if dtype == torch.bfloat16:
        gy = gy.bfloat16().float()
      yo.backward(gy)
      ctx = nn.Ctx(DEV, dtype, training=True, record=True)
      xv = nn.Var(to_dev(x.numpy(), dtype))
      yv = fn_g(ctx, xv)
      assert rel_err(yv.data.float().cpu().numpy(), yo.detach().numpy()) < tol(dtype), name
      yv.grad = to_dev(gy.numpy(), dtype)
      ctx.backward()
      assert rel_err(xv.grad.float().cpu().numpy(), xo.grad.numpy()) < tol(dtype), name


def test_pad_layer_golden_on_gpu(golden_dir):
  # models/layers_test.py:136-179 through the product PadLayer
  g = np.load(os.path.join(golden_dir, 'reference_literals.npz'))
  x = torch.from_numpy(g['pad_input']).reshape(1, 4, 4, 1).to(DEV)
  out = layers.PadLayer(2, True)(x)
  np.testing.assert_array_equal(out[0, :, :, 0].cpu().numpy(), g['pad_const_circ'])
  out = layers.PadLayer(2, False)(x)
  np.testing.assert_array_equal(out[0, :, :, 0].cpu().numpy(), g['pad_const_nocirc'])
  out = layers.PadLayer(2, True, mode='SYMMETRIC')(x)
  np.testing.assert_array_equal(out[0, :, :, 0].cpu().numpy(), g['pad_symm_circ'])
  out = layers.PadLayer(2, True)(x, training=True)
  np.testing.assert_array_equal(out[0, :, :, 0].cpu().numpy(), g['pad_const_nocirc'])


def synth_batch(n, h, seed=1234):
  """SURVEY 8d synthetic inputs."""
  g = torch.Generator().manual_seed(seed)
  w = 2 * h
  image = torch.rand((n, h, w, 3), generator=g)
  depth = torch.rand((n, h, w, 1), generator=g)
  poison = torch.rand((n, h, w, 1), generator=g)
  depth = torch.where(poison < 0.02, torch.zeros_like(depth), depth)
  depth = torch.where(poison > 0.99, torch.ones_like(depth), depth)
  pm = (torch.rand((n, h, w, 1), generator=g) < 0.5).float()
  pm[:, h // 3:h // 3 + max(1, h // 8)] = 0
  bm = torch.zeros((n, h, w, 1))
  bm[:, :h // 8] = 1
  bm[:, -(h // 8):] = 1
  return dict(image=image, depth=depth, proj_mask=pm, proj_image=image * pm,
              proj_depth=depth * pm, blurred_mask=bm)


def capture_clipped_grads(opt):
  """CPU copy of the gradient arena exactly as Adam consumes it (AdamState.on_update fires per
  updated range: once for the whole arena, or per module when the trainer updates modules on its
  side stream).  Returns (arena tensor filled during the step, name -> view function)."""
  st = opt.model.store
  buf = torch.zeros(st.theta.numel(), dtype=torch.float32)
  def hook(e0, e1):
    buf[e0:e1] = st.grad[e0:e1].detach().cpu()
  opt.on_update = hook
  def view(name):
    o, n, shape = st._off_tr[name]
    return buf[o:o + n].view(shape)
  return buf, view


def _oracle_params(model):
  return {k: v.detach().cpu().clone() for k, v in model.store.views.items()}


def _f64(d):
  return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


class fp64_oracle:
  """Runs the oracle in binary64: the yardstick for what fp32 can deliver.  In TRAINING mode the
  toy configurations are ill-conditioned (batch-statistics BN over as few as 16 samples, 50+
  normalisation layers deep): the fp32 oracle itself drifts 1e-3..1e-2 from the fp64 result, so
  the HIP fp32 path is held to "as accurate as the fp32 reference path", i.e.
      err(hip, f64) <= ACC_FACTOR * err(oracle_f32, f64) + 1e-3."""

  def __enter__(self):
    torch.set_default_dtype(torch.float64)

  def __exit__(self, *a):
    torch.set_default_dtype(torch.float32)


ACC_FACTOR = 5.0


def close_to_f64(hip, o32, r64, what):
  """HIP fp32 result is within 1e-3 of the fp32 oracle, or as accurate as the fp32 oracle when
  both are measured against fp64 (factor ACC_FACTOR, + 1e-3).  No cosine fallback: a tensor that
  misses both bars fails."""
  e_direct = rel_err(hip, o32)
  e_hip, e_o32 = rel_err(hip, r64), rel_err(o32, r64)
  assert e_direct <= 1e-3 or e_hip <= ACC_FACTOR * e_o32 + 1e-3, (what, e_direct, e_hip, e_o32)
  return e_hip, e_o32


@pytest.mark.parametrize('size,version,context,training', [
    (64, '50', 'convs', True), (64, '50', 'convs', False), (128, '101', 'none', False)])
def test_generator_forward_parity_fp32(size, version, context, training):
  # image_models_test.py:28-75 shapes/ranges + values vs the oracle
  gin_lite.clear_config()
  G = image_models.ResNetGenerator(image_size=size, gen_dims=4, z_dim=4, resnet_version=version,
                                   context_layer=context, device=DEV, seed=3, dtype=torch.float32)
  batch = synth_batch(2, size)
  p = _oracle_params(G)
  outs_o, upd = O.generator_forward(p, batch, training, gen_dims=4, resnet_version=version,
                                    context_layer=context, z_dim=4)
  dbatch = {k: v.to(DEV) for k, v in batch.items()}
  outs = G([dbatch, None], training=training)
  assert len(outs) == 7
  assert tuple(outs[3].shape) == (2, size, 2 * size, 1) and tuple(outs[6].shape) == (2, size, 2 * size, 3)
  assert tuple(outs[4].shape) == (2, size, 2 * size, 42)
  assert tuple(outs[0].shape) == (2, size // 32, size // 16, 4)
  if training:
    with fp64_oracle():
      outs_64, upd64 = O.generator_forward(_f64(p), _f64(batch), training, gen_dims=4,
                                           resnet_version=version, context_layer=context, z_dim=4)
  for i in (3, 6):
    o = outs[i].cpu().numpy()
    assert o.min() >= 0 and o.max() <= 1
    if not training:
      assert rel_err(o, outs_o[i].detach().numpy()) < 1e-3, i
    else:
      ref64 = outs_64[i].detach().numpy()
      assert rel_err(o, ref64) <= ACC_FACTOR * rel_err(outs_o[i].detach().numpy(), ref64) + 1e-3, i
  if training:   # BN moving statistics and spectral u advanced identically
    for k, v in upd.items():
      ref64 = upd64[k].detach().numpy()
      assert rel_err(G.store[k].cpu().numpy(), ref64) <= \
          ACC_FACTOR * rel_err(v.detach().numpy(), ref64) + 1e-3, k
  with pytest.raises(ValueError):
    G([dbatch, None], sample_noise=True)


def test_generator_errors():
  with pytest.raises(NotImplementedError):
    image_models.ResNetGenerator(context_layer='attention', gen_dims=4, device=DEV)
  with pytest.raises(ValueError):
    image_models.ResNetGenerator(resnet_version='18', gen_dims=4, device=DEV)


@pytest.mark.parametrize('n_layers,kernel', [(5, 4), (3, 3)])
def test_discriminator_parity_fp32(n_layers, kernel):
  # image_models_test.py:77-104 structure + values vs the oracle
  D = image_models.SNMultiScaleDiscriminator(n_dis=2, dis_dims=4, n_layers=n_layers,
                                             kernel_size=kernel, device=DEV, seed=5)
  x = torch.rand((2, 64, 128, 4), generator=torch.Generator().manual_seed(1))
  res_o, _ = O.discriminator_forward(_oracle_params(D), x, False, n_dis=2, n_layers=n_layers,
                                     kernel_size=kernel)
  res = D(x.to(DEV))
  assert len(res) == 2
  for sub, sub_o in zip(res, res_o):
    assert len(sub) == n_layers + 1 and sub[-1].shape[-1] == 1
    for a, b in zip(sub, sub_o):
      assert tuple(a.shape) == tuple(b.shape)
      assert rel_err(a.cpu().numpy(), b.detach().numpy()) < 1e-3


def test_generator_backward_well_conditioned_fp32():
  """Every generator parameter gradient vs oracle autograd in a WELL-CONDITIONED setting:
  zero padding (training flag) but BN on moving statistics, random affine/bias values, random
  cotangents on rgb and depth.  No batch-statistics amplification => fp32 agreement ~1e-6."""
  G = image_models.ResNetGenerator(image_size=64, gen_dims=4, z_dim=4, resnet_version='50',
                                   device=DEV, seed=3)
  gen = torch.Generator().manual_seed(4)
  upd = {}
  for n in G.store.state_names:
    if n.endswith('moving_mean'):
      upd[n] = (torch.randn(G.store[n].shape, generator=gen) * 0.1).numpy()
    if n.endswith('moving_variance'):
      upd[n] = (torch.rand(G.store[n].shape, generator=gen) + 0.5).numpy()
  for n in G.store.trainable_names:
    if n.endswith('gamma'):
      upd[n] = (torch.rand(G.store[n].shape, generator=gen) + 0.5).numpy()
    if n.endswith('beta') or n.endswith('bias'):
      upd[n] = (torch.randn(G.store[n].shape, generator=gen) * 0.1).numpy()
  G.store.load_dict(upd)
  batch = synth_batch(2, 64)
  p = {k: v.detach().cpu().clone().requires_grad_(k in G.store.trainable_names)
       for k, v in G.store.views.items()}
  outs_o, _ = O.generator_forward(p, batch, True, gen_dims=4, resnet_version='50', z_dim=4,
                                  bn_training=False)
  w_rgb = torch.randn(outs_o[6].shape, generator=gen)
  w_d = torch.randn(outs_o[3].shape, generator=gen)
  ((outs_o[6] * w_rgb).sum() + (outs_o[3] * w_d).sum()).backward()
  ctx = G.make_ctx(True, record=True)
  ctx.bn_use_moving = True
  outs, (push_rgb, push_depth) = G.forward(ctx, {k: v.to(DEV) for k, v in batch.items()})
  assert rel_err(outs[6].cpu().numpy(), outs_o[6].detach().numpy()) < 1e-4
  assert rel_err(outs[3].cpu().numpy(), outs_o[3].detach().numpy()) < 1e-4
  push_rgb(w_rgb.to(DEV))
  push_depth(w_d.to(DEV))
  ctx.backward()
  G.spectral.backward_fixup()
  errs = []
  gmax = max(float(p[k].grad.abs().max()) for k in G.store.trainable_names)
  for k in G.store.trainable_names:
    go = p[k].grad.numpy()
    gh = G.store.grad_views[k].cpu().numpy()
    # absolute error relative to the largest gradient entry of the tensor, floored at 1e-5 of
    # the global gradient scale (partial-conv bias gradients are sums of +-1e-7 terms)
    err = float(np.abs(gh - go).max() / max(np.abs(go).max(), 1e-4 * gmax))
    errs.append(err)
    assert err < 1e-3, (k, err)
  assert np.median(errs) < 1e-5, np.median(errs)


def _cfg(gen_dims, version, n_layers):
  return dict(gen=dict(gen_dims=gen_dims, resnet_version=version, context_layer='convs', z_dim=4),
              dis=dict(n_dis=2, n_layers=n_layers, kernel_size=4),
              lambda_gan=1.0, lambda_kld=10.0, lambda_wc=10.0, lambda_depth=100.0,
              mask_blurred=True,
              g_train=lambda k: not k.endswith(('/u', '/moving_mean', '/moving_variance')),
              d_train=lambda k: not k.endswith('/u'))


def _make_gan(size, gen_dims, version, n_layers, dtype=torch.float32):
  from se3ds_amd.trainers import gan_manager, se3ds_trainer
  gin_lite.clear_config()
  gin_lite.parse_config(f'''
image_models.ResNetGenerator.gen_dims = {gen_dims}
image_models.ResNetGenerator.z_dim = 4
image_models.ResNetGenerator.resnet_version = "{version}"
image_models.SNMultiScaleDiscriminator.dis_dims = 4
image_models.SNMultiScaleDiscriminator.n_dis = 2
image_models.SNMultiScaleDiscriminator.n_layers = {n_layers}
''')
  gan = se3ds_trainer.GAN(
      strategy=gan_manager.OneDeviceStrategy(DEV), model_dir='', lambda_gan=1.0, lambda_kld=10.0,
      lambda_wc=10.0, lambda_depth=100.0, mask_blurred=True, predict_depth=True, image_size=size,
      beta1=0.5, g_lr=1e-4, d_lr=4e-4, d_step_per_g_step=1, num_batched_steps=1,
      generator_fn=image_models.ResNetGenerator,
      discriminator_fn=image_models.SNMultiScaleDiscriminator, seed=0, compute_dtype=dtype)
  gan._create_obj()
  return gan


def test_train_g_d_gradients_and_update_fp32():
  """One full train_g_d at toy dims vs the oracle: clipped gradients of every G and D tensor,
  Adam-updated weights, BN/SN state, EMA copy and the metric values."""
  size = 64
  gan = _make_gan(size, 4, '50', 3)
  batch = synth_batch(4, size, seed=77)
  gp, dp = _oracle_params(gan.generator), _oracle_params(gan.discriminator)
  cfg = _cfg(4, '50', 3)
  ref = O.train_g_d(gp, dp, batch, cfg)
  with fp64_oracle():
    ref64 = O.train_g_d(_f64(gp), _f64(dp), _f64(batch), cfg)
  # capture the clipped gradients before Adam consumes them
  views = {tag: capture_clipped_grads(opt)[1]
           for opt, tag in ((gan.g_optimizer, 'g'), (gan.d_optimizer, 'd'))}
  gan.train_g_d({k: v.to(DEV) for k, v in batch.items()})
  torch.cuda.synchronize()
  captured = {tag: {n: views[tag](n).numpy().copy() for n in opt.model.store.trainable_names}
              for opt, tag in ((gan.g_optimizer, 'g'), (gan.d_optimizer, 'd'))}
  # Training-mode gradients of this toy network are noise-limited in fp32 (see fp64_oracle):
  # per-tensor strictness lives in test_generator_backward_well_conditioned_fp32 and the
  # kernel-level tests; here the whole gradient vector must be as close to the fp64 result as
  # the fp32 oracle's is, and every tensor must point the same way.
  for tag, key in (('g', 'g_grads'), ('d', 'd_grads')):
    refg, refg64 = ref[key], ref64[key]
    assert set(refg) == set(captured[tag])
    num_h = num_o = den = 0.0
    for k in refg:
      r64 = refg64[k].numpy().ravel()
      a = captured[tag][k].astype(np.float64).ravel()
      b = refg[k].numpy().astype(np.float64).ravel()
      num_h += float(((a - r64) ** 2).sum()); num_o += float(((b - r64) ** 2).sum())
      den += float((r64 ** 2).sum())
      if np.abs(r64).max() > 1e-6:
        cos = float(a @ r64 / (np.linalg.norm(a) * np.linalg.norm(r64) + 1e-300))
        assert cos > 0.9, (tag, k, cos)
    e_hip, e_o32 = (num_h / den) ** 0.5, (num_o / den) ** 0.5
    print(f'{tag}: ||grad - f64|| / ||f64||: hip {e_hip:.3e}, fp32 oracle {e_o32:.3e}')
    assert e_hip <= ACC_FACTOR * e_o32 + 1e-3, (tag, e_hip, e_o32)
  # the discriminator has no batch statistics (instance norm): every one of its tensors is held
  # to the per-tensor bar (1e-3 of the fp32 oracle, or the fp64 yardstick), no fallback
  for k in ref['d_grads']:
    r64 = ref64['d_grads'][k].numpy()
    if float(np.abs(r64).max()) >= 1e-7:
      close_to_f64(captured['d'][k], ref['d_grads'][k].numpy(), r64, 'd/' + k)
  # Adam (Keras form), applied to the gradients the step actually used
  for tag, opt, lr, p0 in (('g', gan.g_optimizer, 1e-4, gp), ('d', gan.d_optimizer, 4e-4, dp)):
    names = list(captured[tag])
    for k in names[:4] + names[-4:]:
      g = torch.from_numpy(captured[tag][k])
      newp, _, _ = O.adam_keras(p0[k], g, torch.zeros_like(g), torch.zeros_like(g), lr, 0.5,
                                0.999, 1)
      assert rel_err(opt.model.store[k].cpu().numpy(), newp.numpy()) < 1e-5, k
  # BN moving stats / spectral u advanced exactly once
  for k, v in ref['g_updates'].items():
    r64 = ref64['g_updates'][k].detach().numpy()
    assert rel_err(gan.generator.store[k].cpu().numpy(), r64) <= \
        ACC_FACTOR * rel_err(v.detach().numpy(), r64) + 1e-3, k
  # EMA generator is a hard copy during the first cluster (gan_manager.py:642-655)
  np.testing.assert_array_equal(gan.ema_generator.store.theta.cpu().numpy(),
                                gan.generator.store.theta.cpu().numpy())
  m = gan._save_metrics_to_dict()
  for key in ('gen/gen_gan_loss', 'dis/disc_loss', 'gen/depth_loss', 'gen/wc_loss', 'gen/gen_loss',
              'gen/grad_norm', 'dis/grad_norm'):
    r = ref64['metrics'][key]
    assert abs(float(m[key]) - r) <= \
        ACC_FACTOR * abs(ref['metrics'][key] - r) + 2e-3 * max(1.0, abs(r)), key
  assert set(m) >= {'gen/gen_feat_loss', 'gen/kld_nan', 'gen/seg_loss'}


@pytest.mark.parametrize('case', ['zero_mask_no_valid_depth', 'fractional_mask'])
def test_train_g_d_edge_cases_n1(case):
  """se3ds_trainer.py:148-166,176-178 at their clamps, batch 1: (a) an all-zero proj_mask (the
  world-consistency normaliser max(sum m, 1) clamps, every PartialConv window is empty) together
  with a depth map that has NO valid pixel (every value exactly 0 or 1: num_spatial_pixels clamps to
  1, the depth loss vanishes); (b) a FRACTIONAL proj_mask (`gan.binary_masks = False`: the exact
  partial-conv kernels).  Metrics and the whole clipped gradient vector against the oracle, judged
  by the fp64 yardstick like the regular toy step."""
  size = 64
  gan = _make_gan(size, 4, '50', 3)
  batch = synth_batch(1, size, seed=91)
  if case == 'zero_mask_no_valid_depth':
    batch['proj_mask'] = torch.zeros_like(batch['proj_mask'])
    batch['depth'] = (batch['depth'] > 0.5).float()
  else:
    g = torch.Generator().manual_seed(5)
    batch['proj_mask'] = torch.rand(batch['proj_mask'].shape, generator=g)
    gan.binary_masks = False
  batch['proj_image'] = batch['image'] * batch['proj_mask']
  batch['proj_depth'] = batch['depth'] * batch['proj_mask']
  gp, dp = _oracle_params(gan.generator), _oracle_params(gan.discriminator)
  cfg = _cfg(4, '50', 3)
  ref = O.train_g_d(gp, dp, batch, cfg)
  with fp64_oracle():
    ref64 = O.train_g_d(_f64(gp), _f64(dp), _f64(batch), cfg)
  views = {tag: capture_clipped_grads(opt)[1]
           for opt, tag in ((gan.g_optimizer, 'g'), (gan.d_optimizer, 'd'))}
  gan.train_g_d({k: v.to(DEV) for k, v in batch.items()})
  torch.cuda.synchronize()
  for tag, key, opt in (('g', 'g_grads', gan.g_optimizer), ('d', 'd_grads', gan.d_optimizer)):
    num_h = num_o = den = 0.0
    for k in ref[key]:
      r64 = ref64[key][k].numpy().ravel()
      a = views[tag](k).numpy().astype(np.float64).ravel()
      b = ref[key][k].numpy().astype(np.float64).ravel()
      assert np.isfinite(a).all(), (tag, k)
      num_h += float(((a - r64) ** 2).sum()); num_o += float(((b - r64) ** 2).sum())
      den += float((r64 ** 2).sum())
    e_hip, e_o32 = (num_h / den) ** 0.5, (num_o / den) ** 0.5
    print(f'{case} {tag}: ||grad - f64|| / ||f64||: hip {e_hip:.3e}, fp32 oracle {e_o32:.3e}')
    assert e_hip <= ACC_FACTOR * e_o32 + 1e-3, (tag, e_hip, e_o32)
  m = gan._save_metrics_to_dict()
  for key in ('gen/gen_gan_loss', 'dis/disc_loss', 'gen/depth_loss', 'gen/wc_loss', 'gen/gen_loss'):
    r = ref64['metrics'][key]
    assert abs(float(m[key]) - r) <= \
        ACC_FACTOR * abs(ref['metrics'][key] - r) + 2e-3 * max(1.0, abs(r)), (key, float(m[key]), r)
  if case == 'zero_mask_no_valid_depth':
    assert float(m['gen/depth_loss']) == 0.0 and float(m['gen/wc_loss']) == 0.0


def test_train_d_only_updates_discriminator():
  size = 64
  gan = _make_gan(size, 4, '50', 3)
  batch = synth_batch(4, size, seed=78)
  gp, dp = _oracle_params(gan.generator), _oracle_params(gan.discriminator)
  cfg = _cfg(4, '50', 3)
  ref = O.train_d(gp, dp, batch, cfg)
  with fp64_oracle():
    ref64 = O.train_d(_f64(gp), _f64(dp), _f64(batch), cfg)
  theta_g = gan.generator.store.theta.clone()
  _, dview = capture_clipped_grads(gan.d_optimizer)
  gan.train_d({k: v.to(DEV) for k, v in batch.items()})
  torch.cuda.synchronize()
  captured = {n: dview(n).numpy().copy() for n in gan.discriminator.store.trainable_names}
  assert torch.equal(theta_g, gan.generator.store.theta)
  assert gan.d_optimizer.iterations == 1 and gan.g_optimizer.iterations == 0
  # G ran in training mode: BN moving statistics / u advanced (se3ds_trainer.py:292-293)
  for k, v in ref['g_updates'].items():
    r64 = ref64['g_updates'][k].detach().numpy()
    assert rel_err(gan.generator.store[k].cpu().numpy(), r64) <= \
        ACC_FACTOR * rel_err(v.detach().numpy(), r64) + 1e-3, k
  for k, g in ref['d_grads'].items():
    r64 = ref64['d_grads'][k].numpy()
    if float(np.abs(r64).max()) < 1e-7:
      continue
    close_to_f64(captured[k], g.numpy(), r64, k)


def test_bf16_step_runs_and_tracks_fp32():
  """bf16 compute path (the throughput configuration): runs, stays finite, and its losses
  track the fp32 path on identical weights."""
  size = 64
  vals = {}
  for dtype in (torch.float32, torch.bfloat16):
    gan = _make_gan(size, 32, '50', 3, dtype)
    batch = synth_batch(2, size, seed=79)
    gan.train_g_d({k: v.to(DEV) for k, v in batch.items()})
    m = gan._save_metrics_to_dict()
    assert all(np.isfinite(float(v)) for v in m.values())
    assert bool(torch.isfinite(gan.generator.store.theta).all())
    vals[dtype] = m
  for key in ('gen/gen_gan_loss', 'dis/disc_loss', 'gen/depth_loss', 'gen/wc_loss'):
    a, b = float(vals[torch.float32][key]), float(vals[torch.bfloat16][key])
    assert abs(a - b) <= 5e-2 * max(1.0, abs(a)), (key, a, b)


def test_segment_grad_sync_matches_serial_path(monkeypatch):
  """The overlapped path (per-module spectral fix-up -> per-tensor clip -> side-stream
  all-reduce launched from inside the backward pass) must leave exactly the weights, Adam
  slots and grad-norm metrics of the serial path."""
  size = 64
  batch = {k: v.to(DEV) for k, v in synth_batch(4, size, seed=81).items()}
  res = {}
  for mode in ('serial', 'overlap'):
    if mode == 'overlap':
      monkeypatch.setenv('SE3DS_FORCE_GRAD_SYNC', '1')
    gan = _make_gan(size, 8, '50', 3)
    gan.train_g_d(batch)
    gan.global_step += 1
    gan.train_d(batch)
    gan.train_g_d(batch)
    torch.cuda.synchronize()
    if mode == 'overlap':
      segs = gan._g_segments
      assert set(segs) == set(gan.generator.SEGMENTS)
      assert sorted(v[2] for v in segs.values())[0] == 0
    m = gan._save_metrics_to_dict()
    res[mode] = (gan.generator.store.theta.clone(), gan.discriminator.store.theta.clone(),
                 gan.g_optimizer.v.clone(), gan.d_optimizer.m.clone(),
                 float(m['gen/grad_norm']), float(m['dis/grad_norm']))
  for a, b in zip(res['serial'][:4], res['overlap'][:4]):
    assert torch.equal(a, b)
  assert res['serial'][4] == pytest.approx(res['overlap'][4], rel=1e-6)
  assert res['serial'][5] == pytest.approx(res['overlap'][5], rel=1e-6)


@pytest.mark.parametrize('cin,cout,n,h,w,conv_act,k,stride,big', [
    (64, 128, 2, 16, 32, 0, 3, 1, None), (128, 256, 3, 11, 70, 0, 3, 1, None),
    (64, 128, 2, 16, 32, 2, 3, 1, None),          # activation fused into the conv
    (64, 256, 2, 16, 40, 0, 1, 1, '1'),           # 1x1 on the 256-pixel macro tile (ragged last tile)
    (128, 256, 3, 9, 30, 0, 1, 1, '0'),           # 1x1 on the 128 x 128 tile
    (64, 128, 2, 17, 33, 1, 3, 2, '0'),           # strided 3x3, relu fused
])
def test_fused_bn_statistics_match_separate_pass(cin, cout, n, h, w, conv_act, k, stride, big,
                                                 monkeypatch):
  """conv -> SyncBatchNormalization: the column sums emitted by the conv epilogue must give the
  same normalised output / moving statistics as the separate statistics pass."""
  if big is not None:
    monkeypatch.setenv('SE3DS_BIG_TILE', big)
  res = {}
  for mode in ('0', '2'):
    monkeypatch.setenv('SE3DS_FUSED_BN_STATS', mode)
    store = nn.ParamStore()
    conv = nn.ConvLayer(store, 'c', cin, cout, k, stride, 'VALID', True, 'plain')
    bn = nn.NormLayer(store, 'n', cout, 'batch')
    store.finalize(DEV, torch.Generator().manual_seed(3))
    ctx = nn.Ctx(DEV, torch.bfloat16, training=True, record=True)
    x = nn.Var(torch.randn((n, h, w, cin), generator=torch.Generator().manual_seed(4)).to(DEV).bfloat16())
    y = nn.conv2d(ctx, x, conv, pad=k // 2, act=conv_act, alpha=0.3)
    assert (y.col_stats is not None) == (mode == '2')
    z = nn.norm_act(ctx, y, bn, act=2, alpha=0.2)
    z.grad = torch.ones_like(z.data)
    ctx.backward()
    res[mode] = (z.data.float().cpu().numpy(), store['n/moving_mean'].cpu().numpy().copy(),
                 store['n/moving_variance'].cpu().numpy().copy(), x.grad.float().cpu().numpy())
  # fp32 statistics agree to summation-order noise; bf16 tensors to a rounding step
  assert rel_err(res['0'][1], res['2'][1]) < 1e-4 and rel_err(res['0'][2], res['2'][2]) < 1e-4
  assert rel_err(res['0'][0], res['2'][0]) < tol(torch.bfloat16)
  assert rel_err(res['0'][3], res['2'][3]) < tol(torch.bfloat16)


def test_checkpoint_resume_is_bit_exact(tmp_path):
  """save -> restore into a fresh trainer -> the next step lands on identical weights, Adam slots,
  EMA copy and BN / spectral state; SE3DSModel accepts the same file for the EMA generator."""
  size = 64
  batch = {k: v.to(DEV) for k, v in synth_batch(2, size, seed=83).items()}
  a = _make_gan(size, 8, '50', 3)
  a.train_g_d(batch)
  a.global_step += 1
  a.train_g_d(batch)
  a.global_step += 1
  path = str(tmp_path / 'ckpt.npz')
  a.save_checkpoint(path)
  a.train_g_d(batch)
  b = _make_gan(size, 8, '50', 3)
  assert b.restore_checkpoint(path) == []
  assert b.global_step == 2 and b.g_optimizer.iterations == 2
  b.train_g_d(batch)
  for x, y in ((a.generator.store.theta, b.generator.store.theta),
               (a.generator.store.state, b.generator.store.state),
               (a.discriminator.store.theta, b.discriminator.store.theta),
               (a.ema_generator.store.theta, b.ema_generator.store.theta),
               (a.g_optimizer.m, b.g_optimizer.m), (a.d_optimizer.v, b.d_optimizer.v)):
    assert torch.equal(x, y)
  with pytest.raises(KeyError):
    c = _make_gan(size, 8, '50', 3)
    c.load_state_dict({'global_step': np.asarray(0)})
  # inference wrapper: restores the EMA generator from the same file
  from se3ds_amd.models import model_config, models
  cfg = model_config.get_test_config()
  cfg.ckpt_path, cfg.image_height, cfg.gen_dims, cfg.resnet_version = path, size, 8, '50'
  m = models.SE3DSModel(cfg, device=DEV, dtype=torch.float32)
  with np.load(path) as f:
    k = next(k for k in f.files if k.startswith('ema_generator/') and k.endswith('/kernel'))
    np.testing.assert_array_equal(m.model.store[k[len('ema_generator/'):]].cpu().numpy(), f[k])
  # the reference's own format: a tf.train.Checkpoint(ema_generator=...) bundle prefix
  from se3ds_amd.utils import tf_bundle
  prefix = path[:-4] + '_tf/ckpt-1'
  os.makedirs(os.path.dirname(prefix), exist_ok=True)
  tf_bundle.save_generator(m.model, prefix)
  cfg.ckpt_path = prefix
  m2 = models.SE3DSModel(cfg, device=DEV, dtype=torch.float32)
  assert torch.equal(m2.model.store.theta, m.model.store.theta)
  cfg.ckpt_path = '/nonexistent/model.ckpt-1'
  with pytest.raises(FileNotFoundError):
    models.SE3DSModel(cfg, device=DEV, dtype=torch.float32)


def test_split_input_dict_and_cluster():
  gan = _make_gan(64, 4, '50', 3)
  gan.d_step_per_g_step = 2
  batch = {k: v.to(DEV) for k, v in synth_batch(4, 64, seed=80).items()}
  parts = gan._split_input_dict(batch, 2)
  assert len(parts) == 2 and parts[0]['image'].shape[0] == 2
  assert torch.equal(parts[1]['depth'], batch['depth'][2:])
  gan.train_ds = iter([batch])
  gan.train_cluster(1)
  assert gan.d_optimizer.iterations == 2 and gan.g_optimizer.iterations == 1


def test_se3ds_model_roundtrip_and_shapes():
  """models/models_test.py:38-79: add a pano to the memory, predict at the same position ->
  projected RGB equals the input on >= 95 % of the pixels; shapes and ranges."""
  from se3ds_amd.models import model_config, models
  gin_lite.clear_config()
  size = 128
  g = torch.Generator().manual_seed(3)
  rgb = torch.randint(0, 255, (1, size, size * 2, 3), generator=g, dtype=torch.int32).to(torch.uint8)
  seg = torch.randint(0, 42, (1, size, size * 2, 1), generator=g, dtype=torch.int32).to(torch.uint8)
  depth = torch.rand((1, size, size * 2), generator=g)
  pos = torch.randn((1, 3), generator=g)
  config = model_config.get_test_config()
  config.image_height = size
  model = models.SE3DSModel(config, device=DEV)
  model.add_to_memory(rgb.to(DEV), seg.to(DEV), depth.to(DEV), pos.to(DEV), mask_blurred=False)
  out = model(pos.to(DEV))
  eq = torch.all(out.proj_rgb.cpu() == rgb, dim=-1).float().mean()
  assert float(eq) >= 0.95
  assert tuple(out.proj_semantic.shape) == (1, size, size * 2)
  assert tuple(out.pred_semantic.shape) == (1, size, size * 2)
  assert tuple(out.pred_rgb.shape) == tuple(rgb.shape) and out.pred_rgb.dtype == torch.uint8
  assert tuple(out.pred_depth.shape) == (1, size, size * 2)
  assert float(out.pred_depth.min()) >= 0 and float(out.pred_depth.max()) <= 1
  # feedback path: predictions become part of the memory
  m0 = model.get_memory_state().rgb.shape[1]
  model(pos.to(DEV) + 0.1, add_preds_to_memory=True)
  assert model.get_memory_state().rgb.shape[1] > m0
  config.batch_size = 2
  with pytest.raises(ValueError):
    models.SE3DSModel(config, device=DEV)


@pytest.mark.parametrize('cin', [32, 64])
def test_partial_conv_fractional_mask_exact_path(cin):
  """Fractional (non-binary) masks take the exact register-staged kernels (Ctx.binary_masks =
  False): x * mask in the gather, dy * ratio * update_mask in the transposed gather."""
  store, layer, sg = _mk_layer('partial', cin, 32, 3, 1, 'VALID', True, 9)
  gen = torch.Generator().manual_seed(13)
  n, h, w = 2, 12, 20
  x = torch.randn((n, h, w, cin), generator=gen)
  mask = torch.rand((n, h, w, 1), generator=gen)
  mask[:, 3:6] = 0
  p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in store.views.items()}
  xo = x.clone().requires_grad_(True)
  net = O.Net(p, training=True)
  yo, umo = net.partial_conv(O.pad_layer(xo, 1), O.pad_layer(mask, 1), 'c', 1, 'VALID')
  gy = torch.randn(yo.shape, generator=gen)
  yo.backward(gy)
  ctx = nn.Ctx(DEV, torch.float32, training=True, record=True)
  ctx.binary_masks = False
  xv = nn.Var(to_dev(x.numpy(), torch.float32))
  yv, um = nn.conv2d(ctx, xv, layer, pad=1, mask=to_dev(mask.numpy()[..., 0], torch.float32))
  assert rel_err(um.cpu().numpy(), umo.detach().numpy()[..., 0]) < 1e-6
  assert rel_err(yv.data.cpu().numpy(), yo.detach().numpy()) < 1e-4
  yv.grad = to_dev(gy.numpy(), torch.float32)
  ctx.backward()
  assert rel_err(xv.grad.cpu().numpy(), xo.grad.numpy()) < 1e-4
  assert rel_err(store.grad_views['c/kernel'].cpu().numpy(), p['c/kernel'].grad.numpy()) < 1e-4
  assert rel_err(store.grad_views['c/bias'].cpu().numpy(), p['c/bias'].grad.numpy()) < 1e-3
  # SE3DS_CHECK_MASKS (attr nn._CHECK_MASKS, debugging): a fractional mask that reaches a binary-mask
  # fast path -- Ctx.binary_masks left at its default -- is refused instead of silently mis-weighted
  old = nn._CHECK_MASKS
  nn._CHECK_MASKS = True
  try:
    ctx2 = nn.Ctx(DEV, torch.float32, training=True, record=False)
    with pytest.raises(_lib.Se3dsHipError):
      nn.conv2d(ctx2, nn.Var(to_dev(x.numpy(), torch.float32)), layer, pad=1,
                mask=to_dev(mask.numpy()[..., 0], torch.float32))
    ctx2.binary_masks = False   # (declared fractional: the exact path, no complaint)
    nn.conv2d(ctx2, nn.Var(to_dev(x.numpy(), torch.float32)), layer, pad=1,
              mask=to_dev(mask.numpy()[..., 0], torch.float32))
    ctx3 = nn.Ctx(DEV, torch.float32, training=True, record=False)
    nn.conv2d(ctx3, nn.Var(to_dev(x.numpy(), torch.float32)), layer, pad=1,
              mask=to_dev((mask.numpy()[..., 0] > 0.5).astype(np.float32), torch.float32))
  finally:
    nn._CHECK_MASKS = old


def test_fused_adam_ema_is_bit_identical(monkeypatch):
  """The generator's EMA advanced inside the Adam pass (se3ds_multi_adam_keras_ema) leaves exactly
  the EMA copy that the separate se3ds_multi_ema pass produces."""
  size = 64
  batch = {k: v.to(DEV) for k, v in synth_batch(2, size, seed=91).items()}
  res = {}
  for mode in ('0', '1'):
    monkeypatch.setenv('SE3DS_UNFUSED_EMA', mode)
    gan = _make_gan(size, 8, '50', 3)
    for _ in range(3):   # step 0 copies, steps 1 and 2 average
      gan.train_g_d(batch)
      gan.global_step += 1
    res[mode] = (gan.ema_generator.store.theta.clone(), gan.ema_generator.store.state.clone(),
                 gan.generator.store.theta.clone())
  for a, b in zip(res['0'], res['1']):
    assert torch.equal(a, b)
  assert not torch.equal(res['0'][0], res['0'][2])   # the average lags the weights


@pytest.mark.parametrize('num_batched_steps,steps', [(1, 3), (2, 5)])
def test_adam_and_ema_recurrences_vs_oracle(num_batched_steps, steps):
  """Keras Adam with non-zero slots (t = 1..steps, bias-corrected step size) and the EMA
  copy-phase -> decay-phase switch (gan_manager.py:642-655: the copy lasts the whole first
  cluster because global_step only advances per cluster) over ALL variables -- parameters, BN
  moving statistics, spectral u -- against the oracle's recurrences (O.adam_keras, O.ema_step),
  driven by the gradients each HIP step actually produced.  One fp32 ulp per step."""
  size = 64
  gan = _make_gan(size, 8, '50', 3)
  gan.num_batched_steps = num_batched_steps
  G, D = gan.generator, gan.discriminator
  cpu = lambda model: {k: v.detach().cpu().clone() for k, v in model.store.views.items()}
  p = {'g': cpu(G), 'd': cpu(D)}
  ema = cpu(gan.ema_generator)
  slots = {t: {k: (torch.zeros_like(p[t][k]), torch.zeros_like(p[t][k]))
               for k in m.store.trainable_names} for t, m in (('g', G), ('d', D))}
  gviews = {tag: capture_clipped_grads(opt)[1]
            for opt, tag in ((gan.g_optimizer, 'g'), (gan.d_optimizer, 'd'))}
  class _Views:        # cap[tag][name]: the gradient Adam consumed in the LAST step
    def __init__(self, view):
      self.view = view
    def __getitem__(self, name):
      return self.view(name).clone()
  cap = {tag: _Views(v) for tag, v in gviews.items()}
  # parameters: 3e-5 of the step size (the update's own fp32 noise: fused vs separate multiply-
  # add in the slot recurrences) + 2.5 ulp; slots / averages: 1e-5 of the tensor's scale
  close_p = lambda a, b, lr: torch.allclose(a, b, rtol=3e-7, atol=3e-5 * lr)
  close = lambda a, b: torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()) + 1e-30)
  for step in range(steps):
    batch = {k: v.to(DEV) for k, v in synth_batch(2, size, seed=200 + step).items()}
    gs = gan.global_step
    gan.train_g_d(batch)
    if (step + 1) % num_batched_steps == 0:   # host loop, gan_manager.py:409-421
      gan.global_step += num_batched_steps
    for tag, model, opt, lr in (('g', G, gan.g_optimizer, 1e-4), ('d', D, gan.d_optimizer, 4e-4)):
      assert opt.iterations == step + 1
      for k in model.store.trainable_names:
        m0, v0 = slots[tag][k]
        newp, m1, v1 = O.adam_keras(p[tag][k], cap[tag][k], m0, v0, lr, 0.5, 0.999, step + 1)
        o, cnt, shape = model.store._off_tr[k]
        assert close_p(model.store[k].cpu(), newp, lr), (step, tag, k)
        assert close(opt.m[o:o + cnt].view(shape).cpu(), m1), (step, tag, k, 'm')
        assert close(opt.v[o:o + cnt].view(shape).cpu(), v1), (step, tag, k, 'v')
        p[tag][k], slots[tag][k] = newp, (m1, v1)
    new_vals = cpu(G)   # BN moving statistics / u as the step left them
    ema = O.ema_step(ema, new_vals, gs, gan.ema_decay, gan.ema_init_step, num_batched_steps)
    for k, v in ema.items():
      assert close(gan.ema_generator.store[k].cpu(), v), (step, k)
    if gs >= num_batched_steps:   # decay phase: the average lags the weights
      assert not torch.equal(gan.ema_generator.store.theta, G.store.theta)


def test_fused_spectral_fixup_clip_matches_separate_passes():
  """The generator's spectral fix-up folded into the clip pass (se3ds_spectral_bwd_dots +
  se3ds_multi_sqnorm_sn + se3ds_multi_clip_by_norm_sn) against the separate passes
  (se3ds_spectral_bwd_fixup, then sqnorm + clip) on the same gradient arena: whole arena and
  per-segment, clip both active (large gradients) and inactive (small)."""
  gan = _make_gan(64, 8, '50', 3)
  G, opt = gan.generator, gan.g_optimizer
  st = G.store
  st.grad_views   # allocates the arena
  ctx = G.make_ctx(True, record=False)
  G.spectral.power_iteration(training=True)   # sigma, v_hat, u_hat of every layer
  gen = torch.Generator(device=DEV).manual_seed(5)
  for scale in (10.0, 1e-3):
    g0 = torch.randn(st.grad.shape, generator=gen, device=DEV) * scale
    # One spectral gradient dominated by its v u^T component: the fixed gradient is then a small
    # difference of large terms -- in the separate passes element by element, in the fused pass in
    # the closed-form norm.  Both carry the fp32 rounding of coef = <G,W>/(sigma+eps)^2 amplified
    # by |G/sigma|^2 / |fixed|^2 (~1e3 here), so this tensor's norm is compared at 1e-3.
    name = next(n_ for n_ in st.trainable_names if n_.endswith('/kernel') and 'deconv' in n_)
    lay = next(l for l in G.spectral.layers if l.name + '/kernel' == name)
    t_adv = st.trainable_names.index(name)
    o, n_, shape = st._off_tr[name]
    outer = (lay.sn['v'][:, None] * lay.sn['uhat'][None, :]).reshape(-1)
    g0[o:o + n_] = outer * (30.0 * scale * float(n_) ** 0.5) + g0[o:o + n_]
    st.grad.copy_(g0)
    G.spectral.backward_fixup()
    norm_a = opt.clip_gradients(5.0).clone()
    ref, sq_ref = st.grad.clone(), opt.sqnorm.clone()
    st.grad.copy_(g0)
    G.spectral.backward_fixup(dots_only=True)
    norm_b = opt.clip_gradients(5.0, fused_sn=True).clone()
    got, sq = st.grad.clone(), opt.sqnorm.clone()
    tol = 1e-5 * float(ref.abs().max())   # (the dominated tensor: rounding of coef, see above)
    assert float((got - ref).abs().max()) <= tol, (scale, float((got - ref).abs().max()), tol)
    rel = ((sq - sq_ref).abs() / sq_ref.clamp_min(1e-30)).cpu()
    assert float(rel[t_adv]) < 1e-3, (scale, float(rel[t_adv]))
    rel[t_adv] = 0
    assert float(rel.max()) < 5e-5, (scale, float(rel.max()), int(rel.argmax()))
    assert abs(float(norm_a) - float(norm_b)) <= 1e-5 * abs(float(norm_a))
    # per-segment form
    st.grad.copy_(g0)
    segments = st.segments(G.SEGMENTS)
    assert sum(t1 - t0 for t0, t1, _, _ in segments.values()) == len(st.trainable_names)
    for seg, (t0, t1, e0, e1) in segments.items():
      G.spectral.backward_fixup(prefix=G.SEGMENTS[seg], dots_only=True)
      opt.clip_segment(t0, t1, 5.0, fused_sn=True)
    assert float((st.grad - ref).abs().max()) <= tol, ('segments', scale)
    rel = ((opt.sqnorm - sq_ref).abs() / sq_ref.clamp_min(1e-30)).cpu()
    rel[t_adv] = 0
    assert float(rel.max()) < 5e-5, ('segments', scale, float(rel.max()))


def test_fused_clip_adam_is_bit_identical_to_separate_passes():
  """Round 4: per-tensor clip (+ spectral fix-up) applied inside the Adam + EMA pass
  (se3ds_multi_clip_adam_keras_ema, AdamState.clip_apply) against clip_segment + apply_segment on
  the same gradients: theta, m, v and the EMA arena must agree BIT FOR BIT (same per-element
  arithmetic; the fused pass never rewrites the gradient arena), over several steps, with the
  clip both active and inactive, per segment and over the whole arena."""
  gan = _make_gan(64, 8, '50', 3)
  G, opt = gan.generator, gan.g_optimizer
  st = G.store
  st.grad_views
  G.spectral.power_iteration(training=True)
  ema = gan.ema_generator.store.theta
  segments = st.segments(G.SEGMENTS)
  nt = len(st.trainable_names)
  gen = torch.Generator(device=DEV).manual_seed(11)
  snap = lambda: (st.theta.clone(), opt.m.clone(), opt.v.clone(), ema.clone())
  theta0, m0, v0, ema0 = snap()
  it0 = opt.iterations
  def restore():
    st.theta.copy_(theta0); opt.m.copy_(m0); opt.v.copy_(v0); ema.copy_(ema0)
    opt.iterations = it0
  # (random gradients on the TENSORS only: the 16-byte alignment gaps between them carry zero
  # gradients in a real step; a whole-arena Adam pass would update them, a per-chunk pass skips them)
  live = torch.zeros(st.grad.shape, device=DEV)
  for name in st.trainable_names:
    o, n_, _ = st._off_tr[name]
    live[o:o + n_] = 1.0
  grads = [torch.randn(st.grad.shape, generator=gen, device=DEV) * sc * live for sc in (10.0, 1e-3, 1.0)]
  def run(fused, per_segment, with_ema):
    restore()
    for g0 in grads:
      st.grad.copy_(g0)
      opt.begin_step()
      todo = list(segments.items()) if per_segment else [('all', (0, nt, 0, st.theta.numel()))]
      for seg, (t0, t1, e0, e1) in todo:
        G.spectral.backward_fixup(prefix=G.SEGMENTS[seg] if per_segment else None, dots_only=True)
        et, omd = (ema, 1e-3) if with_ema else (None, 0.0)
        if fused:
          assert opt.clip_apply(t0, t1, 5.0, True, et, omd)
        else:
          opt.clip_segment(t0, t1, 5.0, fused_sn=True)
          opt.apply_segment(e0, e1, et, omd)
      opt.end_step()
      if fused:   # the fused pass leaves the gradient arena untouched
        assert torch.equal(st.grad, g0)
    return snap()
  for per_segment in (True, False):
    for with_ema in (True, False):
      ref = run(False, per_segment, with_ema)
      got = run(True, per_segment, with_ema)
      for name, a, b in zip(('theta', 'm', 'v', 'ema'), ref, got):
        assert torch.equal(a, b), (per_segment, with_ema, name, float((a - b).abs().max()))
      assert not torch.equal(ref[0], theta0)
  restore()


def test_grad_sync_drip_feeds_buckets():
  """GradSync on the shared communicator: a slice is cut into buckets, the first goes to the side
  stream at once, one more per pump() (wired behind every SyncBN collective), the rest at
  finish(); without drip everything is issued by reduce_range."""
  from se3ds_amd.trainers import dist_utils
  arena = torch.randn(10 * 1024 + 3, device=DEV)
  ref = arena.clone()
  sync = dist_utils.GradSync(DEV, None, bucket_elems=1024, drip=True)
  sync.reduce_range(arena, 5, arena.numel())
  n_buckets = -(-(arena.numel() - 5) // 1024)
  assert len(sync.pending) == n_buckets - 1
  sync.pump()
  sync.pump(2)
  assert len(sync.pending) == n_buckets - 4
  sync.reduce_range(arena, 0, 5)          # a later slice queues behind the pending buckets
  assert len(sync.pending) == n_buckets - 4   # (one bucket issued, the new one appended)
  sync.finish()
  assert not sync.pending and not sync.launched
  torch.cuda.synchronize()
  assert torch.equal(arena, ref)          # world size 1: the collective is skipped
  # second step: the first step saw 1 collective-paced pump() call, so the pacing now empties the
  # queue by that call instead of leaving it to finish()
  assert sync.prev_seen == 1
  sync.reduce_range(arena, 0, arena.numel())
  assert len(sync.pending) == -(-arena.numel() // 1024) - 1
  sync.pump()
  assert not sync.pending
  sync.finish()
  sync = dist_utils.GradSync(DEV, None, bucket_elems=1024, drip=False)
  sync.reduce_range(arena, 0, arena.numel())
  assert not sync.pending
  sync.finish()
  assert dist_utils.GradSync(DEV, None).bucket == dist_utils.DRIP_BUCKET_ELEMS
  assert dist_utils.GradSync(DEV, None, drip=False).bucket == dist_utils.GRAD_BUCKET_ELEMS


def test_maxpool_backward_ties_go_to_first_maximum_bf16():
  """TF MaxPoolGrad routes the gradient to the FIRST maximal element of a window (row-major);
  the vectorised bf16 kernel on windows that are all ties, partly ties, and ragged (odd H, W)."""
  gen = torch.Generator().manual_seed(3)
  for (h, w) in ((6, 8), (7, 9)):
    x = torch.randint(0, 2, (2, h, w, 16), generator=gen).float()   # values {0, 1}: ties everywhere
    ctx = nn.Ctx(DEV, torch.bfloat16, training=True, record=True)
    xv = nn.Var(x.to(DEV).bfloat16())
    yv = nn.maxpool2x2(ctx, xv)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    gy = torch.randn((2, ho, wo, 16), generator=gen).bfloat16().float()
    yv.grad = gy.to(DEV).bfloat16()
    ctx.backward()
    want = torch.zeros_like(x)
    for oy in range(ho):
      for ox in range(wo):
        win = [(2 * oy + a, 2 * ox + b) for a in (0, 1) for b in (0, 1) if 2 * oy + a < h and 2 * ox + b < w]
        m = torch.stack([x[:, qy, qx] for qy, qx in win]).max(0).values
        taken = torch.zeros_like(m, dtype=torch.bool)
        for qy, qx in win:
          hit = (x[:, qy, qx] == m) & ~taken
          want[:, qy, qx] = torch.where(hit, gy[:, oy, ox], torch.zeros_like(m))
          taken |= hit
    np.testing.assert_array_equal(xv.grad.float().cpu().numpy(), want.numpy())


def test_colsum_row_scale_matches_the_two_separate_passes():
  """se3ds_colsum_row_scale (one read of dy) vs se3ds_row_scale + se3ds_norm_stats: the scaled copy
  and the row-weighted column sums must be bit-identical (same arithmetic, same order)."""
  from se3ds_amd import _lib
  L = _lib.lib()
  gen = torch.Generator().manual_seed(11)
  for rows, c in ((1000, 64), (4096, 256), (37, 8)):
    dy = torch.randn((rows, c), generator=gen).bfloat16().to(DEV)
    ru = torch.rand(rows, generator=gen).to(DEV)
    bu = (torch.rand(rows, generator=gen) > 0.2).float().to(DEV)
    wsz = L.se3ds_norm_workspace_bytes(1, c)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    ref_s = torch.empty_like(dy)
    _lib.check(L.se3ds_row_scale(dy.data_ptr(), _lib.BF16, rows, c, ru.data_ptr(), ref_s.data_ptr(),
                                 _lib.stream()), 'se3ds_row_scale')
    sums = torch.empty((1, 2, c), dtype=torch.float32, device=DEV)
    ref_b = torch.empty(c, dtype=torch.float32, device=DEV)
    _lib.check(L.se3ds_norm_stats(dy.data_ptr(), _lib.BF16, 1, rows, c, bu.data_ptr(), sums.data_ptr(),
                                  ref_b.data_ptr(), ws.data_ptr(), wsz, _lib.stream()), 'se3ds_norm_stats')
    got_s = torch.empty_like(dy)
    got_b = torch.empty(c, dtype=torch.float32, device=DEV)
    _lib.check(L.se3ds_colsum_row_scale(dy.data_ptr(), _lib.BF16, rows, c, bu.data_ptr(), ru.data_ptr(),
                                        got_s.data_ptr(), sums.data_ptr(), got_b.data_ptr(),
                                        ws.data_ptr(), wsz, _lib.stream()), 'se3ds_colsum_row_scale')
    torch.cuda.synchronize()
    assert torch.equal(got_s.view(torch.int16), ref_s.view(torch.int16)), (rows, c)
    assert torch.equal(got_b, ref_b), (rows, c)
    want = (dy.float() * bu[:, None]).double().sum(0)
    assert float((got_b.double() - want).abs().max()) <= 1e-3 * float(want.abs().max() + 1)
  # unsupported layouts are refused (callers fall back to the two passes)
  x = torch.zeros((8, 4), device=DEV)
  assert L.se3ds_colsum_row_scale(x.data_ptr(), _lib.F32, 8, 4, None, None, x.data_ptr(), None, None,
                                  None, 0, _lib.stream()) != 0


def test_norm_reduce_rows_finalize_matches_the_pair():
  """se3ds_norm_reduce_rows_finalize vs se3ds_norm_reduce_rows + se3ds_norm_finalize: scale, shift,
  mean, rstd and the moving statistics are bit-identical."""
  from se3ds_amd import _lib
  L = _lib.lib()
  gen = torch.Generator().manual_seed(12)
  for rows, c in ((256, 1024), (17, 64), (2048, 128)):
    part = (torch.randn((rows, 2, c), generator=gen) * 3).to(DEV)
    part[:, 1] = part[:, 1].abs() * 4 + 10          # sums of squares
    gamma = (torch.rand(c, generator=gen) + 0.5).to(DEV)
    beta = torch.randn(c, generator=gen).to(DEV)
    count = float(rows * 64)
    outs = []
    for fused in (False, True):
      mm, mv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
      o = [torch.empty((1, c), device=DEV) for _ in range(4)]
      if fused:
        _lib.check(L.se3ds_norm_reduce_rows_finalize(
            part.data_ptr(), rows, c, count, gamma.data_ptr(), beta.data_ptr(), 1e-3, 0.99,
            mm.data_ptr(), mv.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
            o[3].data_ptr(), _lib.stream()), 'se3ds_norm_reduce_rows_finalize')
      else:
        sums = torch.empty((1, 2, c), device=DEV)
        wsz = L.se3ds_norm_workspace_bytes(max(1, (rows + 511) // 512), c)
        ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
        _lib.check(L.se3ds_norm_reduce_rows(part.data_ptr(), rows, c, sums.data_ptr(), ws.data_ptr(),
                                            wsz, _lib.stream()), 'se3ds_norm_reduce_rows')
        _lib.check(L.se3ds_norm_finalize(sums.data_ptr(), count, 1, c, gamma.data_ptr(),
                                         beta.data_ptr(), 1e-3, 0.99, mm.data_ptr(), mv.data_ptr(), 0,
                                         o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                         o[3].data_ptr(), _lib.stream()), 'se3ds_norm_finalize')
      torch.cuda.synchronize()
      outs.append([t.clone() for t in o] + [mm, mv])
    for a, b in zip(*outs):
      assert torch.equal(a, b), (rows, c)


def test_scheduling_switches_are_bit_identical():
  """One replica: the decoders' two HIP streams (Ctx.branch) and the per-module optimiser on its
  side stream (GAN.train_g_d) only reorder independent work, so every combination of the switches
  must leave the SAME losses and the same parameter / EMA / state checksums as the serial order,
  bit for bit, step after step (tools/step_compare.py; this is the test that found the gradient
  arena being zero-filled on a branch stream).  Six runs: the serial order with the round-3 passes
  (the reference row) and with the round-4 passes, each switch alone, both together, and both
  together with the round-3 passes.  Small widths keep it to a few seconds per run; the full-size
  comparison is `python tools/step_compare.py 512 8 14`."""
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = dict(os.environ, PYTHONPATH=root,
             SE3DS_CMP_GIN='image_models.ResNetGenerator.gen_dims = 16;'
                           'image_models.ResNetGenerator.resnet_version = "50";'
                           'image_models.SNMultiScaleDiscriminator.dis_dims = 16')
  r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'step_compare.py'), '128', '2', '4'],
                     env=env, cwd=root, capture_output=True, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
  assert r.stdout.count('IDENTICAL to serial') == 6, r.stdout[-2000:]


def test_default_schedule_is_bit_identical_to_serial_at_production_size():
  """The same at the bench's own dimensions (highres.gin, 512x1024, batch 8, ResNet-101 at width
  128): three steps of the default schedule -- two decoder streams, per-module optimiser on the
  side stream -- against the serial order, losses and G / D / EMA / state checksums bit for bit."""
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = dict(os.environ, PYTHONPATH=root, SE3DS_CMP_CONFIGS='0:0:old,1:1:')
  env.pop('SE3DS_CMP_GIN', None)
  r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'step_compare.py'), '512', '8', '3'],
                     env=env, cwd=root, capture_output=True, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
  assert r.stdout.count('IDENTICAL to serial') == 2, r.stdout[-2000:]


def test_bf16_conversion_is_round_to_nearest_even():
  """fp32 -> bf16 goes through gfx950's v_cvt_pk_bf16_f32 (csrc/common.h pack2_bf16; the integer
  formulation it replaced made the conv epilogues VALU-bound): bit-identical to round-to-nearest-
  even on ties, denormals, infinities and a million random values; NaN stays NaN."""
  g = torch.Generator().manual_seed(1)
  one = torch.tensor([1.0]).view(torch.int32)
  ties = (one + torch.tensor([0x8000, 0x18000, 0x7fff, 0x8001, 0x17fff, 0x18001], dtype=torch.int32)).view(torch.float32)
  special = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.38e38, -3.38e38, 3.4028235e38, float('inf'), -float('inf'),
                          1e-40, -1e-40, 1.1754944e-38, 1.1754942e-38, 9.2e-41, 65504.0, 1e-45])
  rnd = torch.randn(1 << 20, generator=g) * torch.exp(torch.randn(1 << 20, generator=g) * 8)
  bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 18,), generator=g, dtype=torch.int32).view(torch.float32)
  x = torch.cat([ties, -ties, special, rnd, bits, torch.tensor([float('nan')])])
  x = torch.cat([x, torch.zeros((-x.numel()) % 8)]).reshape(1, 1, -1, 8)
  ctx = nn.Ctx(DEV, torch.bfloat16)
  got = nn.to_var(ctx, x.to(DEV)).data.cpu()
  want = x.to(torch.bfloat16)
  nan = torch.isnan(x)
  assert bool(torch.isnan(got.float())[nan].all())
  a, b = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
  bad = (a != b).nonzero()
  assert bad.numel() == 0, (bad.numel(), x[~nan][bad[:5, 0]], a[bad[:5, 0]], b[bad[:5, 0]])
