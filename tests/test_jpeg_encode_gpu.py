"""The device JPEG encoder (csrc/jpeg_encode.hip, utils/jpeg.encode_jpeg_batch) against the NumPy
oracle of tests/_jpeg_encode_ref.py and against the files Pillow wrote into
tests/golden/jpeg_encode_fixtures.npz (tools/make_jpeg_encode_golden.py), byte for byte.  Sizes that
matter to the kernels (pack unit, scan group) come from the constants the library reports."""
import os

import numpy as np
import pytest
import torch

import _jpeg_encode_ref as E
import _jpeg_ref as J
from se3ds_amd import _lib
from se3ds_amd.inference import perturbation_utils
from se3ds_amd.utils import jpeg, logger as logger_lib, tf_events

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSAMPLINGS = ['4:4:4', '4:2:2', '4:2:0']


@pytest.fixture(scope='module')
def dev():
  return torch.device('cuda', torch.cuda.current_device())


@pytest.fixture(scope='module')
def consts():
  L = _lib.lib()
  return L.se3ds_jpeg_encode_pack_unit_blocks(), L.se3ds_jpeg_encode_scan_group_blocks()


@pytest.fixture(scope='module')
def golden():
  """[(pixels, quality, subsampling, restart, Pillow's file, the oracle's file)]: the oracle runs once."""
  z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_encode_fixtures.npz'))
  out = []
  for i, (h, w, c, q, s, r) in enumerate(z['params'].tolist()):
    px, restart = z[f'pixels_{h}x{w}x{c}'], 'row' if r == -1 else r
    out.append((px, q, SUBSAMPLINGS[s], restart, z[f'file_{i}'].tobytes(), E.encode(px, q, SUBSAMPLINGS[s], restart)))
  return out


def _same(got: bytes, want: bytes, what):
  if got != want:
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    raise AssertionError(f'{what}: {len(got)} bytes, expected {len(want)}; first difference at {first}')


def _encode(px, dev, **kw):
  (got,) = jpeg.encode_jpeg_batch([torch.from_numpy(np.ascontiguousarray(px)).to(dev)], **kw)
  return got


def test_geometry_sweep_single_calls(dev, golden):
  """Ten sizes x grey, 4:4:4, 4:2:2, 4:2:0 x quality 1, 50, 75, 100; 40 x 40, 20 x 9 and 8 x 17 at 4:2:0
  have dummy blocks, 8 x 17 at 4:2:0 the even-height chroma edge."""
  sweep = [g for g in golden if g[3] == 0]
  assert len(sweep) == 160
  for px, q, sub, restart, pillow, oracle in sweep:
    got = _encode(px, dev, quality=q, subsampling=sub)
    _same(got, oracle, (px.shape, q, sub, 'oracle'))
    _same(got, pillow, (px.shape, q, sub, 'Pillow'))


def test_geometry_sweep_mixed_batches(dev, golden):
  """All sizes, grey and colour, all qualities in one call per subsampling: images share scan
  groups and pack units."""
  for sub in SUBSAMPLINGS:
    cases = [g for g in golden if g[3] == 0 and (g[2] == sub or (g[0].shape[2] == 1 and sub == '4:2:0'))]
    assert len(cases) >= 40
    files = jpeg.encode_jpeg_batch([torch.from_numpy(g[0]).to(dev) for g in cases], quality=[g[1] for g in cases],
                                   subsampling=sub)
    for got, (px, q, _, _, pillow, oracle) in zip(files, cases):
      _same(got, oracle, (px.shape, q, sub, 'oracle'))
      _same(got, pillow, (px.shape, q, sub, 'Pillow'))


def test_restart_intervals(dev, golden):
  """Intervals 1, 2, one row and 65535 on 33 x 47 and 40 x 72: more than eight segments (RSTn counts
  modulo 8), the predictor's reset, every segment's 1-padding."""
  cases = [g for g in golden if g[3] != 0]
  assert {g[3] for g in cases} == {1, 2, 'row', 65535} and len(cases) == 18
  for px, q, sub, restart, pillow, oracle in cases:
    assert restart != 1 or oracle.count(b'\xff\xd7') >= 1   # RST7 reached: more than eight segments
    got = _encode(px, dev, quality=q, subsampling=sub, restart_interval=restart)
    _same(got, oracle, (px.shape, q, sub, restart, 'oracle'))
    _same(got, pillow, (px.shape, q, sub, restart, 'Pillow'))


def test_block_count_boundaries(dev, consts):
  """One block; as many blocks as a pack unit, a scan group and a transform tile hold, and one more; the constant
  picture, whose blocks are 6 bits (grey) -- the most blocks per output byte.  A block longer than
  an owner's range cannot occur: a pack unit owns whole blocks, 64 at a time."""
  unit, group = consts
  tile = _lib.lib().se3ds_jpeg_encode_tile_blocks()
  shapes = [(8, 8, 1), (1, 1, 3)]
  # as many MCUs in a row as a transform tile holds, and one more: 4:4:4 here, the others below
  shapes += [(9, 8 * (tile // 3), 3), (17, 8 * (tile // 3) + 1, 3), (8, 8 * tile + 3, 1)]
  for blocks in (unit, unit + 1, group, group + 1, 2 * group + unit + 1):
    shapes.append((8, 8 * blocks, 1))
  for h, w, c in shapes:
    px = E.scene('mixed', h, w, c, seed=w)
    _same(_encode(px, dev, quality=90, subsampling='4:4:4'), E.encode(px, 90, '4:4:4'), (h, w, c))
  for h, w, sub in ((20, 16 * (tile // 6), '4:2:0'), (20, 16 * (tile // 6) + 1, '4:2:0'), (9, 16 * (tile // 4) + 5, '4:2:2')):
    px = E.scene('mixed', h, w, 3, seed=w)
    _same(_encode(px, dev, quality=75, subsampling=sub), E.encode(px, 75, sub), (h, w, sub))
  for h, w, c, sub in ((8, 8 * (group + unit + 1), 1, '4:4:4'), (136, 136, 1, '4:4:4'), (48, 80, 3, '4:2:0'),
                       (40, 264, 3, '4:4:4')):
    px = E.scene('constant', h, w, c)
    want = E.encode(px, 75, sub)
    if c == 1:   # SOS header to EOI: the first block, then 6 bits a block
      blocks = -(-h // 8) * -(-w // 8)
      assert len(want) - want.index(b'\xff\xda') - 10 - 2 <= (blocks * 6 + 7) // 8 + 3
    _same(_encode(px, dev, quality=75, subsampling=sub), want, ('constant', h, w, c))


def _raw_stream(px, quality):
  """A grey picture's unstuffed bytes and the bit position of every block (no restarts)."""
  coefs, _ = E.coefficients(px, quality, 'grey')
  blocks, comp, mcu = E.scan_order(coefs, 'grey')
  vals, lens, owner = E.symbols(blocks, comp, mcu, 0)
  pos = np.concatenate([[0], np.cumsum(np.bincount(owner, weights=lens, minlength=len(blocks)).astype(np.int64))])
  stuffed, _, ff = J._pack(vals, lens)
  raw = np.delete(np.frombuffer(stuffed, np.uint8), np.asarray(ff, np.int64) + 1)
  return raw, pos


def test_stuffing_at_the_owners_boundaries(dev, consts):
  """Noise at quality 100: dense FF stuffing.  The seed is picked with the oracle so that an FF is
  the last byte of one pack unit's range and an FF is the first byte of the next one's (the byte
  in which the unit's first block begins belongs to the unit in front)."""
  unit, _ = consts
  w = 8 * unit * 6
  last = first = both = None
  for seed in range(400):
    px = E.scene('noise', 8, w, 1, seed=seed)
    raw, pos = _raw_stream(px, 100)
    cuts = (pos[unit::unit][:-1] + 7) // 8   # the first byte of every unit but the first
    cuts = cuts[cuts < len(raw)]
    if last is None and np.any(raw[cuts - 1] == 0xFF):
      last = px
    if first is None and np.any(raw[cuts] == 0xFF):
      first = px
    if both is None and np.any((raw[cuts - 1] == 0xFF) & (raw[cuts] == 0xFF)):
      both = px
    if last is not None and first is not None and (both is not None or seed >= 60):
      break
  assert last is not None and first is not None
  for px in (last, first, both):
    if px is not None:
      want = E.encode(px, 100, '4:4:4')
      assert want.count(b'\xff\x00') >= 20
      _same(_encode(px, dev, quality=100, subsampling='4:4:4'), want, 'noise')
  px = E.scene('noise', 64, 96, 3, seed=7)
  for sub in SUBSAMPLINGS:
    _same(_encode(px, dev, quality=100, subsampling=sub), E.encode(px, 100, sub), ('noise', sub))


def test_checkerboard_largest_magnitudes_and_zero_runs(dev):
  for h, w, c, sub in ((40, 40, 3, '4:4:4'), (40, 40, 3, '4:2:0'), (33, 47, 1, '4:4:4'), (17, 250, 3, '4:2:2')):
    px = E.scene('checker', h, w, c)
    coefs, _ = E.coefficients(px, 100, 'grey' if c == 1 else E.SUBSAMPLING[sub])
    assert np.abs(coefs[0][..., 1:]).max() >= 512   # category 10
    _same(_encode(px, dev, quality=100, subsampling=sub), E.encode(px, 100, sub), ('checker', h, w, c, sub))
  # a coarse quantiser on noise: few coefficients, far apart -- zero runs of 16 and more (ZRL)
  px = E.scene('noise', 24, 56, 1, seed=2)
  blocks, comp, mcu = E.scan_order(E.coefficients(px, 5, 'grey')[0], 'grey')
  gaps = [np.diff(np.flatnonzero(np.concatenate([[1], row[1:]]))).max(initial=0) for row in blocks[:, J.ZZ]]
  assert max(gaps) > 32 and sum(g > 16 for g in gaps) >= 5
  _same(_encode(px, dev, quality=5, subsampling='4:4:4'), E.encode(px, 5, '4:4:4'), 'zero runs')


def test_round_trip_through_the_decoder(dev, golden):
  """decode_jpeg_batch of the encoder's files equals the decoder's oracle on the same bytes; at
  quality 100 and 4:4:4 the pixels come back within the error the encoder's ORACLE has on that
  input (computed here, not a constant)."""
  cases = [g for g in golden if g[0].shape[:2] in ((33, 47), (64, 96), (20, 9)) and g[3] == 0 and g[1] in (50, 100)]
  assert len(cases) == 24
  files = [_encode(px, dev, quality=q, subsampling=sub) for px, q, sub, _, _, _ in cases]
  decoded = jpeg.decode_jpeg_batch(files, dev)
  for f, d, (px, q, sub, _, _, oracle) in zip(files, decoded, cases):
    got = d.cpu().numpy()
    assert np.array_equal(got, J.decode(f)), (px.shape, q, sub)
    if q == 100 and (sub == '4:4:4' or px.shape[2] == 1):
      bound = np.abs(J.decode(oracle).astype(np.int64) - px).max()
      assert np.abs(got.astype(np.int64) - px).max() <= bound, (px.shape, bound)


def test_one_real_shape_and_determinism(dev):
  px = E.scene('mixed', 512, 1024, 3, seed=4)
  want = E.encode(px, 75, '4:2:0')
  x = torch.from_numpy(px).to(dev)
  first = jpeg.encode_jpeg_batch([x], quality=75, subsampling='4:2:0')[0]
  _same(first, want, '512 x 1024')
  assert jpeg.encode_jpeg_batch([x], quality=75, subsampling='4:2:0')[0] == first
  small = [torch.from_numpy(E.scene('noise', 33, 47, 3, seed=s)).to(dev) for s in range(6)]
  a = jpeg.encode_jpeg_batch(small + [x], quality=90, restart_interval='row')
  b = jpeg.encode_jpeg_batch(small + [x], quality=90, restart_interval='row')
  assert a == b
  _same(a[-1], E.encode(px, 90, '4:2:0', 'row'), '512 x 1024, restart rows, in a batch')


def test_table_validation_launches_nothing(dev):
  L = _lib.lib()
  BAD, UNSUPPORTED, WORKSPACE = (_lib.ABI[k] for k in ('SE3DS_E_BADSHAPE', 'SE3DS_E_UNSUPPORTED', 'SE3DS_E_WORKSPACE'))
  x = torch.from_numpy(E.scene('mixed', 16, 24, 3)).to(dev)
  spec = jpeg.encode_specs([x.shape], [x.dtype])
  batch = jpeg.JpegEncodeBatch([x], spec)
  batch.out.fill_(0xA5)
  batch.sizes.fill_(-7)
  good = batch.table.copy()

  def call(table, workspace_bytes=batch.workspace_bytes, out_bytes=batch.out_bytes, table_dev=None, n=1, phases=15):
    return L.se3ds_jpeg_encode(_lib.ptr(batch.table_dev) if table_dev is None else table_dev,
                               None if table is None else table.ctypes.data, n, _lib.ptr(batch.workspace),
                               workspace_bytes, _lib.ptr(batch.out), out_bytes, _lib.ptr(batch.sizes), phases,
                               _lib.stream())

  def edit(field, value):
    t = good.copy()
    t[0, field] = value
    return t

  quant = good.copy()
  quant[0, 16:].view(np.uint16)[5] = 0
  assert call(edit(0, 0)) == BAD                      # null pixels
  assert call(good, table_dev=0) == BAD               # null table
  assert call(None) == BAD                            # null host table
  assert call(good, n=0) == BAD and call(good, phases=0) == BAD and call(good, phases=16) == BAD
  assert call(edit(1, 0)) == BAD and call(edit(2, 0)) == BAD   # zero size
  assert call(edit(1, 65536)) == UNSUPPORTED
  assert call(edit(3, 2)) == BAD                      # two components
  assert call(edit(4, 4)) == UNSUPPORTED                # 4 x 1 sampling
  t = edit(4, 1)
  t[0, 5] = 2
  assert call(t) == UNSUPPORTED                       # 1 x 2 sampling
  assert call(edit(6, 65536)) == BAD and call(edit(7, 1)) == BAD and call(edit(8, 1)) == BAD and call(quant) == BAD
  assert call(good, out_bytes=batch.out_bytes - 1) == BAD
  assert call(good, workspace_bytes=batch.workspace_bytes - 1) == WORKSPACE
  for t in (edit(1, 0), edit(4, 4), quant):
    assert L.se3ds_jpeg_encode_workspace_bytes(t.ctypes.data, 1) == 0
    assert L.se3ds_jpeg_encode_out_bytes(t.ctypes.data, 1) == 0
  torch.cuda.synchronize()
  assert bool((batch.out == 0xA5).all()) and bool((batch.sizes == -7).all())   # nothing ran
  for phases in (1, 2, 4, 8):   # the phases apart, as the timing tool launches them
    batch.launch(phases)
  _same(batch.files()[0], E.encode(x.cpu().numpy(), 75, '4:2:0'), 'the same buffers, valid table')
  with pytest.raises(ValueError, match='images'):
    jpeg.encode_jpeg_batch([x, x.cpu()])


def test_save_augmentation(dev, tmp_path):
  images = torch.from_numpy(np.stack([E.scene('mixed', 32, 64, 3, seed=s) for s in range(3)])).to(dev)
  aug = perturbation_utils.Augmentation(
      images=images, positions=torch.arange(9, dtype=torch.float32, device=dev).reshape(3, 3),
      offsets=np.arange(9, dtype=np.float32).reshape(3, 3) / 4, proportion_invalid=np.array([0.0, 0.01, 0.015]),
      num_drawn=11)
  paths = perturbation_utils.save_augmentation(aug, str(tmp_path / 'out'), prefix='pano', quality=85)
  assert [os.path.basename(p) for p in paths] == ['pano_0.jpg', 'pano_1.jpg', 'pano_2.jpg', 'pano.npz']
  assert sorted(os.listdir(tmp_path / 'out')) == sorted(os.path.basename(p) for p in paths)
  files = [open(p, 'rb').read() for p in paths[:3]]
  for f, x in zip(files, images.cpu().numpy()):
    _same(f, E.encode(x, 85, '4:2:0'), 'augmentation')
  for d, f in zip(jpeg.decode_jpeg_batch(files, dev), files):
    assert np.array_equal(d.cpu().numpy(), J.decode(f))
  z = np.load(paths[3])
  assert np.array_equal(z['positions'], aug.positions.cpu().numpy()) and np.array_equal(z['offsets'], aug.offsets)
  assert np.array_equal(z['proportion_invalid'], aug.proportion_invalid) and int(z['num_drawn']) == 11


def test_logger_writes_jpeg_summaries(dev, tmp_path):
  rgb = torch.from_numpy(np.stack([E.scene('mixed', 24, 40, 3, seed=s) for s in range(2)])).to(dev)
  grey = torch.from_numpy(E.scene('smooth', 24, 40, 1)[None]).to(dev)
  events = {}
  for fmt in ('jpeg', 'png', None):
    kw = {} if fmt is None else {'image_format': fmt}
    log = logger_lib.UniversalLogger(str(tmp_path / str(fmt)), 0, **kw)
    log.log_images(3, rgb=rgb, grey=grey)
    log.close()
    events[fmt] = {k: v for _, _, values in tf_events.read_events(log.summary_writer.path) for k, v in values.items()}
  values = events['jpeg']
  assert sorted(values) == ['grey', 'rgb/image/0', 'rgb/image/1']
  want = jpeg.encode_jpeg_batch([grey[0], rgb[0], rgb[1]], quality=90)
  assert [values[t] for t in ('grey', 'rgb/image/0', 'rgb/image/1')] == [(24, 40, f) for f in want]
  _same(values['rgb/image/1'][2], E.encode(rgb[1].cpu().numpy(), 90, '4:2:0'), 'summary')
  assert jpeg.parse_jpeg(values['grey'][2]).components == 1
  assert events['png'] == events[None] and events[None]['grey'][2][:4] == b'\x89PNG'   # the default is unchanged
