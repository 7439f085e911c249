"""The device JPEG decoder (csrc/jpeg.hip, utils/jpeg.py) against the NumPy oracle of tests/_jpeg_ref.py,
bit for bit.  The files are written from chosen coefficients, so the expected pixels come from the
oracle's vectorised inverse transform on those coefficients; sizes that matter to the kernel (chunk,
window) come from the constants the library reports."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as J
from se3ds_amd import _lib
from se3ds_amd.utils import jpeg

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (8, 8), (9, 17), (17, 33), (5, 4), (3, 5), (40, 2), (33, 6), (64, 48)]


@pytest.fixture(scope='module')
def dev():
  return torch.device('cuda', torch.cuda.current_device())


@pytest.fixture(scope='module')
def consts():
  L = _lib.lib()
  lanes, chunk = L.se3ds_jpeg_decode_lanes(), L.se3ds_jpeg_decode_chunk_bytes()
  return lanes, chunk, lanes * chunk


def _np(tensors):
  return [t.cpu().numpy() for t in tensors]


def _same(got, want, what=''):
  assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
  bad = np.flatnonzero((got != want).reshape(-1))
  assert bad.size == 0, f'{what}: {bad.size} of {got.size} bytes differ, first at {int(bad[0])}'


@pytest.fixture(scope='module')
def sweep():
  rng = np.random.default_rng(21)
  files, want = [], []
  for h, w in SIZES:
    for sampling in J.SAMPLINGS:
      coefs = J.random_coefs(rng, h, w, sampling)
      files.append(J.write_jpeg(coefs, h, w, sampling).data)
      want.append(J.expected(coefs, h, w, sampling))
  return files, want


def test_geometry_sweep_single_calls(dev, sweep):
  files, want = sweep
  for i, (f, w) in enumerate(zip(files, want)):
    (got,) = _np(jpeg.decode_jpeg_batch([f], dev))
    _same(got, w, f'file {i}')


def test_geometry_sweep_one_mixed_batch(dev, sweep):
  files, want = sweep
  got = _np(jpeg.decode_jpeg_batch(files, dev))
  assert len(got) == len(files) == 40
  for i, (g, w) in enumerate(zip(got, want)):
    _same(g, w, f'file {i}')
  for n in (1, 9):
    for i, g in enumerate(_np(jpeg.decode_jpeg_batch(files[7:7 + n], dev))):
      _same(g, want[7 + i], f'batch of {n}, file {i}')


# ------------------------------------------------------------------------------------ windows
def _dense_444(rng, side, dense_coefficients, zero_mcus=()):
  """4:4:4 coefficients of large magnitude, dense in the first `dense_coefficients` AC positions in
  scan order (MCU by MCU, Y Cb Cr, zig-zag), nothing behind; the MCUs of zero_mcus hold DC only."""
  coefs = J.random_coefs(rng, side, side, '444', ac=100)
  for c in coefs:
    c[..., 1:][c[..., 1:] == 0] = 7
  n = coefs[0].shape[0] * coefs[0].shape[1]
  order = np.stack([c.reshape(n, 64)[:, J.ZZ] for c in coefs], 1)   # (mcu, component, zig-zag)
  for m in zero_mcus:
    order[m, :, 1:] = 0
  ac = order[:, :, 1:].reshape(-1)
  ac[dense_coefficients:] = 0
  order[:, :, 1:] = ac.reshape(n, 3, 63)
  for ci, c in enumerate(coefs):
    c.reshape(n, 64)[:, J.ZZ] = order[:, ci]
  return coefs


def _fill(coefs, block, k):
  """The k filler coefficients `write_jpeg(fill=...)` put into luma block `block` of a 4:4:4 file."""
  flat = coefs[0].reshape(-1, 64)
  flat[block // 3, J.ZZ[1:1 + k]] = -1


@pytest.fixture(scope='module')
def window_files(consts):
  """name -> (file, expected pixels, Written): entropy lengths below one chunk, W - 1, W, W + 1, and
  more than 3 W plus a partial window with a stuffed FF on the first window boundary."""
  lanes, chunk, W = consts
  rng = np.random.default_rng(22)
  out = {}
  coefs = J.random_coefs(rng, 8, 8, '444', density=0.2)
  w = J.write_jpeg(coefs, 8, 8, '444')
  assert 0 < w.segments[0][1] < chunk
  out['short'] = (w, J.expected(coefs, 8, 8, '444'))

  # a dense stream that ends about 12 bytes short of W; the last MCU holds the filler
  side = 8 * int(np.ceil(np.sqrt(W / 300.0)))
  mcus = (side // 8) ** 2
  last = (mcus - 1) * 3
  bits = 12.3                                   # per coefficient, measured below
  count = int((W - 12) * 8 / bits)
  for _ in range(8):
    base = _dense_444(np.random.default_rng(23), side, count, zero_mcus=[mcus - 1])
    length = J.write_jpeg(base, side, side, '444').segments[0][1]
    bits = length * 8.0 / count
    if W + 1 - 22 <= length <= W - 3:
      break
    count += int((W - 12 - length) * 8 / bits)
  else:
    raise AssertionError(f'no base stream near W: {length}')
  per_mcu = bits * 189 / 8                      # bytes of a dense MCU
  for name, target in (('W-1', W - 1), ('W', W), ('W+1', W + 1)):
    near = (target - length) * 8 // 3
    w = J.write_jpeg(base, side, side, '444', fill=(last, lambda raw, spans, ff: len(raw) == target,
                                                    range(max(near - 3, 0), min(near + 4, 64))))
    coefs = [c.copy() for c in base]
    _fill(coefs, last, w.filled)
    assert w.segments[0][1] == target
    out[name] = (w, J.expected(coefs, side, side, '444'))

  # > 3 W: dense MCUs, then a band whose luma blocks are three times (run 15, 1023) -- fifteen 1
  # bits, a 0, ten 1 bits: most bytes are stuffed FFs -- across the first window boundary
  lead = int((W - 1200) / per_mcu)
  band = list(range(lead, lead + 120))
  mcus = len(band) + int(np.ceil((3.4 * W - 2400) / per_mcu))
  side = 8 * int(np.ceil(np.sqrt(mcus)))
  coefs = _dense_444(np.random.default_rng(24), side, 1 << 30, zero_mcus=band)
  flat = coefs[0].reshape(-1, 64)
  for m in band[1:]:
    flat[m, J.ZZ[[16, 32, 48]]] = 1023
  w = J.write_jpeg(coefs, side, side, '444', fill=(3 * lead, lambda raw, spans, ff: (W - 1) in ff))
  _fill(coefs, 3 * lead, w.filled)
  assert w.segments[0][1] > 3 * W + chunk and w.segments[0][1] % W > chunk
  out['long'] = (w, J.expected(coefs, side, side, '444'))
  return out


def test_window_files_straddle_what_they_should(consts, window_files):
  lanes, chunk, W = consts
  w = window_files['long'][0]
  spans, ff = w.symbols[0], w.stuffed[0]
  for unit in (chunk, W):
    assert np.any(spans[:, 0] // (8 * unit) != spans[:, 1] // (8 * unit)), f'no symbol across a {unit} boundary'
    assert np.any(ff % unit == unit - 1), f'no stuffed FF 00 across a {unit} boundary'
  assert [window_files[k][0].segments[0][1] for k in ('W-1', 'W', 'W+1')] == [W - 1, W, W + 1]


@pytest.mark.parametrize('name', ['short', 'W-1', 'W', 'W+1', 'long'])
def test_window_logic(dev, consts, window_files, name):
  lanes, chunk, W = consts
  w, want = window_files[name]
  (got,), pending = jpeg.decode_jpeg_batch([w.data], dev, check=False)
  pending.check()
  _same(got.cpu().numpy(), want, name)
  windows = -(-w.segments[0][1] // W)
  rounds = int(jpeg.status_rounds(pending.words)[0])
  assert 2 * windows <= rounds <= windows * (lanes + 1), (rounds, windows)


def test_segment_end_just_behind_a_chunk_boundary(dev, consts):
  """The last symbol starts in one chunk and ends in the first byte of the next chunk of the same
  window, with padding behind it: the lane that owns that byte enters behind the last block and must
  not take the padding for more data."""
  lanes, chunk, W = consts
  written, coefs, h, w = J.chunk_tail_file(chunk, W)
  (at, n), spans = written.segments[0], written.symbols[0]
  assert n % chunk == 1 and n % W != 1 and n > chunk
  assert spans[-1, 0] // (8 * chunk) == n // chunk - 1 and spans[-1, 1] // 8 == n - 1   # the straddle
  assert 8 * n - 1 - spans[-1, 1] > 0                                                  # padding bits
  want = J.expected(coefs, h, w, 'grey')
  (got,) = _np(jpeg.decode_jpeg_batch([written.data], dev))
  _same(got, want)
  # one byte more behind the same stream is too long, whichever lane sees it
  scan = jpeg.parse_jpeg(written.data)
  longer = written.data[:at + n] + b'\x00' + written.data[at + n:]
  with pytest.raises(ValueError, match='behind the last block'):
    jpeg.decode_jpeg_batch([longer], dev)
  assert jpeg.parse_jpeg(longer).segments[0][1] == scan.segments[0][1] + 1


def test_worst_case_for_synchronisation(dev, consts):
  """A flat 4:2:0 image: every block is "DC difference 0, EOB" but the first, whose DC difference
  puts the stream out of step with every guess: a periodic stream never pulls a wrong decoder in."""
  lanes, chunk, W = consts
  mcus = -(-3 * W // 2 // 4) + 64            # 4 bytes per MCU
  mx = 128
  my = -(-mcus // mx)
  data = J.flat_420(16 * my, 16 * mx, 5)
  scan = jpeg.parse_jpeg(data)
  length = scan.segments[0][1]
  assert length >= 3 * W // 2
  (got,), pending = jpeg.decode_jpeg_batch([data], dev, check=False)
  pending.check()
  got = got.cpu().numpy()
  want = J.expected([np.array([[[5] + [0] * 63]])] + [np.zeros((1, 1, 64), np.int64)] * 2, 8, 8, '444')[0, 0]
  assert got.shape == (16 * my, 16 * mx, 3)
  assert np.array_equal(got[:8, :8], np.broadcast_to(want, (8, 8, 3)))
  assert np.all(got == want), 'the flat image is not flat'
  windows = -(-length // W)
  rounds = int(jpeg.status_rounds(pending.words)[0])
  print(f'flat 4:2:0, {length} entropy bytes: {rounds} rounds in {windows} windows')
  assert rounds <= windows * (lanes + 1)


# ------------------------------------------------------------------------------------ the rest
@pytest.mark.parametrize('h,w,sampling,dri', [(24, 40, '420', 1), (32, 80, '422', 5), (40, 40, '444', 7),
                                             (48, 64, '420', 1), (17, 70, 'grey', 2)])
def test_restart_intervals(dev, h, w, sampling, dri):
  """DRI 1, DRI = MCUs per row (5 at 80 wide 4:2:2), a DRI that does not divide the MCU count (25 by
  7), more than 8 segments (the RSTn numbers wrap), a grey file."""
  rng = np.random.default_rng(h * w)
  coefs = J.random_coefs(rng, h, w, sampling)
  written = J.write_jpeg(coefs, h, w, sampling, dri=dri)
  scan = jpeg.parse_jpeg(written.data)
  assert len(scan.segments) == len(written.segments) == -(-scan.mcus_x * scan.mcus_y // dri)
  if (h, w) == (48, 64):
    assert len(scan.segments) > 8
  (got,) = _np(jpeg.decode_jpeg_batch([scan], dev))
  _same(got, J.expected(coefs, h, w, sampling))


def test_coding_extremes(dev):
  rng = np.random.default_rng(25)
  files, want = [], []
  for sampling in J.SAMPLINGS:
    coefs = J.extreme_coefs(rng, 24, 40, sampling)
    files.append(J.write_jpeg(coefs, 24, 40, sampling).data)     # DC category 11, ZRL chains, no EOB
    want.append(J.expected(coefs, 24, 40, sampling))
    coefs = J.random_coefs(rng, 24, 40, sampling)
    files.append(J.write_jpeg(coefs, 24, 40, sampling, huffman=J.LONG_CODES).data)   # 16-bit codes only
    want.append(J.expected(coefs, 24, 40, sampling))
    small = [np.clip(c, -2, 2) for c in coefs]
    quant = (J.FLAT_QUANT * 300, J.FLAT_QUANT * 1000)
    files.append(J.write_jpeg(small, 24, 40, sampling, quant=quant, dqt16=True, sof='C1').data)
    want.append(J.expected(small, 24, 40, sampling, quant))
  for i, (g, w) in enumerate(zip(_np(jpeg.decode_jpeg_batch(files, dev)), want)):
    _same(g, w, f'file {i}')


def test_saturation(dev):
  """A few large coefficients per block: the sample leaves [-512, 511] before the clamp, where a table
  look-up wraps and SIMD builds saturate.  This decoder saturates, and so does the oracle, whose
  int64 arithmetic asserts that every intermediate fits int32."""
  rng = np.random.default_rng(26)
  quant = (J.FLAT_QUANT * 16, J.FLAT_QUANT * 16)
  for sampling in ('444', '420'):
    coefs = J.random_coefs(rng, 40, 56, sampling, density=0.0, dc=300)
    for c in coefs:
      c[..., 1] = rng.integers(-100, 101, c.shape[:2])
      c[..., 8] = rng.integers(-100, 101, c.shape[:2])
    stats = []
    want = J.expected(coefs, 40, 56, sampling, quant, stats=stats)
    assert max(s[1] for s in stats) > 640, stats
    (got,) = _np(jpeg.decode_jpeg_batch([J.write_jpeg(coefs, 40, 56, sampling, quant=quant).data], dev))
    _same(got, want, sampling)
    assert (got == 0).any() and (got == 255).any()


def test_channels(dev):
  rng = np.random.default_rng(27)
  for sampling in ('420', '422', 'grey'):
    coefs = J.random_coefs(rng, 19, 35, sampling)
    data = J.write_jpeg(coefs, 19, 35, sampling).data
    for channels in (0, 1, 3):
      (got,) = _np(jpeg.decode_jpeg_batch([data], dev, channels=channels))
      want = J.expected(coefs, 19, 35, sampling, channels=channels)
      assert want.shape[-1] == (channels or (1 if sampling == 'grey' else 3))
      _same(got, want, f'{sampling} channels={channels}')
  with pytest.raises(ValueError, match='channels'):
    jpeg.decode_jpeg_batch([data], dev, channels=2)


def test_malformed_corpus_and_its_neighbours(dev):
  rng = np.random.default_rng(28)
  good, want = [], []
  for sampling in ('420', '444'):
    coefs = J.random_coefs(rng, 30, 50, sampling)
    good.append(J.write_jpeg(coefs, 30, 50, sampling, dri=3).data)
    want.append(J.expected(coefs, 30, 50, sampling))
  bad = J.bad_cases()
  assert {c.status for c in bad} == set(J.STATUS[1:])
  for c in bad:
    reason = jpeg.jpeg_failure(J.STATUS.index(c.status))
    with pytest.raises(ValueError) as e:
      jpeg.decode_jpeg_batch([good[0], c.data, good[1]], dev)
    assert str(e.value) == f'image 1: {reason}', c.name
    out, pending = jpeg.decode_jpeg_batch([good[0], good[1], c.data], dev, check=False)
    with pytest.raises(ValueError) as e:
      pending.check()
    assert str(e.value) == f'image 2: {reason}', c.name
    for g, w in zip(_np(out[:2]), want):   # the neighbours of a bad file are still exact
      _same(g, w, c.name)


def test_record_writer_takes_jpeg_bytes(dev, tmp_path):
  from se3ds_amd.datasets import record_writer
  rng = np.random.default_rng(29)
  h, w = 16, 32
  coefs = J.random_coefs(rng, h, w, '420')
  data = J.write_jpeg(coefs, h, w, '420').data
  image = torch.from_numpy(J.expected(coefs, h, w, '420')).to(dev)
  planes = dict(depth=torch.from_numpy(rng.integers(-2 ** 15, 2 ** 15, (h, w)).astype(np.int16)).to(dev),
                proj_image=torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev),
                proj_depth=torch.from_numpy(rng.integers(-2 ** 15, 2 ** 15, (h, w)).astype(np.int16)).to(dev),
                proj_mask=torch.from_numpy(rng.integers(0, 2, (h, w), dtype=np.uint8) * 255).to(dev))
  paths = []
  for name, first in (('jpeg', data), ('tensor', image)):
    paths.append(str(tmp_path / f'train-{name}.tfrecord'))
    with record_writer.R2RRecordWriter(paths[-1], dev) as writer:
      writer.add(image=first, scan_id=b'a', **planes)
      writer.add(image=image, scan_id=b'b', **planes)
      with pytest.raises(ValueError, match='image'):
        writer.add(image=J.write_jpeg(J.random_coefs(rng, 8, 8, '420'), 8, 8, '420').data, **planes)
      with pytest.raises(ValueError, match='image'):
        writer.add(image=J.write_jpeg(J.random_coefs(rng, h, w, 'grey'), h, w, 'grey').data, **planes)
  a, b = open(paths[0], 'rb').read(), open(paths[1], 'rb').read()
  assert len(a) > 1000 and a == b


def test_record_writer_keeps_its_examples_when_a_jpeg_does_not_decode(dev, tmp_path):
  from se3ds_amd.datasets import record_writer
  rng = np.random.default_rng(31)
  h, w = 16, 32
  good = J.write_jpeg(J.random_coefs(rng, h, w, '420'), h, w, '420')
  at, n = good.segments[0]
  bad = good.data[:at + n // 2] + b'\xff\xd9'
  planes = dict(depth=torch.zeros((h, w), dtype=torch.int16, device=dev),
                proj_image=torch.zeros((h, w, 3), dtype=torch.uint8, device=dev),
                proj_depth=torch.zeros((h, w), dtype=torch.int16, device=dev),
                proj_mask=torch.zeros((h, w), dtype=torch.uint8, device=dev))
  path = str(tmp_path / 'train-bad.tfrecord')
  writer = record_writer.R2RRecordWriter(path, dev)
  writer.add(image=good.data, **planes)
  writer.add(image=bad, **planes)
  with pytest.raises(ValueError, match='image 1: the scan does not decode'):
    writer.flush()
  assert len(writer._pending) == 2 and writer.examples == 0
  with pytest.raises(ValueError, match='depth'):   # the usual message, also beside JPEG input
    writer.add(image=good.data, **dict(planes, depth=planes['depth'][:8]))
  writer.abort()
  assert not os.path.exists(path) and not os.path.exists(path + '.tmp')


def test_two_runs_give_identical_bytes(dev, sweep, window_files):
  files = sweep[0][::3] + [window_files['long'][0].data]
  first = _np(jpeg.decode_jpeg_batch(files, dev))
  second = _np(jpeg.decode_jpeg_batch(files, dev))
  for a, b in zip(first, second):
    assert a.tobytes() == b.tobytes()


def test_tables_are_validated_before_anything_runs(dev):
  """se3ds_jpeg_decode on the host copies: BADSHAPE and WORKSPACE, nothing launched."""
  L = _lib.lib()
  data = J.write_jpeg(J.random_coefs(np.random.default_rng(30), 16, 32, '420'), 16, 32, '420').data
  scan = jpeg.parse_jpeg(data)
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    jpeg.decode_jpeg_batch([scan._replace(h0=3)], dev)
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    jpeg.decode_jpeg_batch([scan._replace(restart_interval=1)], dev)   # the MCU counts do not add up
  broken = scan.huffman.copy()
  broken[0, :16] = 3                                          # three codes of one bit
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    jpeg.decode_jpeg_batch([scan._replace(huffman=broken)], dev)
  assert L.se3ds_jpeg_decode_fields() == 200 and L.se3ds_jpeg_decode_segment_fields() == 5
