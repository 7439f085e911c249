"""The device PNG encoder on the GPU (csrc/png_encode.hip): filter choice against a NumPy
restatement of the rule, streams byte for byte against the host build of csrc/deflate_core.h
(tools/deflate_host_check.cpp), zlib and both decoders of utils/png.py on the result, the size
bounds, the untouched rest of the output buffer, run-to-run identity; se3ds_grid_quantize and
utils/image_grid.py against NumPy."""
import math
import zlib

import numpy as np
import pytest
import torch

import _png_encode_ref as R
import _png_ref
from se3ds_amd import _lib
from se3ds_amd.utils import image_grid, png

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CANARY = 0xA5
# Per strip beyond zlib's Z_RLE stream of the same bytes: the dynamic block's header with the fixed
# code-length code at its largest (3 + 14 + 57 + 4 x 287 bits = 153 bytes) and the empty stored
# block (5 bytes).  The margin for the length-limited code on top of that is 0: measured, the
# encoder stays below this allowance on every compressible content here.
STRIP_ALLOWANCE = 158


class Encoded:
  """Every geometry x content once, in one mixed launch: the shared reference of the tests below."""

  def __init__(self, tmp):
    max_row = _lib.lib().se3ds_png_encode_max_row_bytes()
    self.names, self.pixels = [], []
    for gi, (h, w, c) in enumerate(R.GEOMETRIES + [(1, max_row, 1)]):
      for name, px in R.contents(h, w, c, seed=gi).items():
        self.names.append(((h, w, c), name))
        self.pixels.append(px)
    self.tensors = [torch.from_numpy(p).to(DEV) for p in self.pixels]
    self.table, self.sizes, self.buffer = png.encode_streams(self.tensors, 'adaptive', fill=CANARY)
    self.streams = [self.buffer[int(r[6]):int(r[6]) + int(s[0])].tobytes()
                    for r, s in zip(self.table, self.sizes)]
    self.filtered = [R.filter_rows(p, R.ADAPTIVE) for p in self.pixels]
    self.strips = [R.strips_of(f, f.shape[1] - 1) for _, f in self.filtered]
    exe = R.build_host_program(tmp, sanitize=False)
    cases = [(s, k == len(strips) - 1) for strips in self.strips for k, s in enumerate(strips)]
    host = iter(R.run_host_program(exe, cases, tmp))
    self.host = [[next(host) for _ in strips] for strips in self.strips]


@pytest.fixture(scope='module')
def enc(tmp_path_factory):
  return Encoded(tmp_path_factory.mktemp('png_encode'))


def test_filter_types_follow_the_rule(enc):
  for (geom, name), stream, (types, filtered), adler in zip(enc.names, enc.streams, enc.filtered,
                                                            enc.sizes[:, 1]):
    data = zlib.decompress(b'\x78\x01' + stream + int(adler).to_bytes(4, 'big'))   # checks the Adler-32
    assert data == filtered.tobytes(), (geom, name)
    got = np.frombuffer(data, np.uint8).reshape(filtered.shape)
    assert np.array_equal(got[:, 0], types), (geom, name)
    if name == 'horizontal ramp' and geom[1] > 1:
      assert np.all(types == 1), geom    # Sub
    if name == 'vertical ramp' and geom[0] > 1:
      assert np.all(types[1:] == 2), geom    # Up


def test_streams_equal_the_host_build_of_the_core(enc):
  for (geom, name), stream, strips, host, adler in zip(enc.names, enc.streams, enc.strips, enc.host,
                                                       enc.sizes[:, 1]):
    assert stream == b''.join(s for s, _, _ in host), (geom, name)
    for data, (s, s1, s2) in zip(strips, host):
      assert len(s) <= R.OVERHEAD + len(data), (geom, name)          # no strip exceeds its bound
      assert (s2 << 16) | s1 == zlib.adler32(data)
    assert int(adler) == zlib.adler32(b''.join(strips)), (geom, name)   # the combine on the device
    if name == 'noise' and geom[0] * geom[1] * geom[2] > 400:
      assert len(stream) == sum(R.OVERHEAD + len(d) for d in strips), geom   # stored, at the bound
      assert stream[0] == 0


def test_sizes_against_zlib_rle(enc):
  for (geom, name), stream, strips in zip(enc.names, enc.streams, enc.strips):
    if name in R.COMPRESSIBLE:
      reference = len(R.zlib_rle(b''.join(strips))) - 6   # without zlib's header and trailer
      print(geom, name, len(strips), len(stream), reference, round(len(stream) / max(reference, 1), 4))
      assert len(stream) <= reference + STRIP_ALLOWANCE * len(strips), (geom, name)


def test_rest_of_the_output_buffer_is_untouched(enc):
  ends = list(enc.table[1:, 6]) + [len(enc.buffer)]
  for (geom, name), row, size, end in zip(enc.names, enc.table, enc.sizes[:, 0], ends):
    rest = enc.buffer[int(row[6]) + int(size):int(end)]
    assert np.all(rest == CANARY), (geom, name)
  need = _lib.lib().se3ds_png_encode_out_bytes(enc.table.ctypes.data, len(enc.table))
  assert len(enc.buffer) == need


def test_two_runs_and_single_launches_are_byte_identical(enc):
  table, sizes, buffer = png.encode_streams(enc.tensors, 'adaptive', fill=CANARY)
  assert np.array_equal(sizes, enc.sizes) and np.array_equal(buffer, enc.buffer)
  for x, stream, size in zip(enc.tensors, enc.streams, enc.sizes):
    _, one_size, one = png.encode_streams([x], 'adaptive')
    assert np.array_equal(one_size[0], size) and one[:int(size[0])].tobytes() == stream


def test_files_decode_to_the_pixels(enc):
  files = png.encode_png_batch(enc.tensors)
  for data, stream in zip(files, enc.streams):
    assert png.parse_png_container(data).compressed[2:-4] == stream
  # the decoder's reconstruction kernel takes rows up to its own limit; the one wider row is
  # reconstructed by the Python reference instead
  limit = _lib.lib().se3ds_png_unfilter_max_row_bytes()
  keyed = {str(i): [f] for i, f in enumerate(files) if enc.pixels[i][0].size <= limit}
  assert len(keyed) == len(files) - 6
  for inflate in ('host', 'device'):
    out = png.decode_png_batch(keyed, DEV, inflate=inflate)
    for i, ((geom, name), px) in enumerate(zip(enc.names, enc.pixels)):
      if str(i) in keyed:
        got = out[str(i)][0].cpu().numpy().reshape(px.shape)
        assert np.array_equal(got, px), (inflate, geom, name)
  for i, ((geom, name), px) in enumerate(zip(enc.names, enc.pixels)):
    if str(i) not in keyed:
      plane = png.parse_png(files[i])
      rows = _png_ref.reconstruct(plane.filtered, plane.height, plane.row_bytes, plane.bytes_per_pixel)
      assert np.array_equal(np.asarray(rows, np.uint8).reshape(px.shape), px), (geom, name)


@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_fixed_filters(enc, mode):
  picks = [i for i, (geom, name) in enumerate(enc.names) if name == 'ramp + noise' and geom[0] > 1]
  files = png.encode_png_batch([enc.tensors[i] for i in picks], filters=mode)
  for i, data in zip(picks, files):
    plane = png.parse_png(data)
    assert plane.filtered == R.filter_rows(enc.pixels[i], mode)[1].tobytes(), enc.names[i]
  with pytest.raises(ValueError, match='filters'):
    png.encode_png_batch(enc.tensors[:2], filters=[0])


# ------------------------------------------------------------------------------ grid quantise
def _lattice(count, seed):
  """k / 255 and its fp32 neighbours, negatives, values above 1, NaN, infinities: `count` values."""
  k = np.arange(256, dtype=np.float32) / np.float32(255.0)
  pool = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                         np.float32([-0.0, -1e-3, -0.5, -7.0, 1.0001, 1.5, 300.0, 1e20, -1e20, np.nan,
                                     np.inf, -np.inf, 0.9999999, 254.5 / 255, 255.5 / 255])])
  rng = np.random.default_rng(seed)
  return pool[np.resize(rng.permutation(len(pool)), count)].astype(np.float32)   # a fresh draw of the pool


def _quantize_ref(x):
  """tf.cast(x * 255.0, tf.uint8) with the out-of-range case pinned: one fp32 product, truncated
  toward zero, saturated to [0, 255], NaN -> 0."""
  v = x.astype(np.float32) * np.float32(255.0)
  with np.errstate(invalid='ignore'):
    inside = np.trunc(np.clip(np.nan_to_num(v, nan=0.0), 0, 255)).astype(np.uint8)
  return np.where(v > 0, inside, 0).astype(np.uint8)


def _grid_ref(q, ny, nx):
  """images_to_grid of the reference (utils/image_grid.py:24-30) in NumPy."""
  _, h, w, c = q.shape
  return q[:ny * nx].reshape(ny, nx, h, w, c).transpose(0, 2, 1, 3, 4).reshape(1, ny * h, nx * w, c)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n,ny,nx', [(1, 1, 1), (3, 1, 3), (5, 2, 2), (16, 4, 4)])
def test_grid_quantize_on_the_lattice(n, ny, nx, dtype):
  for c, out_c in ((1, 1), (1, 3), (3, 3)):
    values = _lattice(n * 3 * 5 * c, seed=n + c).reshape(n, 3, 5, c)
    x = torch.from_numpy(values).to(DEV).to(dtype)
    seen = x.float().cpu().numpy()    # what the kernel reads: bf16 rounds the lattice first
    want = _grid_ref(_quantize_ref(seen), ny, nx)
    if out_c != c:
      want = np.repeat(want, 3, axis=3)
    got = image_grid._quantize_to_grid(x, ny, nx, out_c)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, ny * 3, nx * 5, out_c)
    assert np.array_equal(got.cpu().numpy(), want), (c, out_c)
  if dtype == torch.float32 and n == 16:
    five = torch.from_numpy(_lattice(16 * 3 * 5 * 3, 1).reshape(4, 4, 3, 5, 3)).to(DEV)
    assert np.array_equal(image_grid.images_to_grid(five).cpu().numpy(),
                          _grid_ref(_quantize_ref(five.cpu().numpy().reshape(16, 3, 5, 3)), 4, 4))


@pytest.mark.parametrize('show_num', [1, 2, 3, 5, 16])
def test_image_grid_keys_and_shapes(show_num):
  for batch in (max(1, show_num - 2), show_num + 3):
    values = _lattice(batch * 3 * 5 * 3, seed=show_num).reshape(batch, 3, 5, 3)
    x = torch.from_numpy(values).to(DEV)
    # the reference's index arithmetic (utils/image_grid.py:40-51)
    shown = min(show_num, batch)
    h_num = int(math.sqrt(shown))
    w_num = int(shown / h_num)
    want = _grid_ref(_quantize_ref(values[:shown]), h_num, w_num)
    got = image_grid.get_grid_image(x, show_num, None)
    assert tuple(got.shape) == (1, h_num * 3, w_num * 5, 3) and np.array_equal(got.cpu().numpy(), want)
    as_list = image_grid.get_grid_image_dict([x, x], show_num, None, 'p')
    as_dict = image_grid.get_grid_image_dict({'a': x, 'b': x[..., :1]}, show_num, None, 'p', out_c=3)
    single = image_grid.get_grid_image_dict(x, show_num, None, 'p')
    assert list(as_list) == ['p_0', 'p_1'] and list(as_dict) == ['p_a', 'p_b'] and list(single) == ['p']
    for t in (as_list['p_0'], as_list['p_1'], as_dict['p_a'], single['p']):
      assert np.array_equal(t.cpu().numpy(), want)
    assert np.array_equal(as_dict['p_b'].cpu().numpy(), np.repeat(want[..., :1], 3, axis=3))
