"""se3ds_amd.utils.ply on the device (csrc/ply.hip): the bytes of write_ply(encoder='device') against
the host loop written out in tests/_ply_ref.py, for random coordinates mixed with the values at which
a formatter goes wrong and for point counts around the workgroup's chunk; input layouts, slabs,
leftovers, the binary format and SE3DSModel.write_memory_as_pointcloud.  Comparisons are of bytes."""
import os

import numpy as np
import pytest
import torch

import _ply_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import ply

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
_cases = {}


def _chunk():
  return _lib.lib().se3ds_ply_chunk_points()


def _case(m, dtype=np.int32):
  """inputs and the host loop's file for m points, made once"""
  key = (m, np.dtype(dtype).name)
  if key not in _cases:
    coords, rgb = R.inputs(m, seed=m % 1000 + 1, colour_dtype=dtype)
    coords.setflags(write=False)
    rgb.setflags(write=False)
    _cases[key] = (coords, rgb, R.ascii_file(coords, rgb))
  return _cases[key]


def _dev(a):
  return torch.from_numpy(np.array(a)).to(DEV)


def _sizes():
  c = 256   # the chunk; test_sizes_follow_the_chunk ties it to the library's
  return [0, 1, 63, 64, 65, c - 1, c, c + 1, 3 * c + 1, 4097]


def test_sizes_follow_the_chunk():
  c = _chunk()
  assert _sizes() == [0, 1, 63, 64, 65, c - 1, c, c + 1, 3 * c + 1, 4097]


@pytest.mark.parametrize('dtype', [np.int32, np.uint8])
@pytest.mark.parametrize('m', _sizes())
def test_ascii_bytes_equal_the_host_loop(tmp_path, m, dtype):
  coords, rgb, want = _case(m, dtype)
  path = tmp_path / 'cloud.ply'
  ply.write_ply(path, _dev(coords), _dev(rgb), encoder='device')
  got = path.read_bytes()
  assert len(got) == len(want)
  assert got == want
  assert os.listdir(tmp_path) == ['cloud.ply']   # no temporary file is left behind


def test_adversarial_set_alone(tmp_path):
  """every adversarial value in every column, with the extreme colours"""
  values = R.adversarial_bits().view(np.float32)
  m = len(values)
  coords = np.stack([values, np.roll(values, 1), np.roll(values, 2)])
  rgb = np.array(R.COLOURS_I32, np.int32)[(np.arange(3 * m) % len(R.COLOURS_I32))].reshape(m, 3)
  path = tmp_path / 'adv.ply'
  ply.write_ply(path, _dev(coords), _dev(rgb), encoder='device')
  assert path.read_bytes() == R.ascii_file(coords, rgb)


def test_input_layouts(tmp_path):
  m = 3 * _chunk() + 1
  coords, rgb, want = _case(m)
  path = tmp_path / 'cloud.ply'
  # rows 0-2 of a (1, 4, M) memory, in place
  memory = torch.cat([_dev(coords), torch.ones((1, m), device=DEV)])[None]
  ply.write_ply(path, memory[0], _dev(rgb), encoder='device')
  assert path.read_bytes() == want
  # non-contiguous inputs are made contiguous by the wrapper: a transposed (M, 3), every second column
  # of a wider tensor, colours as a slice of (M, 4)
  ply.write_ply(path, _dev(coords.T.copy()).T, _dev(rgb), encoder='device')
  assert path.read_bytes() == want
  wide = torch.zeros((3, 2 * m), device=DEV)
  wide[:, ::2] = _dev(coords)
  wide_rgb = torch.zeros((m, 4), dtype=torch.int32, device=DEV)
  wide_rgb[:, :3] = _dev(rgb)
  assert not wide[:, ::2].is_contiguous() and not wide_rgb[:, :3].is_contiguous()
  ply.write_ply(path, wide[:, ::2], wide_rgb[:, :3], encoder='device')
  assert path.read_bytes() == want
  # the host encoder on device tensors: the same file
  ply.write_ply(path, memory[0], _dev(rgb))
  assert path.read_bytes() == want


def test_slabs_give_the_same_file(tmp_path):
  m = 4097
  coords, rgb, want = _case(m)
  c, colours = _dev(coords), _dev(rgb)
  slabs = (1, 300, _chunk(), m, 1 << 20)   # 1: a call and a read-back per point, 4097 of them
  for slab in slabs:
    path = tmp_path / ('slab%d.ply' % slab)
    ply.write_ply(path, c, colours, encoder='device', slab_points=slab)
    assert path.read_bytes() == want, slab
  assert sorted(os.listdir(tmp_path)) == sorted('slab%d.ply' % s for s in slabs)


def test_a_failing_write_leaves_nothing(tmp_path):
  coords, rgb, _ = _case(65)
  missing = tmp_path / 'no_such_directory' / 'cloud.ply'
  for format in ply.FORMATS:
    with pytest.raises(OSError):
      ply.write_ply(missing, _dev(coords), _dev(np.clip(rgb, 0, 255)), format=format, encoder='device')
  assert os.listdir(tmp_path) == []


@pytest.mark.parametrize('dtype', [np.int32, np.uint8])
@pytest.mark.parametrize('m', [0, 1, 17, 255, 256, 257, 4097])
def test_binary_format(tmp_path, m, dtype):
  coords, rgb, _ = _case(m, dtype)
  rgb = np.clip(rgb, 0, 255)
  path = tmp_path / 'cloud.ply'
  for slab in (1 << 20, 300):
    ply.write_ply(path, _dev(coords), _dev(rgb), format='binary_little_endian', encoder='device', slab_points=slab)
    assert path.read_bytes() == R.binary_file(coords, rgb)
  xyz, colours = ply.read_ply(path)
  assert np.array_equal(xyz.view(np.uint32), np.ascontiguousarray(coords.T).view(np.uint32))   # bit for bit
  assert np.array_equal(colours, rgb.astype(np.int32))
  assert os.listdir(tmp_path) == ['cloud.ply']


@pytest.mark.parametrize('bad', [-1, 256, -2147483648, 2147483647])
def test_binary_format_refuses_a_colour_that_is_no_uchar(tmp_path, bad):
  coords, rgb, _ = _case(4097)
  rgb = np.clip(rgb, 0, 255)
  rgb[4000, 1] = bad
  path = tmp_path / 'cloud.ply'
  for slab in (1 << 20, 300):
    with pytest.raises(ValueError, match='colour'):
      ply.write_ply(path, _dev(coords), _dev(rgb), format='binary_little_endian', encoder='device', slab_points=slab)
    assert os.listdir(tmp_path) == []


def test_reader_round_trips_the_device_text(tmp_path):
  coords, rgb, _ = _case(4097)
  path = tmp_path / 'cloud.ply'
  ply.write_ply(path, _dev(coords), _dev(rgb), encoder='device')
  xyz, colours = ply.read_ply(path)
  want = np.ascontiguousarray(coords.T)
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(xyz), nan)
  assert np.array_equal(xyz.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
  assert np.array_equal(colours, rgb)


def test_model_memory_as_pointcloud(tmp_path):
  from se3ds_amd import gin_lite
  from se3ds_amd.models import model_config, models
  gin_lite.clear_config()
  size = 16
  g = torch.Generator().manual_seed(5)
  rgb = torch.randint(0, 255, (1, size, size * 2, 3), generator=g, dtype=torch.int32).to(torch.uint8)
  seg = torch.randint(0, 42, (1, size, size * 2, 1), generator=g, dtype=torch.int32).to(torch.uint8)
  depth = torch.rand((1, size, size * 2), generator=g)
  pos = torch.randn((1, 3), generator=g)
  config = model_config.get_test_config()
  config.image_height = size
  model = models.SE3DSModel(config, device=DEV)
  p, q, b = tmp_path / 'host.ply', tmp_path / 'device.ply', tmp_path / 'binary.ply'
  model.write_memory_as_pointcloud(p)                    # an empty memory
  model.write_memory_as_pointcloud(q, encoder='device')
  assert p.read_bytes() == q.read_bytes() == (R.HEADER_ASCII % 0).encode()
  model.add_to_memory(rgb.to(DEV), seg.to(DEV), depth.to(DEV), pos.to(DEV), mask_blurred=False)
  state = model.get_memory_state()
  m = state.rgb.shape[1]
  assert m > 0
  model.write_memory_as_pointcloud(p)
  model.write_memory_as_pointcloud(q, encoder='device')
  model.write_memory_as_pointcloud(b, encoder='device', format='binary_little_endian')
  want = R.ascii_file(state.rgb_coords[0].cpu().numpy(), state.rgb[0].cpu().numpy())
  assert p.read_bytes() == want and q.read_bytes() == want
  for path in (q, b):
    xyz, colours = ply.read_ply(path)
    assert np.array_equal(xyz.view(np.uint32), state.rgb_coords[0, 0:3].T.contiguous().cpu().numpy().view(np.uint32))
    assert np.array_equal(colours, state.rgb[0].cpu().numpy())
  with pytest.raises(ValueError):
    model.write_memory_as_pointcloud(p, format='binary_little_endian')
  with pytest.raises(ValueError):
    model.write_memory_as_pointcloud(p, encoder='fast')
