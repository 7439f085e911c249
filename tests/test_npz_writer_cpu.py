"""utils/npz_writer: a stored-zip .npz written by hand with the CRCs as given, against np.load,
zipfile and np.savez.  Pure host."""
import os
import zipfile
import zlib

import numpy as np
import pytest

from se3ds_amd.utils import npz_writer as W


def _arrays():
  rng = np.random.default_rng(5)
  return {
      'global_step': np.asarray(12345678901, np.int64),                    # 0-d
      'generator/conv/kernel': rng.standard_normal((3, 3, 5, 7)).astype(np.float32),
      'generator/bn/moving_mean': np.zeros((0,), np.float32),              # empty
      'empty2d': np.zeros((4, 0, 2), np.float32),
      'odd': rng.integers(0, 255, 1001).astype(np.uint8),                  # odd-sized
      'd_optimizer/x/m': rng.standard_normal(777).astype(np.float32),
      'f64': rng.standard_normal((2, 3)),
  }


def _chunked(key, a, sizes):
  """The member of `a` handed over in chunks of the given sizes (cycled), CRC from zlib."""
  header = W.npy_header(a.shape, a.dtype)
  data = a.tobytes()

  def chunks():
    pos, i = 0, 0
    while pos < len(data):
      n = sizes[i % len(sizes)]
      yield memoryview(data)[pos:pos + n]
      pos, i = pos + n, i + 1
  return key + '.npy', header, chunks(), zlib.crc32(data, zlib.crc32(header))


def _check(path, arrays):
  with np.load(path) as f:
    assert f.files == list(arrays)
    for k, a in arrays.items():
      got = f[k]
      assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a), k
  with zipfile.ZipFile(path) as z:
    assert z.testzip() is None
    assert [i.filename for i in z.infolist()] == [k + '.npy' for k in arrays]
    assert all(i.compress_type == zipfile.ZIP_STORED and not i.flag_bits & 8 for i in z.infolist())
  assert not os.path.exists(path + '.tmp')


@pytest.mark.parametrize('force_zip64', [False, True])
def test_round_trip(tmp_path, force_zip64):
  arrays = _arrays()
  path = str(tmp_path / 'a.npz')
  size = W.savez(path, arrays, force_zip64=force_zip64)
  assert size == os.path.getsize(path)
  _check(path, arrays)
  # multi-chunk members: chunk sizes that divide nothing
  W.write_npz(path, (_chunked(k, a, (1, 7, 64, 1000)) for k, a in arrays.items()), force_zip64=force_zip64)
  _check(path, arrays)
  raw = open(path, 'rb').read()
  assert (b'PK\x06\x06' in raw) == force_zip64 and (b'PK\x06\x07' in raw) == force_zip64


def test_the_header_is_what_numpy_writes(tmp_path):
  for a in _arrays().values():
    np.save(str(tmp_path / 'x.npy'), a)
    raw = open(str(tmp_path / 'x.npy'), 'rb').read()
    header = W.npy_header(a.shape, a.dtype)
    assert raw == header + a.tobytes()


def test_same_members_and_arrays_as_savez(tmp_path):
  arrays = _arrays()
  ours, theirs = str(tmp_path / 'ours.npz'), str(tmp_path / 'theirs.npz')
  W.savez(ours, arrays)
  np.savez(theirs, **arrays)
  with zipfile.ZipFile(ours) as a, zipfile.ZipFile(theirs) as b:
    assert a.namelist() == b.namelist()
    for name in a.namelist():
      assert a.read(name) == b.read(name), name
      assert a.getinfo(name).CRC == b.getinfo(name).CRC
  with np.load(ours) as a, np.load(theirs) as b:
    assert a.files == b.files
    for k in a.files:
      assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])


@pytest.mark.parametrize('force_zip64', [False, True])
def test_a_wrong_crc_is_rejected_by_np_load(tmp_path, force_zip64):
  arrays = _arrays()
  path = str(tmp_path / 'bad.npz')
  key = 'generator/conv/kernel'

  def members():
    for k, a in arrays.items():
      name, header, chunks, crc = W.array_member(k, a)
      yield name, header, chunks, crc ^ (1 << 9 if k == key else 0)   # one stored bit flipped
  W.write_npz(path, members(), force_zip64=force_zip64)
  with np.load(path) as f:
    assert np.array_equal(f['odd'], arrays['odd'])   # the other members are intact
    with pytest.raises(zipfile.BadZipFile, match='CRC'):
      f[key]


def test_a_failure_in_the_middle_leaves_nothing(tmp_path):
  arrays = _arrays()
  path = str(tmp_path / 'c.npz')

  def members(fail):
    for i, (k, a) in enumerate(arrays.items()):
      if i == 3 and fail == 'raise':
        raise OSError('no space left on device')
      name, header, chunks, crc = W.array_member(k, a)
      if i == 4 and fail == 'short':   # one byte too few
        chunks = (a.tobytes()[:-1],)
      yield name, header, chunks, crc

  with pytest.raises(OSError, match='no space'):
    W.write_npz(path, members('raise'))
  assert os.listdir(str(tmp_path)) == []           # no <path>, no <path>.tmp
  with pytest.raises(ValueError, match='bytes handed over'):
    W.write_npz(path, members('short'))
  assert os.listdir(str(tmp_path)) == []
  # over an existing file: the old one stays whole, never a partial new one
  W.savez(path, {'old': np.arange(3)})
  with pytest.raises(OSError):
    W.write_npz(path, members('raise'))
  assert os.listdir(str(tmp_path)) == ['c.npz']
  with np.load(path) as f:
    assert f.files == ['old']
  with pytest.raises(OSError):   # a directory that is not there
    W.savez(str(tmp_path / 'nowhere' / 'd.npz'), arrays)
