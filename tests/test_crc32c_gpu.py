"""The device CRC-32C (csrc/crc32c.hip, utils/crc32c.py) and its consumers on an MI355X.  Every
comparison is exact equality.  The yardstick is `tf_bundle.crc32c`, the host byte loop that
tests/test_tf_bundle.py pins to RFC 3720; the references of the sweep are computed once per module.

In the consumer tests the host loop is patched to raise on any input above 64 bytes, so a
`'device'` that merely counted as truthy and went through the loop fails.  The blocks of a bundle's
index file are exempt from the patch: they stay on the host by design (a few KB), and without them
no bundle can be written or opened at all."""
import sys

import numpy as np
import pytest
import torch

from _records import image_record, video_record
from se3ds_amd import _lib
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.utils import crc32c as C
from se3ds_amd.utils import tf_bundle, tf_records

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
HOST = tf_bundle.crc32c   # the yardstick, bound before any test patches the module attribute


def _block():
  return _lib.lib().se3ds_crc32c_block_bytes()


def _lengths():
  b = _block()
  return (list(range(10)) + [15, 16, 17, 63, 64, 65, 255, 256, 257] +
          [b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1, 3 * b + 5])


def _layout(aligns):
  """Disjoint ranges: every length of the sweep at every start alignment (mod 16) of `aligns`, a gap
  of at least one byte between neighbours.  -> (offsets, lengths, buffer size)"""
  offs, lens, pos = [], [], 0
  for n in _lengths():
    for a in aligns:
      pos = (pos + 1 + 15) // 16 * 16 + a
      offs.append(pos)
      lens.append(n)
      pos += n
  return offs, lens, pos + 3


def _device(data, offs, lens):
  return C.crc32c_device(torch.from_numpy(np.array(data, dtype=np.uint8)).to(DEV), offs, lens).tolist()


@pytest.fixture(scope='module')
def sweep():
  """Random bytes, the full length x alignment layout and the host CRC of every range (about 3 MB
  through the Python loop, once)."""
  offs, lens, size = _layout(range(16))
  data = np.random.default_rng(7).integers(0, 256, size, dtype=np.uint8)
  raw = data.tobytes()
  want = [HOST(raw[o:o + n]) for o, n in zip(offs, lens)]
  return data, offs, lens, want


def test_block_size_contract():
  b = _block()
  assert 0 < b <= 1 << 20
  assert _lib.lib().se3ds_crc32c_fields() == 2


def test_known_answers_on_the_device():
  vectors = [(b'123456789', 0xE3069283), (bytes(32), 0x8A9136AA), (b'\xff' * 32, 0x62A8AB43),
             (bytes(range(32)), 0x46DD794E), (bytes(range(31, -1, -1)), 0x113FDB5C), (b'abc', 0x364b3fb7)]
  blob = b''.join(v for v, _ in vectors)
  offs = np.cumsum([0] + [len(v) for v, _ in vectors[:-1]]).tolist()
  got = _device(np.frombuffer(blob, np.uint8), offs, [len(v) for v, _ in vectors])
  assert got == [c for _, c in vectors]
  for v, c in vectors:
    assert HOST(v) == c
  assert C.crc32c_host_slabs([v for v, _ in vectors]).tolist() == [c for _, c in vectors]


def test_length_and_alignment_sweep(sweep):
  data, offs, lens, want = sweep
  got = _device(data, offs, lens)
  bad = [(o % 16, n, hex(g), hex(w)) for o, n, g, w in zip(offs, lens, got, want) if g != w]
  assert not bad, bad[:8]
  assert sorted({o % 16 for o in offs}) == list(range(16))
  assert got[lens.index(0)] == 0


def test_constant_data_isolates_the_length_term():
  """All-zero and all-0xff data at the same lengths (the CRC depends on the length alone, so a wrong
  x^(8 L) shows), and random data behind a long run of zeros.  The references of the constant fills
  are continued from one length to the next, which keeps the host loop short."""
  aligns = (0, 5, 11)
  offs, lens, size = _layout(aligns)
  for fill in (0, 255):
    want, crc, done = {}, 0, 0
    for n in sorted(set(lens)):
      crc = HOST(bytes([fill]) * (n - done), crc)
      want[n], done = crc, n
    got = _device(np.full(size, fill, np.uint8), offs, lens)
    assert got == [want[n] for n in lens], fill
  data = np.random.default_rng(8).integers(0, 256, size, dtype=np.uint8)
  for o, n in zip(offs, lens):
    data[o:o + (3 * n) // 4] = 0
  raw = data.tobytes()
  want, crc_of_zeros = [], {}
  for o, n in zip(offs, lens):   # zeros depend on their count alone; the tail continues from there
    z = (3 * n) // 4
    if z not in crc_of_zeros:
      crc_of_zeros[z] = HOST(bytes(z))
    want.append(HOST(raw[o + z:o + n], crc_of_zeros[z]))
  assert _device(data, offs, lens) == want


def test_isolation(sweep):
  data, offs, lens, want = sweep
  inside = np.zeros(data.size, bool)
  for o, n in zip(offs, lens):
    inside[o:o + n] = True
  other = data.copy()
  other[~inside] ^= 0xff                     # differs in every byte outside the ranges
  assert (~inside).sum() >= len(offs)
  assert _device(other, offs, lens) == want
  for k in (lens.index(1), lens.index(257) + 3, len(lens) - 1, lens.index(_block()) + 9):
    flipped = data.copy()
    flipped[offs[k] + lens[k] // 2] ^= 0x04
    got = _device(flipped, offs, lens)
    assert got[k] != want[k]
    assert got[:k] == want[:k] and got[k + 1:] == want[k + 1:]


def test_mixed_launch_and_overlap():
  b = _block()
  rng = np.random.default_rng(9)
  size = 3 * b + 5 + 40000
  data = rng.integers(0, 256, size, dtype=np.uint8)
  raw = data.tobytes()
  offs, lens = [], []
  for i in range(300):
    n = int(rng.integers(0, 2001))
    offs.append(int(rng.integers(0, size - n + 1)))
    lens.append(n)
    if i % 2:
      offs.append(int(rng.integers(0, size - 8)))
      lens.append(8)
    if i == 150:
      offs.append(17)
      lens.append(3 * b + 5)
  # a range and its two halves
  o, n, h = 1001, 2 * b + 77, b + 13
  offs += [o, o, o + h]
  lens += [n, h, n - h]
  got = _device(data, offs, lens)
  want = [HOST(raw[a:a + m]) for a, m in zip(offs, lens)]
  assert got == want
  whole, first, second = got[-3:]
  assert HOST(raw[o + h:o + n], first) == whole and second == want[-1]


@pytest.mark.parametrize('size', [4 * 300 + 1, 4 * 300 + 2, 4 * 300 + 3, 13, 16 * 70 + 13, 16 * 2048 + 13])
def test_buffer_end(size):
  """Buffers of 1, 2, 3 mod 4 and of 13 mod 16 bytes, the last beyond two blocks: ranges that end on
  the last byte and ranges that start at byte 0 -- a 4- or 16-byte load past the range would leave
  the buffer."""
  data = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
  raw = data.tobytes()
  offs = [0, 0, size - 1, size // 2, 3, 0, size - 7]
  lens = [size, size - 1, 1, size - size // 2, size - 3, 5, 7]
  assert _device(data, offs, lens) == [HOST(raw[o:o + n]) for o, n in zip(offs, lens)]


def test_validation_launches_nothing():
  L = _lib.lib()
  buf = torch.arange(100, dtype=torch.uint8, device=DEV)
  crc = torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
  ws_bytes = int(L.se3ds_crc32c_workspace_bytes(200, 2))
  ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=DEV)
  stream = torch.cuda.current_stream().cuda_stream

  def call(table, n=2, buf_p=buf.data_ptr(), table_p=True, host=True, crc_p=crc.data_ptr(),
           ws_p=ws.data_ptr(), ws_n=ws_bytes):
    t = np.asarray(table, np.int64).reshape(-1, 2)
    td = torch.from_numpy(t).to(DEV)
    rc = L.se3ds_crc32c_multi(buf_p, 100, td.data_ptr() if table_p else None,
                              t.ctypes.data if host else None, n, crc_p, ws_p if ws_p else None, ws_n, stream)
    torch.cuda.synchronize()
    return rc

  good = [[0, 100], [99, 1]]
  cases = [call(good, n=0), call(good, buf_p=None), call(good, table_p=False), call(good, host=False),
           call(good, crc_p=None), call(good, ws_p=0), call([[-1, 4], [0, 0]]), call([[0, 0], [4, -1]]),
           call([[0, 101], [0, 0]]), call([[0, 0], [100, 1]]), call(good, ws_n=ws_bytes - 1)]
  assert cases == [-1] * len(cases)
  assert crc.tolist() == [0x5a5a5a5a] * 2 and not ws.any()
  assert call(good) == 0
  raw = bytes(range(100))
  assert (crc.cpu().numpy().view(np.uint32)).tolist() == [HOST(raw), HOST(raw[99:])]
  with pytest.raises(_lib.Se3dsHipError, match='BADSHAPE'):
    C.crc32c_device(buf, [50], [51])
  assert C.crc32c_device(buf, [], []).shape == (0,)
  assert C.crc32c_device(buf[:0], [0, 0], [0, 0]).tolist() == [0, 0]


def test_host_slabs_across_slab_boundaries():
  rng = np.random.default_rng(10)
  items = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (10, 500, 0, 7, 3, 90, 90)]
  items.append(np.arange(9, dtype='<f4'))
  want = [HOST(bytes(x) if isinstance(x, bytes) else x.tobytes()) for x in items]
  for slab in (100, 64, 1 << 20):
    assert C.crc32c_host_slabs(items, slab_bytes=slab).tolist() == want
  assert C.crc32c_host_slabs([]).shape == (0,)


# --------------------------------------------------------------------------------- consumers
def _forbid_host_loop(monkeypatch):
  """tf_bundle.crc32c raises on more than 64 bytes -- except for the blocks of an index file."""
  def guarded(data, crc=0):
    if len(data) > 64 and sys._getframe(1).f_code.co_name not in ('add_block', 'block'):
      raise AssertionError(f'{len(data)} bytes went through the Python CRC-32C loop')
    return HOST(data, crc)
  monkeypatch.setattr(tf_bundle, 'crc32c', guarded)
  monkeypatch.setattr(tf_records, 'crc32c', guarded)


def _collect(it):
  got = []
  try:
    for x in it:
      got.append(x)
  except ValueError as e:
    return got, str(e)
  return got, None


def test_read_records_on_the_device(tmp_path, monkeypatch):
  rng = np.random.default_rng(11)
  payloads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (300, 0, 70000, 65, 1, 4000, 129)]
  path = str(tmp_path / 'a.tfrecord')
  tf_records.write_records(path, payloads)
  good = open(path, 'rb').read()
  starts = np.cumsum([0] + [16 + len(p) for p in payloads]).tolist()
  # what the host path says about each damaged file, before the loop is forbidden
  damaged = {}
  for name, k, at in (('payload', 4, 12 + 1), ('payload-crc', 2, 12 + 70000 + 2), ('length-crc', 3, 9),
                      ('length', 5, 0), ('length-high', 2, 6), ('payload-first', 0, 12 + 299)):
    data = bytearray(good)
    data[starts[k] + at] ^= 0x01 if name != 'length-high' else 0x40
    p = str(tmp_path / f'{name}.tfrecord')
    open(p, 'wb').write(bytes(data))
    damaged[name] = (p, k) + _collect(tf_records.read_records(p, verify=True))
  truncated = str(tmp_path / 'cut.tfrecord')
  open(truncated, 'wb').write(good[:starts[3] + 30])
  cut = _collect(tf_records.read_records(truncated, verify=True))
  _forbid_host_loop(monkeypatch)
  with pytest.raises(AssertionError, match='Python CRC-32C loop'):
    list(tf_records.read_records(path, verify=True))
  for batch in (64 << 20, 100, 1):
    assert list(tf_records.read_records(path, verify='device', device_batch_bytes=batch)) == payloads
    for name, (p, k, host_got, host_err) in damaged.items():
      got, err = _collect(tf_records.read_records(p, verify='device', device_batch_bytes=batch))
      assert host_err is not None and f'offset {starts[k]}' in host_err, name
      assert err == host_err and got == host_got == payloads[:k], (name, batch)
    assert _collect(tf_records.read_records(truncated, verify='device', device_batch_bytes=batch)) == cut
  assert cut[1] is not None and 'truncated record' in cut[1] and len(cut[0]) == 3
  assert 'length checksum mismatch' in damaged['length'][3] and 'length checksum' in damaged['length-crc'][3]
  assert 'payload checksum mismatch' in damaged['payload'][3]


def test_dataset_entry_points_accept_device(tmp_path, monkeypatch):
  rng = np.random.default_rng(12)
  made = [image_record(8, rng, depth_scale=np.array([10.0 + i], np.float32)) for i in range(2)]
  (tmp_path / 'img').mkdir()
  tf_records.write_records(str(tmp_path / 'img' / 'train-00000.tfrecord'), [m[0] for m in made])
  vpath = str(tmp_path / 'val_unseen-0.tfrecord')
  tf_records.write_records(vpath, [video_record(4, rng)[0], video_record(4, rng)[0]])
  _forbid_host_loop(monkeypatch)
  ds = indoor_datasets.R2RImageDataset(image_size=4, preprocessed_image_height=8, data_dir=str(tmp_path / 'img'))
  kw = dict(batch_size=2, seed=5, num_epochs=1, device=DEV)
  plain, checked = list(ds.input_fn('train', **kw)), list(ds.input_fn('train', verify_crc='device', **kw))
  assert len(plain) == len(checked) == 1 and set(plain[0]) == set(checked[0])
  for k, v in plain[0].items():
    assert torch.equal(checked[0][k], v), k
  with pytest.raises(AssertionError, match='Python CRC-32C loop'):
    list(ds.input_fn('train', verify_crc=True, **kw))
  vds = indoor_datasets.R2RVideoDataset(image_size=2, preprocessed_image_height=4)
  a = list(vds.examples_from_tfrecords(file_pattern=vpath)())
  b = list(vds.examples_from_tfrecords(file_pattern=vpath, verify_crc='device')())
  assert len(a) == len(b) == 2
  for x, y in zip(a, b):
    assert set(x) == set(y)
    for k in x:
      assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
  data = bytearray(open(vpath, 'rb').read())
  data[len(data) // 4] ^= 0x20
  open(vpath, 'wb').write(bytes(data))
  with pytest.raises(ValueError, match='payload checksum mismatch at offset'):
    list(vds.examples_from_tfrecords(file_pattern=vpath, verify_crc='device')())


def _state():
  rng = np.random.default_rng(13)
  return {'a/flag': np.array([True, False, True]),                       # 3 bytes: later offsets are odd
          'b/bytes': rng.integers(0, 256, (5, 12), dtype=np.uint8),
          'c/w': rng.standard_normal((33, 7)).astype(np.float32),
          'd/i64': rng.integers(-2 ** 60, 2 ** 60, 40),
          'e/f64': rng.standard_normal(50),
          'f/f16': rng.standard_normal((9, 11)).astype(np.float16),
          'g/i32': rng.integers(-2 ** 30, 2 ** 30, 5000).astype(np.int32),
          'h/scalar': np.float32(2.5),
          'i/empty': np.zeros((0, 4), np.float32),
          'j/u16': rng.integers(0, 65536, 77).astype(np.uint16)}


def test_bundle_checksums_on_the_device(tmp_path, monkeypatch):
  state = _state()
  host, dev, none = (str(tmp_path / n) for n in ('host', 'dev', 'none'))
  tf_bundle.write_bundle(host, state, checksums=True)
  tf_bundle.write_bundle(none, state, checksums=False)
  _forbid_host_loop(monkeypatch)
  with pytest.raises(AssertionError, match='Python CRC-32C loop'):
    tf_bundle.write_bundle(dev, state, checksums=True)
  tf_bundle.write_bundle(dev, state, checksums='device')
  for ext in ('.index', '.data-00000-of-00001'):
    assert open(dev + ext, 'rb').read() == open(host + ext, 'rb').read(), ext
  with pytest.raises(AssertionError, match='Python CRC-32C loop'):
    tf_bundle.read_bundle(dev, verify=True)
  got = tf_bundle.read_bundle(dev, verify='device')
  assert set(got) == set(state)
  for k, v in state.items():
    assert got[k].dtype == np.asarray(v).dtype and np.array_equal(got[k], v), k
  # a flipped data byte names its tensor; of two damaged tensors the first in key order
  sizes = [np.asarray(state[k]).nbytes for k in sorted(state)]
  starts = dict(zip(sorted(state), np.cumsum([0] + sizes[:-1]).tolist()))
  assert starts['c/w'] % 2 == 1
  shard = dev + '.data-00000-of-00001'
  sound = open(shard, 'rb').read()
  for names in (('g/i32',), ('j/u16', 'c/w'), ('a/flag',)):
    data = bytearray(sound)
    for name in names:
      data[starts[name] + 1] ^= 0x80
    open(shard, 'wb').write(bytes(data))
    with pytest.raises(ValueError) as e:
      tf_bundle.read_bundle(dev, verify='device')
    assert str(e.value) == f'{min(names)}: tensor checksum mismatch'
    assert set(tf_bundle.read_bundle(dev, verify='device', keys=['e/f64'])) == {'e/f64'}   # not among the read
  # entries whose stored CRC is 0 are skipped
  data = bytearray(open(none + '.data-00000-of-00001', 'rb').read())
  data[starts['g/i32']] ^= 1
  open(none + '.data-00000-of-00001', 'wb').write(bytes(data))
  assert set(tf_bundle.read_bundle(none, verify='device')) == set(state)


@pytest.fixture(scope='module')
def generator_files(tmp_path_factory):
  """The smallest test generator (model_config.get_test_config, 4.5 MB of fp32) on the device and
  what save_generator writes for it today: default arguments, CRCs by the host loop."""
  from se3ds_amd.models import image_models, model_config
  c = model_config.get_test_config()
  make = lambda seed: image_models.ResNetGenerator(resnet_version=c.resnet_version, gen_dims=c.gen_dims,
                                                   use_blurred_mask=c.use_blurred_mask, device=DEV, seed=seed)
  G = make(3)
  prefix = str(tmp_path_factory.mktemp('gen') / 'today')
  tf_bundle.save_generator(G, prefix)
  return G, make, prefix


def test_generator_checksums_from_the_arena(generator_files, tmp_path, monkeypatch):
  G, make, today = generator_files
  entries = [tf_bundle._decode_entry(v) for k, v in tf_bundle._read_table(today + '.index') if k]
  assert len(entries) > 100 and all(e[5] != 0 for e in entries)   # the 64 MB rule: all set
  _forbid_host_loop(monkeypatch)
  with pytest.raises(AssertionError, match='Python CRC-32C loop'):
    tf_bundle.save_generator(G, str(tmp_path / 'x'), checksums=True)
  # every tensor lies in the arena as the file's bytes: nothing may be uploaded
  def no_upload(*a, **k):
    raise AssertionError('save_generator uploaded a tensor that lies in the arena')
  with monkeypatch.context() as m:
    m.setattr(C, 'crc32c_host_slabs', no_upload)
    tf_bundle.save_generator(G, str(tmp_path / 'dev'), checksums='device')
  for ext in ('.index', '.data-00000-of-00001'):
    assert open(str(tmp_path / 'dev') + ext, 'rb').read() == open(today + ext, 'rb').read(), ext
  G2 = make(11)
  assert not torch.equal(G2.store.theta, G.store.theta)
  assert tf_bundle.load_generator(G2, str(tmp_path / 'dev'), verify='device') == []
  assert torch.equal(G2.store.theta, G.store.theta) and torch.equal(G2.store.state, G.store.state)
  # a tensor that is not in place goes through the slabs and gets the same value
  with monkeypatch.context() as m:
    m.setattr(tf_bundle, '_arena_checksums', lambda store, names: {})
    tf_bundle.save_generator(G, str(tmp_path / 'slabs'), checksums='device')
  assert open(str(tmp_path / 'slabs.index'), 'rb').read() == open(today + '.index', 'rb').read()
  # and a damaged shard does not load
  shard = str(tmp_path / 'dev.data-00000-of-00001')
  data = bytearray(open(shard, 'rb').read())
  data[len(data) // 2] ^= 0x01
  open(shard, 'wb').write(bytes(data))
  with pytest.raises(ValueError, match='tensor checksum mismatch'):
    tf_bundle.load_generator(make(12), str(tmp_path / 'dev'), verify='device')
