"""utils/tf_records.py on the host: record framing, tf.train.Example, TensorProto and the
FixedLenFeature handling, against hand-assembled byte literals and writer -> reader round trips;
then the datasets' `_parse` and `get_file_patterns` over synthetic records."""
import struct

import numpy as np
import pytest

import _png_ref
from _records import image_record, video_record
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.utils import png, tf_records
from se3ds_amd.utils.tf_bundle import crc32c, mask_crc, unmask_crc
from se3ds_amd.utils.tf_records import FixedLenFeature

# The one-record file holding the payload b'abc', every byte written out and the two checksum words
# worked by hand from the specification (record_writer.h, crc32c.h), not through mask_crc / crc32c:
#   mask(crc) = ((crc >> 15) | (crc << 17)) + 0xa282ead8 mod 2^32, stored little-endian
#   length    03 00 00 00 00 00 00 00
#   CRC-32C of those eight bytes = 0x576c35e3 (bit by bit, reflected polynomial 0x82f63b78)
#             >> 15 = 0x0000aed8, << 17 = 0x6bc60000, rotated 0x6bc6aed8,
#             + 0xa282ead8 = 0x1_0e4999b0 -> 0x0e4999b0 -> b0 99 49 0e
#   payload   61 62 63
#   CRC-32C('abc') = 0x364b3fb7 (a published check value)
#             >> 15 = 0x00006c96, << 17 = 0x7f6e0000, rotated 0x7f6e6c96,
#             + 0xa282ead8 = 0x1_21f1576e -> 0x21f1576e -> 6e 57 f1 21
ONE_RECORD = bytes.fromhex('0300000000000000' 'b099490e' '616263' '6e57f121')


# --------------------------------------------------------------------------------- records
def test_record_framing_round_trip(tmp_path):
  path = str(tmp_path / 'a.tfrecord')
  recs = [b'', b'x', bytes(range(256)) * 5, b'last']
  tf_records.write_records(path, recs)
  assert list(tf_records.read_records(path)) == recs
  assert list(tf_records.read_records(path, verify=False)) == recs


def test_hand_assembled_record(tmp_path):
  assert len(ONE_RECORD) == 19
  # the pieces of the literal, one by one: the CRC, the masking and its inverse
  assert crc32c(b'abc') == 0x364b3fb7 and crc32c(ONE_RECORD[:8]) == 0x576c35e3
  assert mask_crc(0x364b3fb7) == 0x21f1576e and mask_crc(0x576c35e3) == 0x0e4999b0
  assert unmask_crc(0x21f1576e) == 0x364b3fb7 and unmask_crc(0x0e4999b0) == 0x576c35e3
  path = tmp_path / 'one.tfrecord'
  path.write_bytes(ONE_RECORD)
  assert list(tf_records.read_records(str(path))) == [b'abc']
  tf_records.write_records(str(tmp_path / 'w.tfrecord'), [b'abc'])
  assert (tmp_path / 'w.tfrecord').read_bytes() == ONE_RECORD


def _flipped(data: bytes, byte: int) -> bytes:
  return data[:byte] + bytes([data[byte] ^ 0x10]) + data[byte + 1:]


def test_flipped_payload_and_length_bits_raise(tmp_path):
  path = tmp_path / 'bad.tfrecord'
  path.write_bytes(_flipped(ONE_RECORD, 13))   # a payload byte
  with pytest.raises(ValueError, match='bad.tfrecord.*offset 0'):
    list(tf_records.read_records(str(path)))
  assert list(tf_records.read_records(str(path), verify=False)) == [b'a' + bytes([ord('b') ^ 0x10]) + b'c']
  path.write_bytes(_flipped(ONE_RECORD, 0))    # a length byte: 3 -> 19
  with pytest.raises(ValueError, match='bad.tfrecord.*offset 0'):
    list(tf_records.read_records(str(path)))
  with pytest.raises(ValueError, match='truncated'):   # without the CRC the length runs off the end
    list(tf_records.read_records(str(path), verify=False))


@pytest.mark.parametrize('cut', [1, 4, 5, 12, 15])
def test_truncated_tail_raises(tmp_path, cut):
  path = tmp_path / 't.tfrecord'
  path.write_bytes(ONE_RECORD + ONE_RECORD[:-cut])
  it = tf_records.read_records(str(path))
  assert next(it) == b'abc'
  with pytest.raises(ValueError, match=f't.tfrecord.*offset {len(ONE_RECORD)}'):
    next(it)


# --------------------------------------------------------------------------------- Example
KNOWN = bytes.fromhex('0a0c0a0a0a016112051a030a0101')


def test_example_known_answer():
  assert tf_records.encode_example({'a': np.array([1], np.int64)}) == KNOWN
  got = tf_records.parse_example(KNOWN)
  assert list(got) == ['a'] and got['a'].dtype == np.int64 and got['a'].tolist() == [1]


def test_example_packed_and_unpacked_lists():
  # Example{features{ entry 'i': int64_list unpacked 3, 300 ; entry 'f': float_list unpacked 1.5, -2 }}
  i_unpacked = bytes.fromhex('0803') + bytes.fromhex('08ac02')
  f_unpacked = b'\x0d' + struct.pack('<f', 1.5) + b'\x0d' + struct.pack('<f', -2.0)
  def entry(key, feature_field, body):
    feat = bytes([feature_field << 3 | 2, len(body)]) + body
    kv = b'\x0a' + bytes([len(key)]) + key + b'\x12' + bytes([len(feat)]) + feat
    return b'\x0a' + bytes([len(kv)]) + kv
  feats = entry(b'i', 3, i_unpacked) + entry(b'f', 2, f_unpacked)
  got = tf_records.parse_example(b'\x0a' + bytes([len(feats)]) + feats)
  assert got['i'].tolist() == [3, 300] and got['i'].dtype == np.int64
  assert got['f'].tolist() == [1.5, -2.0] and got['f'].dtype == np.float32
  packed = tf_records.parse_example(tf_records.encode_example(
      {'i': np.array([3, 300]), 'f': np.array([1.5, -2.0], np.float32)}))
  assert packed['i'].tolist() == [3, 300] and packed['f'].tolist() == [1.5, -2.0]


def test_example_negative_int64_and_bytes_list():
  buf = tf_records.encode_example({'n': np.array([-1, -2 ** 63, 2 ** 63 - 1, 0]),
                                   'b': [b'', b'one', bytes(range(200))], 's': 'text'})
  # -1 is ten bytes of varint: ff x 9, 01
  assert b'\xff' * 9 + b'\x01' in buf
  got = tf_records.parse_example(buf)
  assert got['n'].tolist() == [-1, -2 ** 63, 2 ** 63 - 1, 0]
  assert got['b'] == [b'', b'one', bytes(range(200))] and got['s'] == [b'text']
  assert list(got) == ['n', 'b', 's']


def test_apply_features_defaults_and_shape_errors():
  spec = {'name': FixedLenFeature([], 'string', ''), 'k': FixedLenFeature([], 'int64', 7),
          'scale': FixedLenFeature([], 'float32', 10.0),
          'bbox': FixedLenFeature([4], 'float32', [0.0, 0.0, 0.0, 0.0]),
          'grid': FixedLenFeature([2, 2], 'int64', [1, 2, 3, 4])}
  out = tf_records.apply_features({}, spec)
  assert out['name'] == b'' and out['k'] == 7 and isinstance(out['k'], int)
  assert out['scale'] == np.float32(10.0) and isinstance(out['scale'], np.float32)
  assert out['bbox'].tolist() == [0.0] * 4 and out['bbox'].dtype == np.float32
  assert out['grid'].tolist() == [[1, 2], [3, 4]]
  parsed = tf_records.parse_example(tf_records.encode_example(
      {'name': b'n', 'k': [-3], 'scale': [2.5], 'bbox': [1.0, 2.0, 3.0, 4.0], 'other': [1]}))
  out = tf_records.apply_features(parsed, spec)
  assert out['name'] == b'n' and out['k'] == -3 and out['scale'] == np.float32(2.5)
  assert out['bbox'].tolist() == [1.0, 2.0, 3.0, 4.0] and 'other' not in out
  # a present feature with an empty list counts as missing, as in tf.io.parse_single_example
  empty = tf_records.parse_example(bytes.fromhex('0a10' '0a07' '0a016b' '1202' '1a00' '0a05' '0a0162' '1200'))
  assert empty['k'].tolist() == [] and 'b' not in empty
  assert tf_records.apply_features(empty, spec)['k'] == 7
  assert tf_records.apply_features({'name': [], 'bbox': np.zeros(0, np.float32)}, spec)['name'] == b''
  with pytest.raises(ValueError, match='required'):
    tf_records.apply_features(empty, {'k': FixedLenFeature([], 'int64')})
  with pytest.raises(ValueError, match='required'):
    tf_records.apply_features({}, {'need': FixedLenFeature([], 'int64')})
  with pytest.raises(ValueError, match='bbox'):
    tf_records.apply_features({'bbox': np.zeros(3, np.float32)}, spec)
  with pytest.raises(ValueError, match='k'):
    tf_records.apply_features({'k': np.array([1, 2])}, spec)
  with pytest.raises(ValueError, match='scale'):   # an int64 list where float32 is declared
    tf_records.apply_features({'scale': np.array([1])}, spec)
  with pytest.raises(ValueError, match='name'):
    tf_records.apply_features({'name': [b'a', b'b']}, spec)


# ----------------------------------------------------------------------------- TensorProto
@pytest.mark.parametrize('dtype', [np.float32, np.int32, np.uint8, np.int64])
def test_tensor_round_trip(dtype):
  rng = np.random.default_rng(3)
  a = rng.integers(0, 200, (3, 5)).astype(dtype)
  back = tf_records.parse_tensor(tf_records.serialize_tensor(a), dtype)
  assert back.dtype == dtype and back.shape == (3, 5) and (back == a).all()


def test_tensor_ranks_and_literal():
  scalar = tf_records.parse_tensor(tf_records.serialize_tensor(np.float32(2.5)), np.float32)
  assert scalar.shape == () and scalar == np.float32(2.5)
  a = np.arange(2 * 1 * 3 * 2 * 2, dtype=np.int32).reshape(2, 1, 3, 2, 2)
  back = tf_records.parse_tensor(tf_records.serialize_tensor(a), np.int32)
  assert back.shape == a.shape and (back == a).all()
  # uint8 [2] = 7, 9 by hand: dtype 4; shape{dim{size 2}}; tensor_content
  lit = bytes.fromhex('0804' '1204' '1202' '0802' '2202' '0709')
  assert tf_records.serialize_tensor(np.array([7, 9], np.uint8)) == lit
  assert tf_records.parse_tensor(lit, np.uint8).tolist() == [7, 9]
  with pytest.raises(ValueError):
    tf_records.parse_tensor(bytes.fromhex('0804' '1204' '1202' '0803' '2202' '0709'), np.uint8)


def test_tensor_not_implemented_cases():
  # float_val (field 5) instead of tensor_content
  with pytest.raises(NotImplementedError, match='float_val'):
    tf_records.parse_tensor(bytes.fromhex('0801' '1200' '2a04') + struct.pack('<f', 1.0), np.float32)
  with pytest.raises(NotImplementedError, match='int_val'):
    tf_records.parse_tensor(bytes.fromhex('0803' '1200' '3801'), np.int32)
  with pytest.raises(NotImplementedError, match='dtype code 2'):   # DT_DOUBLE
    tf_records.parse_tensor(bytes.fromhex('0802' '1200' '2208') + bytes(8), np.float64)
  with pytest.raises(NotImplementedError, match='asked for'):
    tf_records.parse_tensor(tf_records.serialize_tensor(np.zeros(2, np.int32)), np.uint8)
  with pytest.raises(NotImplementedError):
    tf_records.serialize_tensor(np.zeros(2, np.float64))


# ---------------------------------------------------------------------- datasets on the host
def test_image_parse_keys_defaults_and_errors():
  rng = np.random.default_rng(11)
  ds = indoor_datasets.R2RImageDataset(image_size=4, preprocessed_image_height=8)
  rec, pix = image_record(8, rng)
  out = ds._parse(rec)
  assert set(out) == set(indoor_datasets.RAW_DTYPES) | {'dataset_type', 'depth_scale', 'bbox'}
  assert out['depth_scale'] == np.float32(10.0) and out['dataset_type'] == 0
  assert out['bbox'].tolist() == [0.0] * 4
  for name, (_, channels, depth) in indoor_datasets.IMAGE_PLANES.items():
    p = out[name]
    assert isinstance(p, png.PngPlane)
    assert (p.height, p.width, p.channels, p.bit_depth) == (8, 16, channels, depth)
    want = pix[name]
    assert (_png_ref.decode_png(p.filtered, 8, 16, depth, channels) == want).all()
  rec, _ = image_record(8, rng, depth_scale=np.array([20.0], np.float32), scan_id=b'scan',
                        **{'image/filename': b'f.png', 'bbox': np.array([1, 2, 3, 4], np.float32)})
  out = indoor_datasets.R2RImageDataset(image_size=4, preprocessed_image_height=8,
                                        return_filename=True)._parse(rec)
  assert out['depth_scale'] == np.float32(20.0) and out['bbox'].tolist() == [1.0, 2.0, 3.0, 4.0]
  assert out['filename'] == b'f.png' and out['scan_id'] == b'scan'
  # geometry: a record preprocessed to another height
  with pytest.raises(ValueError, match='8x16'):
    indoor_datasets.R2RImageDataset(image_size=4, preprocessed_image_height=4)._parse(rec)
  # a missing plane is the default '' and no PNG
  rec, _ = image_record(8, rng, **{'proj/mask': b''})
  with pytest.raises(ValueError, match='proj/mask'):
    ds._parse(rec)
  rec, _ = image_record(8, rng, dataset_type=np.array([2]))
  with pytest.raises(NotImplementedError, match='RE10K'):
    ds._parse(rec)


def test_image_file_patterns():
  ds = indoor_datasets.R2RImageDataset(data_dir='data/train/')
  assert ds.get_file_patterns('train') == 'data/train/train*.tfrecord'
  assert indoor_datasets.R2RImageDataset(data_dir='d').get_file_patterns('val_seen') == 'd/val_seen*.tfrecord'
  assert ds.get_file_patterns('train', 'x/*.rec') == 'x/*.rec'
  for bad in ('validation', None):
    with pytest.raises(ValueError) as e:
      ds.get_file_patterns(bad)
    assert str(e.value) == f"Expected split to be one of ['train', 'val'], got {bad}"


def test_video_parse(tmp_path):
  rng = np.random.default_rng(12)
  ds = indoor_datasets.R2RVideoDataset(image_size=2, preprocessed_image_height=4)
  rec, arrays = video_record(4, rng)
  old, old_arrays = video_record(4, rng, pathdreamer=False)
  tf_records.write_records(str(tmp_path / 'val_seen-0.tfrecord'), [rec, old])
  ds.data_dir = str(tmp_path) + '/'
  examples = ds.examples_from_tfrecords('val_seen')
  for _ in range(2):   # a fresh iterator per call
    got = list(examples())
    assert len(got) == 2
    for g, want in zip(got, (arrays, old_arrays)):
      assert set(g) == set(want)
      for k in want:
        assert np.asarray(g[k]).dtype == np.asarray(want[k]).dtype, k
        assert (np.asarray(g[k]) == want[k]).all(), k
  for k, dt in indoor_datasets.VIDEO_PLANES.items():
    assert str(got[0][k].dtype) == str(dt).replace('torch.', '')
  assert not set(indoor_datasets.VIDEO_OPTIONAL) & set(got[1])
  # the record checksum is a Python byte loop: off by default on the dataset path, on by request
  data = bytearray((tmp_path / 'val_seen-0.tfrecord').read_bytes())
  data[-1] ^= 0x01   # the last record's payload CRC word
  (tmp_path / 'val_seen-0.tfrecord').write_bytes(bytes(data))
  assert len(list(ds.examples_from_tfrecords('val_seen')())) == 2
  with pytest.raises(ValueError, match='payload checksum'):
    list(ds.examples_from_tfrecords('val_seen', verify_crc=True)())
  with pytest.raises(ValueError, match='video/rgb'):
    indoor_datasets.R2RVideoDataset(image_size=2, preprocessed_image_height=8)._parse(rec)
  with pytest.raises(ValueError, match='num_frames'):
    ds._parse(tf_records.encode_example({'id': [1]}))
  with pytest.raises(ValueError, match='No data files'):
    ds.examples_from_tfrecords('train')
