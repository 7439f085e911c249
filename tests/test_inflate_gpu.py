"""se3ds_png_inflate (csrc/inflate.hip) on the device: every stream of the corpus in
tests/_deflate_ref.py compared exactly with CPython's zlib.decompress, the malformed ones by status;
decode_png_batch(inflate='device') bit for bit against inflate='host' for every filter type,
bytes-per-pixel and geometry; both datasets from TFRecord files; the async form.  The corpus has
passed the sanitised host build of the same decoder (tests/test_inflate_cpu.py) -- the malformed
streams are bounds-handling cases, not meant to fault.

The issue's "HCLEN = 4" cannot be a good stream: with lengths for the code-length symbols 16, 17,
18 and 0 alone every literal/length length is zero.  It is here as a well-formed header that must
end NO_END_OF_BLOCK (zlib: "missing end-of-block"), next to HCLEN = 5, the shortest good one."""
import zlib

import numpy as np
import pytest
import torch

import _deflate_ref as D
import _png_ref
from _records import image_record, video_record
from se3ds_amd import _lib
from se3ds_amd.datasets import indoor_datasets
from se3ds_amd.utils import png, tf_records

DEV = torch.device('cuda:0')
pytestmark = pytest.mark.gpu


def _ring():
  return _lib.lib().se3ds_png_inflate_ring_bytes()


def inflate_streams(cases, misalign=0):
  """One launch over `cases` through the C entry -> (status words, inflated regions)."""
  L = _lib.lib()
  n = len(cases)
  table = np.zeros((n, L.se3ds_png_inflate_fields()), np.int64)
  offset = (table.nbytes + 15) & ~15
  ws = misalign
  for i, c in enumerate(cases):
    table[i] = (offset, len(c.stream), ws, c.expected_len, c.pitch)
    offset += (len(c.stream) + 15) & ~15
    ws += ((c.expected_len + 15) & ~15) + misalign
  host = np.zeros(offset, np.uint8)
  host[:table.nbytes] = table.reshape(-1).view(np.uint8)
  for row, c in zip(table, cases):
    host[row[0]:row[0] + row[1]] = np.frombuffer(c.stream, np.uint8)
  buf = torch.from_numpy(host).to(DEV)
  workspace = torch.full((ws + 16,), 0xA5, dtype=torch.uint8, device=DEV)
  status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
  rc = L.se3ds_png_inflate(buf.data_ptr(), offset, workspace.data_ptr(), workspace.numel(),
                           table.ctypes.data, n, status.data_ptr(), _lib.stream())
  _lib.check(rc, 'se3ds_png_inflate')
  out = workspace.cpu().numpy()
  return status.cpu().numpy(), [out[row[2]:row[2] + row[3]].tobytes() for row in table], out, table


@pytest.fixture(scope='module')
def good():
  return D.good_cases(_ring())


@pytest.fixture(scope='module')
def good_results(good):
  """The whole good corpus in ONE launch, shared by the tests below."""
  return inflate_streams(good)


GROUPS = {
    'stored': ('stored_',),
    'fixed': ('fixed_',),
    'dynamic': ('dynamic_',),
    'overlapping_and_wave_width_matches': ('period_',),
    'far_matches': ('far_',),
    'hand_built_dynamic_headers': ('repeat_', 'single_distance', 'no_distance', 'hclen_', 'fifteen_bit'),
    'block_boundaries_off_the_byte_grid': ('sync_and_full_flush',),
    'ring': ('ring_', 'match_258_across_'),
}


@pytest.mark.parametrize('group', list(GROUPS))
def test_good_streams_inflate_exactly(good, good_results, group):
  status, outs, _, _ = good_results
  picked = [i for i, c in enumerate(good) if c.name.startswith(GROUPS[group])]
  assert picked, group
  for i in picked:
    c = good[i]
    assert int(status[i]) == 0, (c.name, D.STATUS[int(status[i]) & 255])
    want = zlib.decompress(c.stream)
    assert len(outs[i]) == len(want) and outs[i] == want, c.name


def test_every_good_case_belongs_to_a_group_and_nothing_else_is_written(good, good_results):
  prefixes = tuple(p for g in GROUPS.values() for p in g)
  assert all(c.name.startswith(prefixes) for c in good)
  _, _, out, table = good_results
  mask = np.ones(out.size, bool)
  for row in table:
    mask[row[2]:row[2] + row[3]] = False
  assert (out[mask] == 0xA5).all()   # the gaps between the regions keep the fill pattern


def test_misaligned_regions_take_the_byte_flush(good):
  picked = [c for c in good if c.name in ('dynamic_text_level6', 'stored_70000_level0', 'period_65',
                                          'fixed_empty_8_bytes', 'match_258_across_granule_boundary')]
  assert len(picked) == 5
  status, outs, out, table = inflate_streams(picked, misalign=3)
  assert not status.any()
  for c, got in zip(picked, outs):
    assert got == c.data, c.name
  mask = np.ones(out.size, bool)
  for row in table:
    mask[row[2]:row[2] + row[3]] = False
  assert (out[mask] == 0xA5).all()


def test_malformed_streams_get_their_status_next_to_good_ones(good):
  bad = D.bad_cases()
  keep = [c for c in good if c.name in ('dynamic_text_level9', 'period_3', 'far_32506')]
  cases = []
  for i, c in enumerate(bad):    # a good stream after every third bad one
    cases.append(c)
    if i % 3 == 0:
      cases.append(keep[(i // 3) % len(keep)])
  status, outs, _, _ = inflate_streams(cases)
  for c, word, got in zip(cases, status, outs):
    assert int(word) == c.word, (c.name, D.STATUS[int(word) & 255], int(word) >> 8)
    if c.status == 'OK':
      assert got == c.data, c.name
    elif c.status == 'TOO_SHORT':
      assert got[:-1] == zlib.decompress(c.stream) and got[-1] == 0, c.name
    elif c.status not in ('BAD_ADLER', 'BAD_FILTER') and c.name != 'truncated_before_trailer_end':
      # failed before the first granule was written: the whole region is zero-filled
      assert got == bytes(c.expected_len), c.name


def test_entry_point_rejects_bad_tables():
  L = _lib.lib()
  buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
  ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
  st = torch.zeros(4, dtype=torch.int32, device=DEV)

  def call(row, n=1, nbytes=4096, ws_bytes=4096, b=None, status=st.data_ptr()):
    t = np.array([row] * max(n, 1), np.int64)
    return L.se3ds_png_inflate(buf.data_ptr() if b is None else b, nbytes, ws.data_ptr(), ws_bytes,
                               t.ctypes.data, n, status, None)
  for bad in ([8, 10, 0, 20, 10],        # the stream starts inside the table
              [4000, 97, 0, 20, 10],     # leaves buf
              [-1, 10, 0, 20, 10], [64, -1, 0, 20, 10],
              [64, 10, 4090, 20, 10],    # leaves the workspace
              [64, 10, -1, 20, 10], [64, 10, 0, -10, 10],
              [64, 10, 0, 20, 1],        # pitch < 2
              [64, 10, 0, 25, 10],       # no whole number of scan lines
              [64, 2 ** 31, 0, 20, 10], [64, 10, 0, 2 ** 31, 2]):
    assert call(bad) == -1, bad
  good = [64, 10, 0, 20, 10]
  assert call(good, n=0) == -1 and call(good, n=65536) == -1
  assert call(good, nbytes=39) == -1 and call(good, ws_bytes=19) == -1
  assert call(good, b=buf.data_ptr() + 4) == -1 and call(good, status=None) == -1


# ------------------------------------------------------------------------------- end to end
SIZES = [(1, 1), (1, 7), (7, 1), (65, 70), (130, 67)]


def _pixels(rng, h, w, bpp):
  if bpp == 2:
    return rng.integers(0, 65536, (h, w)).astype(np.uint16)
  return rng.integers(0, 256, (h, w, 3) if bpp == 3 else (h, w), dtype=np.uint8)


def test_every_filter_type_geometry_and_pixel_size_equals_the_host_path():
  rng = np.random.default_rng(41)
  batch = {}
  for ft in range(5):
    for bpp in (1, 2, 3):
      for h, w in SIZES:
        # smooth-ish pixels so that the filtered rows compress into matches, not only literals
        pix = _pixels(rng, h, w, bpp)
        pix = (pix // 64 * 64).astype(pix.dtype)
        batch[(ft, bpp, h, w)] = [_png_ref.encode_png(pix, [ft] * h, idat_split=1 + (h + w) % 3)]
  host = png.decode_png_batch(batch, DEV)
  dev = png.decode_png_batch(batch, DEV, inflate='device')
  assert list(dev) == list(host)
  for k in batch:
    assert dev[k].dtype == host[k].dtype and dev[k].shape == host[k].shape, k
    assert torch.equal(dev[k], host[k]), k


def test_mixed_launch_of_all_raw_planes_and_png_streams():
  rng = np.random.default_rng(42)
  kinds = dict(image=3, proj_image=3, depth=2, proj_depth=2, proj_mask=1, blurred_mask=1, segmentation=1)
  assert set(kinds) == set(indoor_datasets.RAW_DTYPES)
  batch = {k: [_png_ref.encode_png(_pixels(rng, 9, 20, bpp) // 32 * 32, rng.integers(0, 5, 9))
               for _ in range(3)] for k, bpp in kinds.items()}
  host = png.decode_png_batch(batch, DEV)
  dev = png.decode_png_batch(batch, DEV, inflate='device')
  streams = {k: [png.parse_png_container(b) for b in v] for k, v in batch.items()}
  dev2 = png.decode_png_batch(streams, DEV, inflate='device')
  for k, dt in indoor_datasets.RAW_DTYPES.items():
    assert dev[k].dtype == dt and torch.equal(dev[k], host[k]) and torch.equal(dev2[k], host[k]), k
  with pytest.raises(ValueError, match='already inflated'):
    png.decode_png_batch({'x': [png.parse_png(batch['image'][0])]}, DEV, inflate='device')
  with pytest.raises(ValueError, match='image'):
    png.decode_png_batch(dict(image=[batch['image'][0], batch['depth'][0]]), DEV, inflate='device')


def _grey_png(case):
  """The case's stream as the IDAT of an 8-bit grey PNG whose geometry is the case's."""
  h = case.expected_len // case.pitch
  assert h >= 1
  return D.png_container(h, case.pitch - 1, 8, 0, case.stream)


REASONS = {
    'TRUNCATED': 'the IDAT stream does not inflate: incomplete or truncated stream',
    'BAD_BLOCK_TYPE': 'the IDAT stream does not inflate: invalid block type',
    'BAD_STORED_LENGTH': 'the IDAT stream does not inflate: invalid stored block lengths',
    'BAD_COUNTS': 'the IDAT stream does not inflate: too many length or distance symbols',
    'BAD_DISTANCE': 'the IDAT stream does not inflate: distance beyond the start of the output',
    'OVER_SUBSCRIBED': 'the IDAT stream does not inflate: over-subscribed set of code lengths',
    'INCOMPLETE': 'the IDAT stream does not inflate: incomplete set of code lengths',
    'BAD_CODE': 'the IDAT stream does not inflate: invalid literal/length or distance code',
    'BAD_REPEAT': 'the IDAT stream does not inflate: invalid bit length repeat',
    'NO_END_OF_BLOCK': 'the IDAT stream does not inflate: missing end-of-block code',
    'TOO_LONG': 'more inflated bytes than 1 x (1 + 99)',
    'TOO_SHORT': 'fewer inflated bytes than 1 x (1 + 101)',
    'BAD_ADLER': 'the IDAT stream does not inflate: incorrect data check',
    'BAD_FILTER': 'filter type 5 in row 2',
    'BAD_HEADER': 'the IDAT stream does not inflate: incorrect zlib header',
}


def test_errors_name_the_first_bad_plane_and_good_planes_still_decode():
  import re
  rng = np.random.default_rng(43)
  pix = [rng.integers(0, 4, (6, 11), dtype=np.uint8) * 60 for _ in range(3)]
  good = [_png_ref.encode_png(p, rng.integers(0, 5, 6)) for p in pix]
  want = png.decode_png_batch({'g': good}, DEV)['g']
  bad = D.bad_cases()
  assert {c.status for c in bad} == set(REASONS)
  for c in bad:
    # one launch: good planes, the bad one at index 1 of its key, more good planes
    zeros = _grey_png(c._replace(stream=D.compress(bytes(c.expected_len))))
    batch = {'before': good[:2], 'pred_depth': [zeros, _grey_png(c)], 'after': good[2:]}
    out, pending = png.decode_png_batch_async(batch, DEV)
    with pytest.raises(ValueError, match='^' + re.escape(f'pred_depth[1]: {REASONS[c.status]}') + '$'):
      pending.check()
    assert torch.equal(out['before'], want[:2]) and torch.equal(out['after'], want[2:]), c.name
    assert not out['pred_depth'][0].any(), c.name
    with pytest.raises(ValueError, match=re.escape('pred_depth[1]')):
      png.decode_png_batch(batch, DEV, inflate='device')
  # the first failed plane is the one named
  sound = _grey_png(bad[5]._replace(stream=D.compress(bytes(bad[5].expected_len))))
  two = {'a': [sound, _grey_png(bad[5])], 'b': [_grey_png(bad[0])]}
  with pytest.raises(ValueError, match=re.escape('a[1]: ')):
    png.decode_png_batch(two, DEV, inflate='device')


def test_async_form_returns_before_the_wait():
  rng = np.random.default_rng(44)
  bufs = [_png_ref.encode_png(rng.integers(0, 3, (40, 50, 3), dtype=np.uint8) * 100, rng.integers(0, 5, 40))
          for _ in range(4)]
  want = png.decode_png_batch({'x': bufs}, DEV)['x']
  torch.cuda.synchronize()
  gate = torch.cuda.Event()
  # a long queue of device work in front: the call returns while the stream is still busy with it
  a = torch.ones((64 << 20,), device=DEV)
  for _ in range(400):
    a.mul_(1.0001)
  out, pending = png.decode_png_batch_async({'x': bufs}, DEV)
  gate.record()
  returned_early = not gate.query()
  pending.check()          # returns for a good batch
  assert returned_early, 'decode_png_batch_async waited for the device'
  assert pending._event.query()
  assert torch.equal(out['x'], want)
  pending.check()          # and may be asked again


def test_image_input_fn_device_inflate_equals_host(tmp_path):
  rng = np.random.default_rng(45)
  made = [image_record(8, rng, depth_scale=np.array([10.0 + i], np.float32)) for i in range(4)]
  tf_records.write_records(str(tmp_path / 'train-00000.tfrecord'), [m[0] for m in made[:3]])
  tf_records.write_records(str(tmp_path / 'train-00001.tfrecord'), [made[3][0]])
  ds = indoor_datasets.R2RImageDataset(image_size=4, preprocessed_image_height=8, data_dir=str(tmp_path),
                                       return_filename=True)
  kw = dict(batch_size=2, seed=5, input_pipeline_id=2, device=DEV, shuffle=True, shuffle_buffer_size=3)
  host_it = ds.input_fn('train', **kw)
  dev_it = ds.input_fn('train', inflate='device', **kw)
  for _ in range(3):
    h, d = next(host_it), next(dev_it)
    assert set(h) == set(d)
    for k, v in h.items():
      if torch.is_tensor(v):
        assert d[k].dtype == v.dtype and torch.equal(d[k], v), k
      else:
        assert d[k] == v, k
  host_it.close()
  dev_it.close()
  # a finite stream ends where the host path's ends, the remainder dropped
  n_host = len(list(ds.input_fn('train', num_epochs=1, batch_size=3, device=DEV)))
  n_dev = len(list(ds.input_fn('train', num_epochs=1, batch_size=3, device=DEV, inflate='device')))
  assert n_host == n_dev == 1
  with pytest.raises(ValueError, match='inflate'):
    next(ds.input_fn('train', device=DEV, inflate='both'))


def test_video_input_fn_accepts_the_argument(tmp_path):
  rng = np.random.default_rng(46)
  rec, _ = video_record(4, rng)
  rec2, _ = video_record(4, rng)
  path = str(tmp_path / 'val_unseen-0.tfrecord')
  tf_records.write_records(path, [rec, rec2])
  ds = indoor_datasets.R2RVideoDataset(image_size=2, preprocessed_image_height=4, horizontal_mask_ratio=0.25)
  run = lambda **kw: list(ds.input_fn(ds.examples_from_tfrecords(file_pattern=path), 2, seed=3, num_epochs=1,
                                      device=DEV, **kw))
  host, dev = run(), run(inflate='device')
  assert len(host) == len(dev) == 1 and set(host[0]) == set(dev[0])
  for k, v in host[0].items():
    assert dev[0][k].dtype == v.dtype and torch.equal(dev[0][k], v), k
  with pytest.raises(ValueError, match='inflate'):
    run(inflate='gpu')
