"""The record writer on the GPU (csrc/records.hip, the 16-bit path of csrc/png_encode.hip,
datasets/record_writer.py): streams byte for byte against the host build of csrc/deflate_core.h, both
decoders on the files, the segment copy against a NumPy gather with canaries, the CRC patch against
struct.pack, the planes kernel on a lattice, and written files against the Python layout and this
project's own input pipeline.  Every comparison is of bytes or integers."""
import os
import struct

import numpy as np
import pytest
import torch

import _png_encode_ref as R
import _record_ref as Q
from _records import video_record
from se3ds_amd import constants
from se3ds_amd.datasets import indoor_datasets, record_writer
from se3ds_amd.utils import pano_utils, png, tf_records

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CANARY = 0xA5


def _as_int16(samples):
  return torch.from_numpy(samples.view(np.int16).copy()).to(DEV)[:, :, None].contiguous()


class Encoded:
  """Every 16-bit size x content, each under another filter mode, mixed with 8-bit grey and RGB
  images in one launch: the shared reference of the tests below."""

  def __init__(self, tmp):
    self.names, self.pixels, self.modes, self.entries = [], [], [], []
    k = 0
    for si, (h, w) in enumerate(Q.SIZES_16):
      for name, samples in Q.contents_16(h, w, seed=20 + si).items():
        for mode in ((k % 6, (k + 3) % 6) if h < 128 else (k % 6, 5)):
          self.names.append(((h, w, 16), name))
          self.pixels.append(samples)
          self.modes.append(mode)
          self.entries.append(Q.corpus_entry_16(samples, mode))
        k += 1
      for c in (1, 3):   # an 8-bit neighbour of each kind behind every 16-bit size
        px = R.contents(min(h, 9), w, c, seed=40 + si)['ramp + noise']
        self.names.append(((px.shape[0], w, c), 'ramp + noise'))
        self.pixels.append(px)
        self.modes.append(5)
        self.entries.append(R.corpus_file([(px, 5)])[8:])
    self.tensors = [_as_int16(p) if p.dtype == np.uint16 else torch.from_numpy(p).to(DEV)
                    for p in self.pixels]
    if hasattr(torch, 'uint16'):   # the same bits under torch's own name for them: a single pixel,
      for i in (0, self.names.index(((7, 64, 16), 'ramp')),      # rows, and two strips
                self.names.index(((128, 256, 16), 'noise'))):
        self.tensors[i] = self.tensors[i].view(torch.uint16)
    self.filters = ['adaptive' if m == 5 else m for m in self.modes]
    self.table, self.sizes, self.buffer = png.encode_streams(self.tensors, self.filters, fill=CANARY)
    self.streams = [self.buffer[int(r[6]):int(r[6]) + int(s[0])].tobytes()
                    for r, s in zip(self.table, self.sizes)]
    exe = R.build_host_program(tmp, sanitize=False)
    self.host, _ = Q.run_host_program_raw(exe, self.entries, tmp)


@pytest.fixture(scope='module')
def enc(tmp_path_factory):
  return Encoded(tmp_path_factory.mktemp('record_png'))


def test_16_bit_streams_equal_the_host_build_of_the_core(enc):
  assert sum(p.dtype == np.uint16 for p in enc.pixels) >= 24
  for key, stream, (want, s1, s2), adler in zip(enc.names, enc.streams, enc.host, enc.sizes[:, 1]):
    assert stream == want, key
    assert int(adler) == (s2 << 16) | s1, key
  assert int(enc.table[enc.names.index(((128, 256, 16), 'noise')) + 1, 5]) - \
      int(enc.table[enc.names.index(((128, 256, 16), 'noise')), 5]) == 2   # two strips


def test_16_bit_files_decode_to_the_samples(enc):
  files = png.encode_png_batch(enc.tensors, enc.filters)
  for f, stream, adler in zip(files, enc.streams, enc.sizes[:, 1]):
    assert png.parse_png_container(f).compressed == b'\x78\x01' + stream + struct.pack('>I', int(adler))
  keyed = {str(i): [f] for i, f in enumerate(files)}
  for inflate in ('host', 'device'):
    out = png.decode_png_batch(keyed, DEV, inflate=inflate)
    for i, (px, key) in enumerate(zip(enc.pixels, enc.names)):
      got = out[str(i)][0].cpu().numpy()
      if px.dtype == np.uint16:
        assert got.dtype == np.int16 and np.array_equal(got.view(np.uint16), px), (key, inflate)
      else:
        assert np.array_equal(got.reshape(px.shape), px), (key, inflate)


def test_rest_of_the_output_buffer_is_untouched_and_runs_are_identical(enc):
  ends = list(enc.table[1:, 6]) + [len(enc.buffer)]
  for row, size, end in zip(enc.table, enc.sizes[:, 0], ends):
    assert np.all(enc.buffer[int(row[6]) + int(size):int(end)] == CANARY)
  table, sizes, buffer = png.encode_streams(enc.tensors, enc.filters, fill=CANARY)
  assert np.array_equal(sizes, enc.sizes) and np.array_equal(buffer, enc.buffer)


def _small_images():
  """A 3x5 RGB and a 1x1 grey uint8 image and a 2x7 int16 plane."""
  rng = np.random.default_rng(31)
  rgb = torch.from_numpy(rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)).to(DEV)
  grey = torch.from_numpy(rng.integers(0, 256, (1, 1, 1), dtype=np.uint8)).to(DEV)
  return rgb, grey, _as_int16(rng.integers(0, 65536, (2, 7), dtype=np.uint16))


def test_launch_encode_and_a_download_equal_encode_streams():
  images = list(_small_images())
  want_table, want_sizes, want_streams = png.encode_streams(images, 'adaptive', fill=CANARY)
  table, result, head = png.launch_encode(images, [png.ADAPTIVE] * 3, fill=CANARY)
  buf = result.cpu().numpy()   # waits for the stream the encode is queued on
  assert head == 32   # the 24 bytes of sizes, rounded up to 16
  assert np.array_equal(table, want_table)
  assert np.array_equal(buf[:8 * 3].view(np.uint32).reshape(3, 2), want_sizes)
  assert np.array_equal(buf[head:], want_streams)
  assert all(int(s) > 0 for s in want_sizes[:, 0])


def test_a_uint8_batch_equals_its_images_encoded_one_by_one():
  """A batch without a 16-bit plane takes se3ds_png_encode, as every image alone does."""
  rgb, grey, _ = _small_images()
  table, sizes, streams = png.encode_streams([rgb, grey], 'adaptive')
  assert not np.any(table[:, 3] == 2)
  for i, x in enumerate((rgb, grey)):
    _, one_size, one = png.encode_streams([x], 'adaptive')
    assert np.array_equal(sizes[i], one_size[0])
    at, size = int(table[i, 6]), int(sizes[i, 0])
    assert size > 0 and np.array_equal(streams[at:at + size], one[:size])
  assert png.encode_png_batch([rgb, grey]) == png.encode_png_batch([rgb]) + png.encode_png_batch([grey])


LENGTHS = (0, 1, 3, 15, 16, 17, 63, 64, 65, 4097, 70001)


def test_segment_copy_equals_a_numpy_gather():
  """Every length at every source residue mod 16, each with four destination residues that put the
  source 0..3 bytes off the destination's word phase, from two source buffers; what lies outside the
  destinations -- at least 32 bytes between two segments -- keeps its canary."""
  rng = np.random.default_rng(7)
  sources = [rng.integers(0, 256, 300000, dtype=np.uint8), rng.integers(0, 256, 200001, dtype=np.uint8)]
  rows, pos, seen = [], 16, set()
  for li, length in enumerate(LENGTHS):
    for r in range(16):
      for j in range(4):
        which = (r + j + li) % 2
        at = 16 * int(rng.integers(0, (len(sources[which]) - length - 16) // 16)) + r
        to = ((pos + 15) & ~15) + 32 + (r + 5 * j + li) % 16
        rows.append((which, at, to, length))
        seen.add((length, at % 16, to % 16, (at - to) % 4))
        pos = to + length
  for length in LENGTHS:
    assert {s[1] for s in seen if s[0] == length} == set(range(16))
    assert {s[2] for s in seen if s[0] == length} == set(range(16))
    assert {s[3] for s in seen if s[0] == length} == set(range(4))
  rows.append((1, len(sources[1]) - 7, pos + 40, 7))   # the last bytes of a source, of out
  total = pos + 47
  want = np.full(total, CANARY, np.uint8)
  for which, at, to, length in rows:
    want[to:to + length] = sources[which][at:at + length]
  out = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
  record_writer.assemble_segments([torch.from_numpy(s).to(DEV) for s in sources], rows, out)
  got = out.cpu().numpy()
  assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
  again = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
  record_writer.assemble_segments([torch.from_numpy(s).to(DEV) for s in sources], rows, again)
  assert torch.equal(again, out)


def test_crc_patch_both_forms_at_odd_offsets():
  rng = np.random.default_rng(8)
  crcs = np.concatenate([rng.integers(0, 1 << 32, 6, dtype=np.uint64).astype(np.uint32),
                         np.array([0, 0xffffffff, 0x80000000, 0x00007fff, 0x5d7d1527], np.uint32)])
  patches = [(i, 1 + 6 * i + (i % 2) * 2, i % 2) for i in range(len(crcs))]   # 1, 9, 13, 21, ...
  patches += [(4, 101, 1), (4, 105, 0), (0, 196, 1)]                          # back to back; the last 4 bytes
  assert all(at % 2 == 1 for _, at, _ in patches[:-1])
  want = np.full(200, CANARY, np.uint8)
  for which, at, form in patches:
    c = int(crcs[which])
    word = struct.pack('>I', c) if form == 0 else \
        struct.pack('<I', (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xffffffff)
    want[at:at + 4] = np.frombuffer(word, np.uint8)
  out = torch.full((200,), CANARY, dtype=torch.uint8, device=DEV)
  record_writer.patch_crc(out, torch.from_numpy(crcs.view(np.int32)).to(DEV), patches)
  assert np.array_equal(out.cpu().numpy(), want)


def test_planes_kernel_on_a_lattice():
  special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, -1e-30, 1e-30, -0.5, 1.5, 2.0, 256.0, 300.0,
                      1e30, -1e30, 65535.0, 65536.0, constants.INVALID_RGB_VALUE], np.float32)
  codes = np.arange(65536, dtype=np.float32)
  depth = np.concatenate([Q.neighbours(codes / np.float32(65535)),
                          Q.neighbours(codes * (np.float32(1) / np.float32(65535))),
                          Q.neighbours((codes[:-1] + np.float32(0.5)) / np.float32(65535)), special])
  k = np.arange(256, dtype=np.float32)
  rgb_lattice = np.concatenate([Q.neighbours(k), Q.neighbours(k / np.float32(255)),
                                Q.neighbours(k + np.float32(0.5)), special])
  mask_lattice = np.concatenate([Q.neighbours(np.array([0, 1, 0.5, 255], np.float32)), special])
  pixels = len(depth)
  rgb = np.resize(rgb_lattice, 3 * pixels).reshape(pixels, 3)
  mask = np.resize(mask_lattice, pixels)
  want = (Q.rgb_codes(rgb), Q.depth_codes(depth), Q.mask_codes(mask))
  assert np.array_equal(want[1][:65536], np.arange(65536))
  rgb_d, depth_d, mask_d = (torch.from_numpy(a).to(DEV) for a in (rgb, depth, mask))
  for lo, hi in ((0, pixels), (0, pixels - 1), (1, pixels), (3, pixels - 2), (5, 8), (7, 8)):
    # whole and odd counts (the last pixels go one by one), and starts 4 or 12 bytes off a 16-byte
    # boundary (the kernel's one-by-one form)
    got = record_writer.record_planes(rgb_d[lo:hi], depth_d[lo:hi], mask_d[lo:hi])
    assert [g.dtype for g in got] == [torch.uint8, torch.int16, torch.uint8]
    assert np.array_equal(got[0].cpu().numpy(), want[0][lo:hi]), (lo, hi)
    assert np.array_equal(got[1].cpu().numpy().view(np.uint16), want[1][lo:hi]), (lo, hi)
    assert np.array_equal(got[2].cpu().numpy(), want[2][lo:hi]), (lo, hi)
  # any subset of the pairs
  only = record_writer.record_planes(proj_depth=depth_d.reshape(1, -1))
  assert only.shape == (1, pixels) and np.array_equal(only.cpu().numpy().view(np.uint16)[0], want[1])
  two = record_writer.record_planes(proj_rgb=rgb_d, proj_mask=mask_d)
  assert np.array_equal(two[0].cpu().numpy(), want[0]) and np.array_equal(two[1].cpu().numpy(), want[2])


def _examples(h, rng, count):
  w = 2 * h
  x, y = np.arange(w)[None, :], np.arange(h)[:, None]
  out = []
  for i in range(count):
    planes = dict(
        image=((3 * x + 2 * y)[:, :, None] + rng.integers(0, 9, (h, w, 3))).astype(np.uint8),
        depth=((300 * x + 77 * y + rng.integers(0, 50, (h, w))) % 65536).astype(np.uint16),
        proj_image=rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
        proj_depth=rng.integers(0, 65536, (h, w)).astype(np.uint16),
        proj_mask=(rng.integers(0, 2, (h, w)) * 255).astype(np.uint8),
        blurred_mask=(y + 0 * x > h // 2).astype(np.uint8),
        segmentation=((x // 16 + y // 16) % 42).astype(np.uint8))
    meta = dict(scan_id=b'scan%d' % i, filename=b'%d.png' % i, depth_scale=10.0 + i,
                bbox=(0.0, 0.25, 0.5, 1.0)) if i != 1 else {}
    out.append((planes, meta))
  return out


def _to_device(planes):
  return {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).to(DEV)
          for k, v in planes.items()}


def test_writer_file_equals_the_python_layout_and_reads_back(tmp_path):
  rng = np.random.default_rng(9)
  h = 128
  examples = _examples(h, rng, 3)
  examples[2][0].pop('blurred_mask')   # absent planes are zeros
  examples[2][0].pop('segmentation')
  path = str(tmp_path / 'train-00000.tfrecord')
  with record_writer.R2RRecordWriter(path, DEV, examples_per_flush=2) as writer:
    for planes, meta in examples:
      writer.add(**_to_device(planes), **meta)
      assert os.path.exists(path + '.tmp') and not os.path.exists(path)
    assert writer.examples == 2   # one flush is done, a partial one is left for the exit
  assert sorted(os.listdir(tmp_path)) == ['train-00000.tfrecord']
  blob = open(path, 'rb').read()
  assert writer.examples == 3 and writer.bytes_written == len(blob)
  zeros = np.zeros((h, 2 * h), np.uint8)
  full = [dict(dict(blurred_mask=zeros, segmentation=zeros), **planes) for planes, _ in examples]
  # the same planes' PNGs from the device encoder, laid out in Python
  tensors = [t.reshape(t.shape[0], t.shape[1], -1) for p in full for t in _to_device(p).values()]
  files = iter(png.encode_png_batch(tensors, 'adaptive'))
  hosts = [dict({name: next(files) for name in p}, **meta) for p, (_, meta) in zip(full, examples)]
  assert blob == record_writer.encode_records_host(hosts)
  # strips as the issue says: depth and RGB planes two, masks one
  assert png.strip_rows(2 * 2 * h) < h <= 2 * png.strip_rows(2 * 2 * h) and png.strip_rows(2 * h) >= h
  records = list(tf_records.read_records(path, verify=True))
  assert records == list(tf_records.read_records(path, verify='device')) and len(records) == 3
  for rec, planes, host in zip(records, full, hosts):
    parsed = tf_records.parse_example(rec)
    by_plane = {name: [parsed[feature][0]] for name, (feature, _, _) in indoor_datasets.IMAGE_PLANES.items()}
    for inflate in ('host', 'device'):
      decoded = png.decode_png_batch(by_plane, DEV, inflate=inflate)
      for name, want in planes.items():
        got = decoded[name][0].cpu().numpy()
        assert got.dtype == (np.int16 if want.dtype == np.uint16 else np.uint8), name
        assert np.array_equal(got.view(want.dtype), want), (name, inflate)
    assert parsed['scan_id'] == [host.get('scan_id', b'')]
    assert parsed['depth_scale'][0] == np.float32(host.get('depth_scale', 10.0))
  # one batch through the input pipeline, in the shapes the training step takes
  ds = indoor_datasets.R2RImageDataset(image_size=32, preprocessed_image_height=h, data_dir=str(tmp_path))
  for inflate in ('host', 'device'):
    it = ds.input_fn('train', batch_size=2, seed=1, device=DEV, verify_crc=True, inflate=inflate)
    batch = next(it)
    it.close()
    for key, channels in dict(image=3, proj_image=3, proj_mask=1, proj_depth=1, depth=1, blurred_mask=1).items():
      assert batch[key].shape == (2, 32, 64, channels) and batch[key].dtype == torch.float32, key
    assert batch['segmentation'].shape == (2, 32, 64, 1) and batch['segmentation'].dtype == torch.int32
  # views that are dense but not row-major are written as they index: an RGB plane that is a
  # permuted CHW tensor, a grey and a 16-bit plane that are transposed views
  strided = str(tmp_path / 'strided.tfrecord')
  planes = _to_device(full[0])
  chw = planes['image'].permute(2, 0, 1).contiguous()
  views = dict(planes, image=chw.permute(1, 2, 0), proj_mask=planes['proj_mask'].t().contiguous().t(),
               depth=planes['depth'].t().contiguous().t())
  assert not any(views[k].is_contiguous() for k in ('image', 'proj_mask', 'depth'))
  with record_writer.R2RRecordWriter(strided, DEV) as writer:
    writer.add(**views, **examples[0][1])
  assert open(strided, 'rb').read() == blob[:len(open(strided, 'rb').read())]   # the first record again
  rec, = tf_records.read_records(strided, verify=True)
  parsed = tf_records.parse_example(rec)
  decoded = png.decode_png_batch({name: [parsed[feature][0]] for name, (feature, _, _) in
                                  indoor_datasets.IMAGE_PLANES.items()}, DEV)
  for name, want in full[0].items():
    assert np.array_equal(decoded[name][0].cpu().numpy().view(want.dtype), want), name
  os.remove(strided)
  # a writer that is dropped without close or abort leaves nothing either
  dropped = record_writer.R2RRecordWriter(str(tmp_path / 'dropped.tfrecord'), DEV)
  dropped.add(**planes)
  del dropped
  import gc
  gc.collect()
  assert sorted(os.listdir(tmp_path)) == ['train-00000.tfrecord']
  # a writer that fails leaves nothing
  bad = str(tmp_path / 'train-00001.tfrecord')
  with pytest.raises(ValueError):
    with record_writer.R2RRecordWriter(bad, DEV) as writer:
      good = _to_device(examples[0][0])
      writer.add(**good)
      writer.add(**dict(good, depth=good['depth'].to(torch.float32)))
  assert sorted(os.listdir(tmp_path)) == ['train-00000.tfrecord']


def test_guidance_planes_equal_the_public_calls():
  torch.manual_seed(11)
  n, h, w = 2, 32, 64
  void = constants.INVALID_RGB_VALUE
  prev_rgb = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=DEV)
  prev_depth = (0.15 + 0.5 * torch.rand((n, h, w), device=DEV)).contiguous()
  prev_position = torch.tensor([[0.0, 0.0, 0.0], [1.0, -0.5, 0.2]], device=DEV)
  position = prev_position + torch.tensor([[0.4, 0.3, 0.0], [-0.2, 0.5, 0.1]], device=DEV)
  got = record_writer.guidance_planes(prev_rgb, prev_depth, prev_position, position, depth_scale=10.0)
  assert [(g.dtype, tuple(g.shape)) for g in got] == [
      (torch.uint8, (n, h, w, 3)), (torch.int16, (n, h, w)), (torch.uint8, (n, h, w))]
  masked = pano_utils.mask_pano(prev_rgb.to(torch.int32), masked_region_value=void)
  xyz1, feats = pano_utils.equirectangular_to_pointcloud(masked, prev_depth, void, 10.0,
                                                         interpolation_method='bilinear',
                                                         position=prev_position)
  f_xyz1, f_rgb = pano_utils.compact_valid_points(xyz1, feats, void)
  proj_depth, proj_rgb, proj_mask = pano_utils.project_feats_to_equirectangular(
      f_rgb.to(torch.int32), f_xyz1, h, w, void, 10.0, offset=position, with_mask=True, mask_void=void)
  assert np.array_equal(got[0].cpu().numpy(), Q.rgb_codes(proj_rgb.cpu().numpy()))
  assert np.array_equal(got[1].cpu().numpy().view(np.uint16), Q.depth_codes(proj_depth.cpu().numpy()))
  assert np.array_equal(got[2].cpu().numpy(), Q.mask_codes(proj_mask.cpu().numpy()))
  assert 0 < int((got[2] == 255).sum()) < n * h * w   # holes and hits: the target is displaced
  # the rows mask_pano makes void never enter the warp: it keeps rows [h / 8, h - h / 8], the last
  # one included as in the reference (utils/pano_utils.py:245-265), so the top eighth and the rows
  # below h - h / 8
  other = prev_rgb.clone()
  other[:, :h // 8] = 255 - other[:, :h // 8]
  other[:, h - h // 8 + 1:] = 7
  again = record_writer.guidance_planes(other, prev_depth, prev_position, position, depth_scale=10.0)
  assert all(torch.equal(a, b) for a, b in zip(again, got))
  other[:, h - h // 8] = 255 - other[:, h - h // 8]   # the kept boundary row does
  moved = record_writer.guidance_planes(other, prev_depth, prev_position, position, depth_scale=10.0)
  assert not torch.equal(moved[0], got[0]) and torch.equal(moved[1], got[1]) and torch.equal(moved[2], got[2])


def test_trajectory_example_round_trip(tmp_path):
  rng = np.random.default_rng(12)
  h = 4
  ds = indoor_datasets.R2RVideoDataset(image_size=2, preprocessed_image_height=h, return_filename=True)
  made = [video_record(h, rng, pathdreamer=True)[1], video_record(h, rng, pathdreamer=False)[1]]
  records = [record_writer.encode_trajectory_example(dict(a, scan_id=b'scanA')) for a in made]
  device_path, host_path = str(tmp_path / 'val-0.tfrecord'), str(tmp_path / 'val-1.tfrecord')
  tf_records.write_records(device_path, records, checksums='device')
  tf_records.write_records(host_path, records)
  assert open(device_path, 'rb').read() == open(host_path, 'rb').read()
  assert sorted(os.listdir(tmp_path)) == ['val-0.tfrecord', 'val-1.tfrecord']
  for rec, arrays in zip(tf_records.read_records(device_path, verify=True), made):
    out = ds._parse(rec)
    assert set(out) == set(arrays) | {'scan_id'} and out['scan_id'] == b'scanA'
    for key, want in arrays.items():
      assert np.array_equal(out[key], want) and np.asarray(out[key]).dtype == np.asarray(want).dtype, key
  # several slabs give the same file
  tf_records.write_records(device_path, records, checksums='device', slab_bytes=1000)
  assert open(device_path, 'rb').read() == open(host_path, 'rb').read()
