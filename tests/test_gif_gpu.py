"""The GIF encoder on the GPU (csrc/gif.hip): every stage and the whole files against the
restatement of tests/_gif_ref.py, exact equality throughout; the ABI's refusals; log_videos and
GANManager.test(rollout_video=True)."""
import io
import os

import numpy as np
import pytest
import torch

import _gif_ref as R
from se3ds_amd import _lib
from se3ds_amd.utils import gif, logger as logger_lib, tf_events

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _colour(t, h, w, seed):
  """Smooth gradients with a noisy patch, drifting over the frames; some pixels at 0 and 255."""
  base = R.synthetic_frame(max(h, 8), max(w, 8), seed)[:h, :w]
  video = np.stack([np.roll(base, 3 * i, axis=1) for i in range(t)])
  video[0, 0, :2] = [[0, 0, 0], [255, 255, 255]]
  return video


# --------------------------------------------------------------------------------- the stages
def test_histogram():
  random = R.noise((3, 37, 53, 3), 1)
  constant = np.full((1, 300, 300, 3), (200, 17, 90), np.uint8)    # 90 000 pixels in one bin
  odd = _colour(2, 19, 23, 2)                                      # 874 pixels: a tail of two
  grey = R.noise((2, 5, 5, 1), 3)
  for videos in ([random], [constant], [random, grey, odd, constant]):
    batch = gif.GifBatch([_dev(v) for v in videos])
    batch.histogram()
    got = batch.histograms().cpu().numpy().view(np.uint32)
    for i, v in enumerate(videos):
      want = R.histogram(v) if v.shape[3] == 3 else np.zeros(32768, np.uint32)
      assert np.array_equal(got[i], want), i
  assert got[3].max() == 90000


def test_look_up_table():
  rng = np.random.default_rng(5)
  dup = rng.integers(0, 256, (256, 3)).astype(np.uint8)
  dup[1::2] = dup[::2]                      # ties: the lower index wins
  dup[100:] = 0                             # padding behind n_used is not a candidate
  dup[7] = 0                                # ... but black in use is
  random = rng.integers(0, 256, (256, 3)).astype(np.uint8)
  videos = [_dev(_colour(1, 8, 8, 1)), _dev(R.noise((1, 4, 4, 1), 2)), _dev(_colour(1, 9, 9, 3))]
  batch = gif.GifBatch(videos)
  batch.region(1).fill_(0xee)
  batch.lut(np.stack([dup, np.zeros((256, 3), np.uint8), random]), np.array([100, 0, 256], np.int32))
  got = batch.region(1).cpu().numpy()[:3 * 32768].reshape(3, 32768)
  assert np.array_equal(got[0], R.nearest_lut(dup, 100)) and got[0].max() < 100
  assert (got[1] == 0xee).all()             # a grey video has no table
  assert np.array_equal(got[2], R.nearest_lut(random, 256))


@pytest.mark.parametrize('dither', [0, 32])
def test_index_plane(dither):
  video = _colour(2, 19, 23, 4)             # rows of 69 bytes: no row but the first starts on a dword
  other = R.noise((1, 3, 5, 3), 6)
  palette, used = R.median_cut(R.histogram(video))
  lut = R.nearest_lut(palette, used)
  lut2 = R.nearest_lut(palette[::-1].copy(), 256)
  batch = gif.GifBatch([_dev(video), _dev(other)], dither)
  batch.lut(np.stack([palette, palette[::-1]]), np.array([used, 256], np.int32))
  batch.index()
  plane = batch.region(2).cpu().numpy()
  for row, v, table in zip(batch.table, (video, other), (lut, lut2)):
    n = v.size // 3
    got = plane[int(row[8]):int(row[8]) + n].reshape(v.shape[:3])
    assert np.array_equal(got, R.index_plane(v, table, dither))


# ------------------------------------------------------------------------------ whole files
def _grey_cases():
  """name -> (T,H,W,1): the LZW and pack paths; the index plane is the input."""
  cases = {}
  for w in (1, 7, 64, 65, 255, 256, 1000):
    rows = R.strip_rows(w)
    heights = (17, 34, 40) if w == 1000 else (rows, 2 * rows, 2 * rows + max(1, rows // 3))
    for h in heights:    # one strip, two, three with a short last one; noise: >= 16 384 pixels a strip
      cases[f'noise {h}x{w}'] = R.noise((1, h, w, 1), h + w)
  cases['noise T=5'] = R.noise((5, 40, 1000, 1), 8)
  cases['constant'] = np.full((1, 40, 1000, 1), 77, np.uint8)
  cases['constant T=5 2 strips'] = np.full((5, 300, 64, 1), 255, np.uint8)
  cases['constant 1x1'] = np.zeros((1, 1, 1, 1), np.uint8)
  ramp = (np.arange(3 * 50 * 700) % 5).astype(np.uint8)
  cases['ramp'] = ramp.reshape(3, 50, 700, 1)
  for w in range(250, 262):   # the closing code meets the 9 -> 10 bit switch
    cases[f'row {w}'] = R.noise((1, 1, w, 1), w)
  return cases


@pytest.fixture(scope='module')
def grey_files():
  cases = _grey_cases()
  files = gif.encode_gif_batch([_dev(v) for v in cases.values()])   # one batch, one launch per stage
  return cases, dict(zip(cases, files))


def test_lzw_and_pack_whole_files(grey_files):
  cases, files = grey_files
  assert len(files) == len(cases) == 21 + 5 + 12
  for name, video in cases.items():
    assert files[name] == R.encode(video), name


def test_grey_decodes_to_itself(grey_files):
  cases, files = grey_files
  for name in ('noise 40x1000', 'noise T=5', 'ramp', 'row 256', 'noise 32768x1'):
    f = R.decode_file(files[name])
    assert np.array_equal(f['frames'][..., None], cases[name]), name
    assert np.array_equal(f['palette'], R.grey_palette())


def test_mixed_batch_and_end_to_end():
  grey, colour = R.noise((2, 40, 1000, 1), 11), _colour(3, 33, 65, 12)
  files = gif.encode_gif_batch([_dev(grey), _dev(colour)], fps=30, loop=None)
  assert files[0] == R.encode(grey, fps=30, loop=None)
  assert files[1] == R.encode(colour, fps=30, loop=None)
  assert files[1] == gif.encode_gif_host(colour, fps=30, loop=None)
  palette, index = R.quantise(colour, 32)
  f = R.decode_file(files[1])
  assert f['loop'] is None and f['delays'] == [3, 3, 3]
  assert np.array_equal(f['palette'][f['frames']], palette[index])
  parsed = gif.parse_gif(files[1])
  assert [len(d) for d in parsed.frames] == [sum(b) for b in f['blocks']]
  try:
    from PIL import Image
  except ImportError:
    return
  im = Image.open(io.BytesIO(files[1]))
  assert im.n_frames == 3
  for i in range(3):
    im.seek(i)
    assert np.array_equal(np.asarray(im.convert('RGB')), palette[index[i]])


@pytest.mark.parametrize('dither', [0, 32])
def test_colour_dither_settings(dither):
  colour = _colour(2, 21, 37, 13)
  assert gif.encode_gif_batch([_dev(colour)], dither=dither) == [R.encode(colour, dither=dither)]


def test_a_view_gives_the_bytes_of_its_copy():
  wide = _dev(_colour(2, 24, 50, 14))
  view = wide[:, ::2, 3:40]
  assert not view.is_contiguous()
  got = gif.encode_gif_batch([view, wide.permute(0, 2, 1, 3)])
  assert got == gif.encode_gif_batch([view.contiguous(), wide.permute(0, 2, 1, 3).contiguous()])
  assert got[0] == R.encode(view.cpu().numpy())


# ----------------------------------------------------------------------------------- the ABI
def test_abi_refusals():
  L = _lib.lib()
  src = torch.zeros((4 * 8 * 8 * 3,), dtype=torch.uint8, device=DEV)

  def table(t=4, h=8, w=8, c=3, dither=32):
    row = np.zeros((1, L.se3ds_gif_fields()), np.int64)
    row[0, :6] = (src.data_ptr(), t, h, w, c, dither)
    return row

  good = table()
  assert L.se3ds_gif_plan(good.ctypes.data, 1) == 0
  need = L.se3ds_gif_workspace_bytes(good.ctypes.data, 1)
  out_need = L.se3ds_gif_out_bytes(good.ctypes.data, 1)
  assert need > 0 and out_need > 0
  workspace = torch.full((need,), 0x5a, dtype=torch.uint8, device=DEV)
  out = torch.full((out_need,), 0x5a, dtype=torch.uint8, device=DEV)
  table_dev = _dev(good.view(np.uint8).reshape(-1))
  stages = [lambda host, size, fn=getattr(L, name): fn(table_dev.data_ptr(), host.ctypes.data, 1,
                                                       workspace.data_ptr(), size, _lib.stream())
            for name in ('se3ds_gif_histogram', 'se3ds_gif_index', 'se3ds_gif_lzw')]
  stages.append(lambda host, size: L.se3ds_gif_lut(table_dev.data_ptr(), host.ctypes.data, 1, src.data_ptr(),
                                                   src.data_ptr(), workspace.data_ptr(), size, _lib.stream()))
  stages.append(lambda host, size: L.se3ds_gif_pack(table_dev.data_ptr(), host.ctypes.data, 1, workspace.data_ptr(),
                                                    size, out.data_ptr(), out_need, _lib.stream()))
  bad_shape, bad_workspace = _lib.ABI['SE3DS_E_BADSHAPE'], _lib.ABI['SE3DS_E_WORKSPACE']
  for kw in (dict(c=2), dict(t=0), dict(w=65536), dict(h=0), dict(dither=256)):
    bad = table(**kw)
    assert L.se3ds_gif_plan(bad.ctypes.data, 1) == bad_shape, kw
    assert L.se3ds_gif_workspace_bytes(bad.ctypes.data, 1) == 0
    assert L.se3ds_gif_out_bytes(bad.ctypes.data, 1) == 0
    for stage in stages:
      assert stage(bad, need) == bad_shape, kw
  unplanned = table()
  unplanned[0, 11] = 1
  for stage in stages:
    assert stage(unplanned, need) == bad_shape       # a derived field that plan did not write
    assert stage(good, need - 1) == bad_workspace
  assert L.se3ds_gif_pack(table_dev.data_ptr(), good.ctypes.data, 1, workspace.data_ptr(), need, out.data_ptr(),
                          out_need - 1, _lib.stream()) == bad_shape
  assert L.se3ds_gif_pack(table_dev.data_ptr(), good.ctypes.data, 1, workspace.data_ptr(), need, None,
                          out_need, _lib.stream()) == bad_shape
  assert L.se3ds_gif_lzw(None, good.ctypes.data, 1, workspace.data_ptr(), need, _lib.stream()) == bad_shape
  assert L.se3ds_gif_lzw(table_dev.data_ptr(), None, 1, workspace.data_ptr(), need, _lib.stream()) == bad_shape
  torch.cuda.synchronize()
  assert bool((workspace == 0x5a).all()) and bool((out == 0x5a).all())   # nothing was launched
  with pytest.raises(ValueError):
    gif.encode_gif_batch([torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device=DEV)])
  with pytest.raises(ValueError):
    gif.encode_gif_batch([torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device=DEV)])
  with pytest.raises(_lib.Se3dsHipError):
    gif.encode_gif_batch([torch.zeros((1, 4, 4, 3), dtype=torch.uint8)])


# --------------------------------------------------------------------------- logger, test loop
def test_log_videos_on_the_device(tmp_path):
  log = logger_lib.UniversalLogger(str(tmp_path), step=0)
  pair = _dev(np.stack([_colour(3, 16, 24, 20), _colour(3, 16, 24, 21)]))
  depth = _dev(R.noise((1, 2, 9, 13, 1), 22))
  log.log_videos(5, fps=20, rollout=pair, depth=depth)
  with pytest.raises(ValueError):
    log.log_videos(6, bad=pair.cpu().numpy())
  log.close()
  values = {}
  for _, step, v in tf_events.read_events(log.summary_writer.path):
    assert step in (0, 5)
    values.update(v)
  want = gif.encode_gif_batch([depth[0], pair[0], pair[1]], fps=20)
  assert sorted(values) == ['depth', 'rollout/video/0', 'rollout/video/1']
  assert values['depth'] == (9, 13, want[0])
  assert values['rollout/video/0'] == (16, 24, want[1]) and values['rollout/video/1'] == (16, 24, want[2])


def _files_under(root):
  return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_gan_manager_test_writes_rollout_videos(tmp_path):
  """The smallest configuration of tests/test_gan_test_loop_gpu.py."""
  import _video_input_ref as ref
  import test_gan_test_loop_gpu as loop
  from se3ds_amd import gin_lite
  from se3ds_amd.utils import inception_utils as iu
  examples = ref.synth_examples(2 * loop.BATCH, loop.T, 2 * loop.SIZE, seed=31)
  inception = iu.inception_model(init='random', seed=12, device=DEV)
  with_video = str(tmp_path / 'model')
  root = os.path.join('images', loop.SPLIT, '1')
  pngs = sorted(os.path.join(root, str(f), f'{e}_{s}.png')
                for f in range(loop.SEQ) for e in range(loop.BATCH) for s in ('rgb', 'depth'))
  gifs = sorted(os.path.join(root, f'{e}_{s}.gif') for e in range(loop.BATCH) for s in ('rgb', 'depth'))
  try:
    gan = loop._make_gan(with_video)
    # frechet='device': the scores are not what is tested here, and the host's sqrtm takes seconds
    gan.test(eval_examples=examples, unit_test=True, inception=inception, frechet='device')
    # without the flag: PNGs and the score file, as before
    assert _files_under(with_video) == sorted(pngs + [f'scores_{loop.SPLIT}.csv'])
    log = logger_lib.UniversalLogger(str(tmp_path / 'events'), step=0)
    gan.test(eval_examples=examples, unit_test=True, inception=inception, frechet='device', rollout_video=True,
             logger=log)
    log.close()
  finally:
    gin_lite.clear_config()
  assert _files_under(with_video) == sorted(pngs + gifs + [f'scores_{loop.SPLIT}.csv'])
  for e in range(loop.BATCH):
    for suffix in ('rgb', 'depth'):
      with open(os.path.join(with_video, root, f'{e}_{suffix}.gif'), 'rb') as f:
        got = R.decode_file(f.read())
      assert got['frames'].shape == (loop.SEQ, loop.SIZE, 2 * loop.SIZE) and got['delays'] == [10] * loop.SEQ
      frames = []
      for k in range(loop.SEQ):
        with open(os.path.join(with_video, root, str(k), f'{e}_{suffix}.png'), 'rb') as f:
          frames.append(ref.decode_png(f.read()))
      video = np.stack(frames)
      if suffix == 'depth':
        assert np.array_equal(got['frames'][..., None], video)       # grey: exact
      else:
        palette, index = R.quantise(video, 32)
        assert np.array_equal(got['palette'], palette) and np.array_equal(got['frames'], index)
  tags = set()
  for _, _, values in tf_events.read_events(log.summary_writer.path):
    tags.update(t for t, v in values.items() if isinstance(v, tuple) and v[2][:6] == b'GIF89a')
  want = {f'{loop.SPLIT}_{m}_generated_video' + (f'/video/{i}' if loop.BATCH > 1 else '')
          for m in ('raw', 'ema') for i in range(min(loop.BATCH, 3))}
  assert tags == want
