"""The two launches of RE10KImageDataset's device transform, timed on their own: N = 8 frames of
512 x 1024, image_size 256 and 512, re_10k_crop = random_crop = True, each mask a centred visible
rectangle of about half the frame with a ragged edge.

Per launch: device events around back-to-back launches on one stream after a warm-up, in a window
of at least `--window` seconds (so the figure for the small extent kernel includes what separates
two launches in a stream: it is an upper bound on the kernel).  Bytes are the ones the algorithm
needs, computed here from the shapes -- the mask once for the reduction; per output pixel the
4 taps x 3 B + 13 B read and the 40 B written that the header of csrc/input.hip lists -- and are
set against the HBM peak bench.py uses.  For the extent kernel the ratio to one pass over the mask
at that peak is printed, with the load path that ran.  The batch is checked against the restatement's
boxes (tests/_re10k_ref.py) before anything is timed.  Nothing here is a gate.

The kernels alone, without the gap between launches: the same tool with one size and a short window
under `rocprofv3 --kernel-trace --stats`, in a run of its own (tools/rocpd_summary.py prints the table).

  python tools/re10k_input_bench.py [--window 0.4] [--rounds 5] [--sizes 256,512] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from se3ds_amd import _lib  # noqa: E402
from se3ds_amd.datasets import indoor_datasets  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s: bench.py's HBM_PEAK_GBS
N, H0, W0 = 8, 512, 1024
READ_PER_PIXEL, WRITE_PER_PIXEL = 4 * 3 + 13, 40


def make_raw(dev):
  rng = np.random.default_rng(0)
  masks = np.zeros((N, H0, W0), np.uint8)
  for i, m in enumerate(masks):   # ~ half the frame: 0.7 x 0.7 of each side, edges ragged
    y0, x0 = int(0.15 * H0) + i, int(0.15 * W0) - 2 * i
    m[y0:y0 + int(0.7 * H0), x0:x0 + int(0.7 * W0)] = 255
    m[y0, x0:x0 + int(0.7 * W0)] = rng.integers(0, 2, int(0.7 * W0), dtype=np.uint8)
  u8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
  raw = dict(image=u8(N, H0, W0, 3), proj_image=u8(N, H0, W0, 3),
             depth=rng.integers(0, 65536, (N, H0, W0)).astype(np.uint16).view(np.int16),
             proj_depth=rng.integers(0, 65536, (N, H0, W0)).astype(np.uint16).view(np.int16),
             proj_mask=u8(N, H0, W0), visible_mask=masks, segmentation=u8(N, H0, W0) % 42)
  return masks, {k: torch.from_numpy(v).to(dev) for k, v in raw.items()}


def time_ms(fn, window, rounds):
  """Median over `rounds` of the time per call, each round a window of >= `window` seconds."""
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

  def run(iters):
    e0.record()
    for _ in range(iters):
      fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters
  for _ in range(20):
    fn()
  probe = run(200)
  iters = int(min(max(200, window * 1e3 / max(probe, 1e-4)), 500000))
  return float(np.median([run(iters) for _ in range(rounds)])), iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--window', type=float, default=0.4)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--sizes', default='256,512', help='image_size values, comma separated')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('re10k_input_bench needs an MI355X: there is nothing to time without one')
  import _re10k_ref
  dev = torch.device('cuda:0')
  L = _lib.lib()
  masks, raw = make_raw(dev)
  mask_bytes = N * H0 * W0
  vector_bytes = L.se3ds_re10k_extent_vector_bytes(_lib.ptr(raw['visible_mask']), W0)
  results = []
  for size in (int(s) for s in a.sizes.split(',')):
    ds = indoor_datasets.RE10KImageDataset(image_size=size, preprocessed_image_height=H0,
                                           re_10k_crop=True)
    rng = np.random.default_rng(7)
    params = [ds.draw_params(rng, H0, W0) for _ in range(N)]
    out = ds.device_transform(raw, params)
    want = [_re10k_ref.box(*_re10k_ref.extents(m), H0, W0, p['pad'], p['x_shift'], p['y_shift'])
            for m, p in zip(masks, params)]
    assert out['bbox'].tolist() == [b for b, _ in want] and all(s == 0 for _, s in want)
    h, w = size, 2 * size
    ext = torch.from_numpy(np.tile(np.array([H0, -1, W0, -1], np.int32), (N, 1))).to(dev)
    ip = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    ip[:, 2] = 1
    fp = torch.tensor([[0, 0, 0, 0, p['pad'], p['x_shift'], p['y_shift']] for p in params],
                      dtype=torch.float32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    stream = _lib.stream()
    ext_args = (_lib.ptr(raw['visible_mask']), N, H0, W0, _lib.ptr(ext), stream)
    xf_args = tuple(_lib.ptr(raw[k]) for k in indoor_datasets.RE10K_RAW_DTYPES) + (
        _lib.ptr(ext), _lib.ptr(ip), _lib.ptr(fp), N, H0, W0, h, w) + tuple(
            _lib.ptr(out[k]) for k in ('image', 'proj_image', 'proj_mask', 'proj_depth', 'depth',
                                       'blurred_mask', 'segmentation', 'bbox')) + (_lib.ptr(status), stream)

    def extent():
      assert L.se3ds_re10k_extent(*ext_args) == 0

    def transform():
      assert L.se3ds_re10k_transform(*xf_args) == 0
    ext_ms, ext_iters = time_ms(extent, a.window, a.rounds)
    xf_ms, xf_iters = time_ms(transform, a.window, a.rounds)
    assert status.tolist() == [0] * N
    px = N * h * w
    xf_bytes = px * (READ_PER_PIXEL + WRITE_PER_PIXEL)
    floor_ms = mask_bytes / HBM_PEAK * 1e3
    r = dict(batch=N, src=[H0, W0], dst=[h, w], extent_ms=ext_ms, extent_launches_per_round=ext_iters,
             extent_bytes=mask_bytes, extent_vector_bytes=vector_bytes,
             extent_share_of_hbm_peak=mask_bytes / (ext_ms * 1e-3) / HBM_PEAK,
             extent_over_one_pass_at_peak=ext_ms / floor_ms, transform_ms=xf_ms,
             transform_launches_per_round=xf_iters, transform_bytes=xf_bytes,
             transform_share_of_hbm_peak=xf_bytes / (xf_ms * 1e-3) / HBM_PEAK)
    results.append(r)
    print(f'{N} x {H0}x{W0} -> {h}x{w}: extent {1e3 * ext_ms:7.2f} us ({mask_bytes / 1e6:.1f} MB, '
          f'{vector_bytes}-byte path, {ext_ms / floor_ms:5.1f} x one pass at {HBM_PEAK / 1e12:.0f} TB/s)  '
          f'transform {1e3 * xf_ms:8.2f} us ({xf_bytes / 1e6:6.1f} MB, '
          f'{100 * r["transform_share_of_hbm_peak"]:4.1f} % of peak)', flush=True)
  doc = dict(tool='tools/re10k_input_bench.py', window_s=a.window, rounds=a.rounds,
             hbm_peak_bytes_per_s=HBM_PEAK, device=torch.cuda.get_device_name(0), results=results)
  print(json.dumps(doc))
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(doc, f, indent=1)


if __name__ == '__main__':
  main()
