"""se3ds_amd.utils.utils on the device: the two passes of nearest_neighbor_inpaint apart and
together, and the two sequence reductions.  Recorded, not gated: there is no earlier implementation
to race, and the reference's pairwise inpaint cannot run at these sizes.

Inpaint: uint8 label panoramas at 512 x 1024 and 1024 x 2048, N = 1 and 8, for three hole patterns:
  room    proj_semantic of the project's own warp: the box room of bench.py, unprojected and splatted
          at a 0.5 m offset -- the holes users will feed it
  half    half the pixels void at random
  single  one non-void pixel: the worst case of the column pass's outward scan
Reductions: compute_sequence_accuracy on (1, 8, 512, 1024) uint8 labels and compute_sequence_iou on
their (1, 8, 512, 1024, 42) one-hot encodings, with the bytes they must read per second set against
the HBM peak.

Timing: device events after warm-up, median over `rounds` windows of at least `iters` calls and at
least 20 ms each; the min / max over the windows is the spread a figure has to be read against.  The
"both" figure is the public wrapper (its two allocations included), the passes are bare library
calls.  For scale only, never a gate: the host time of
scipy.ndimage.distance_transform_edt(return_indices=True) on the same masks (field `context_only`,
absent when SciPy is not importable).

  python tools/semantic_utils_bench.py [--rounds 5] [--iters 10] [--out profiles/semantic_utils_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  the room scene of the flagship workload
from se3ds_amd import _lib, constants  # noqa: E402
from se3ds_amd.utils import pano_utils  # noqa: E402
from se3ds_amd.utils import utils as U  # noqa: E402

DEV = torch.device('cuda:0')
HBM_PEAK = 8.0e12   # bytes / s, MI355X data sheet
DEPTH_SCALE = 20.0


def room_semantic(h, w, n):
  """(n, h, w) uint8 proj_semantic: a label panorama of the box room, warped 0.5 m along x."""
  out = []
  for k in range(n):
    rng = np.random.default_rng(100 + k)
    pos = np.zeros(3)
    depth = bench._room_depth(rng, h, w, pos)
    # labels 1..40 in blocks of 32 x 32 pixels: regions, as a segmentation has them
    blocks = rng.integers(1, 41, (h // 32 + 1, w // 32 + 1))
    sem = np.kron(blocks, np.ones((32, 32), np.int64))[:h, :w].astype(np.int32).reshape(1, h, w, 1)
    xyz1, feats = pano_utils.equirectangular_to_pointcloud(
        torch.from_numpy(sem).to(DEV), torch.from_numpy(depth).to(DEV), constants.INVALID_SEM_VALUE, DEPTH_SCALE)
    offset = torch.tensor([[0.5, 0.0, 0.0]], dtype=torch.float32, device=DEV)
    _, proj = pano_utils.project_feats_to_equirectangular(feats, xyz1, h, w, constants.INVALID_SEM_VALUE,
                                                          DEPTH_SCALE, offset=offset)
    out.append(proj.reshape(h, w).to(torch.uint8))
  return torch.stack(out).contiguous()


def patterns(h, w, n):
  g = torch.Generator(device=DEV).manual_seed(h + n)
  labels = torch.randint(1, 41, (n, h, w), device=DEV, generator=g, dtype=torch.uint8)
  half = torch.where(torch.rand((n, h, w), device=DEV, generator=g) < 0.5, torch.zeros_like(labels), labels)
  single = torch.zeros_like(labels)
  single[:, h // 3, w // 5] = 7
  return dict(room=room_semantic(h, w, n), half=half, single=single)


MIN_WINDOW_MS = 20.0   # a shorter timed window measures the clock and the scheduler


def time_ms(fn, iters, rounds):
  """(median, min, max) ms per call over `rounds` windows between two device events; a window holds
  at least `iters` calls and enough of them to last MIN_WINDOW_MS (sized from one trial window)."""
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

  def window(calls):
    e0.record()
    for _ in range(calls):
      fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls

  trial = window(iters)
  calls = int(min(20000, max(iters, np.ceil(MIN_WINDOW_MS / max(trial, 1e-4)))))
  got = [window(calls) for _ in range(rounds)]
  return float(np.median(got)), float(min(got)), float(max(got)), calls


def inpaint_case(image, iters, rounds):
  L = _lib.lib()
  n, h, w = image.shape
  out = torch.empty_like(image)
  ws = torch.empty((int(L.se3ds_nn_inpaint_workspace_bytes(n, h, w)),), dtype=torch.uint8, device=DEV)

  def phase(which):
    _lib.check(L.se3ds_nn_inpaint(image.data_ptr(), _lib.U8, 0, n, h, w, out.data_ptr(), None, ws.data_ptr(),
                                  ws.numel(), which, _lib.stream()), 'nn_inpaint')

  both = lambda: U.nearest_neighbor_inpaint(image, 0)
  assert torch.equal(both(), (phase(3), out)[1])          # the wrapper and the phases agree
  filled = out.clone()
  void_share = float((image == 0).float().mean())
  assert void_share == 1.0 or int((filled == 0).sum()) == 0
  for fn in (lambda: phase(1), lambda: phase(2), both):    # warm-up
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  rows, cols, whole = (time_ms(f, iters, rounds) for f in (lambda: phase(1), lambda: phase(2), both))
  return dict(void_share=void_share, row_pass_ms=rows[0], column_pass_ms=cols[0], both_ms=whole[0],
              row_pass_ms_min_max=rows[1:3], column_pass_ms_min_max=cols[1:3], both_ms_min_max=whole[1:3],
              calls_per_window=[rows[3], cols[3], whole[3]])


def edt_context(image):
  try:
    from scipy import ndimage
  except ImportError:
    return None
  hole = (image[0] == 0).cpu().numpy()
  t0 = time.perf_counter()
  ndimage.distance_transform_edt(hole, return_indices=True)
  return dict(what='host scipy.ndimage.distance_transform_edt(return_indices=True), one image, one run',
              host_ms=1e3 * (time.perf_counter() - t0))


def reductions(iters, rounds):
  n, t, h, w, c = 1, 8, 512, 1024, 42
  g = torch.Generator(device=DEV).manual_seed(3)
  pred = torch.randint(0, c, (n, t, h, w), device=DEV, generator=g, dtype=torch.uint8)
  gt = torch.where(torch.rand((n, t, h, w), device=DEV, generator=g) < 0.7, pred, pred.roll(1, 3))
  mask = torch.ones((n, t), device=DEV)
  hot_p = torch.nn.functional.one_hot(pred.long(), c).float()
  hot_g = torch.nn.functional.one_hot(gt.long(), c).float()
  a = U.sequence_iou_from_labels(pred, gt, mask)
  b = U.compute_sequence_iou(hot_p, hot_g, mask)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])     # the two routes agree bit for bit
  out = {}
  for name, fn, nbytes in (('labels', lambda: U.compute_sequence_accuracy(pred, gt, mask), 2 * pred.numel()),
                           ('one_hot', lambda: U.compute_sequence_iou(hot_p, hot_g, mask), 8 * hot_p.numel())):
    for _ in range(2):
      fn()
    torch.cuda.synchronize()
    ms, lo, hi, calls = time_ms(fn, iters, rounds)
    out[name] = dict(shape=[n, t, h, w] + ([c] if name == 'one_hot' else []), ms=ms, ms_min_max=[lo, hi],
                     calls_per_window=calls,
                     bytes_read=nbytes, bytes_per_s=nbytes / (ms * 1e-3), share_of_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK)
    print(f'{name:8s} {ms:8.3f} ms  {nbytes / 1e6:8.1f} MB  {100 * out[name]["share_of_hbm_peak"]:5.1f} % of '
          f'{HBM_PEAK / 1e12:.1f} TB/s', flush=True)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  results = []
  for h in (512, 1024):
    w = 2 * h
    for n in (1, 8):
      for name, image in patterns(h, w, n).items():
        # the single-pixel scan is long: fewer calls per round
        r = inpaint_case(image, max(1, a.iters // 5) if name == 'single' else a.iters, a.rounds)
        r.update(pattern=name, batch=n, size=[h, w])
        if n == 1:
          ctx = edt_context(image)
          if ctx is not None:
            r['context_only'] = ctx
        results.append(r)
        print(f'{name:7s} {h} x {w} N={n}: void {100 * r["void_share"]:5.1f} %  rows {r["row_pass_ms"]:8.3f} ms  '
              f'columns {r["column_pass_ms"]:9.3f} ms  both {r["both_ms"]:9.3f} ms', flush=True)
      torch.cuda.empty_cache()
  doc = dict(tool='tools/semantic_utils_bench.py', rounds=a.rounds, iters=a.iters, hbm_peak_bytes_per_s=HBM_PEAK,
             device=torch.cuda.get_device_name(0), inpaint=results, reductions=reductions(a.iters, a.rounds))
  print(json.dumps(doc))
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(doc, f, indent=1)


if __name__ == '__main__':
  main()
