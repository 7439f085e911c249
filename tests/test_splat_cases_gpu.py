"""The z-buffer splat (se3ds_amd/csrc/geom.hip: scatter, binned, 20-byte three-pass, packed, sorted)
on CONSTRUCTED clouds (tests/_splat_cases.py), bit for bit against oracle/warp_c.py and
oracle/warp_np.py.  The random clouds of tests/test_warp_gpu.py reach every route but cannot show
three things: a `<=` or a differently rounded edge in the 0.1 tolerance (no random point lies
within ulps of fl(zmin + 0.1f)), a route that drops one chunk's, image's, tile's or tail's
contribution to the sink pixel (random byte features saturate the sink at 255), and points of which
only some channels are void.  Each case plants exactly that at every row of the route table; the
stated values at the planted pixels and at the sink are checked next to the whole-image
comparison, so a failure names the case.  tests/test_splat_cases_cpu.py guards the builder."""
import os

import numpy as np
import pytest
import torch

from oracle import warp_c
from oracle import warp_np
from se3ds_amd.utils import pano_utils
from se3ds_amd.utils import point_cloud_utils
import _splat_cases as S

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev():
  assert torch.cuda.is_available(), 'GPU tests need an MI355X'
  return torch.device('cuda:0')


def t(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def compare(rid, label, got, want_c, want_np, notes, mask_void):
  d_g, f_g, m_g = (x.cpu().numpy() for x in got)
  # the stated values first: their message names the case, the planted pixel and what it shows
  S.check_expected(notes, d_g, f_g, f'device, {rid}')
  for name, (d_o, f_o) in (('warp_c', want_c), ('warp_np', want_np)):
    np.testing.assert_array_equal(d_g, d_o, err_msg=f'depth vs {name}, {label}')
    np.testing.assert_array_equal(f_g, f_o, err_msg=f'features vs {name}, {label}')
  np.testing.assert_array_equal(m_g[..., None], warp_np.proj_mask(want_np[0], want_np[1], mask_void),
                                err_msg=f'mask, {label}')


@pytest.mark.parametrize('case,row', S.CASE_ROWS, ids=S.CASE_ROW_IDS)
def test_constructed_cloud_bit_exact(case, row):
  rid, n, h, w, dtype, c, void, m = row
  for variant in S.variants(case, n, m):
    xyz1, feats, offset, notes = S.build(case, n, h, w, c, dtype, void, m, variant)
    label = f'{rid} {case} {S.variant_id(variant)}'
    rel = (xyz1 - np.concatenate([offset, np.zeros((n, 1), F32)], 1)[:, :, None]).astype(F32)
    want_np = warp_np.project_feats_to_equirectangular(feats, rel, h, w, void, S.DEPTH_SCALE)
    want_c = warp_c.project_feats_to_equirectangular(feats, xyz1, h, w, void, S.DEPTH_SCALE, offset=offset)
    got = pano_utils.project_feats_to_equirectangular(t(feats), t(xyz1), h, w, void, S.DEPTH_SCALE,
                                                      offset=t(offset), with_mask=True, mask_void=void)
    compare(rid, label, got, want_c, want_np, notes, void)


@pytest.mark.parametrize('row', S.ROWS, ids=S.ROW_IDS)
def test_border_cloud_bit_exact(row):
  """The perspective entry: view coordinates ON the image borders (fx = -1, -0.5, 0, k, k + 0.5,
  the float below W, W; the same in y; the oracle truncates toward zero), z = -1, z = +-0
  (div_no_nan), and an output void of -5 (with float features and on the scatter row: the
  ordered-float kernels; on the byte rows it takes the call off the packed routes, so they keep 0)."""
  rid, n, h, w, dtype, c, void, m = row
  coords, feats, notes = S.build('borders', n, h, w, c, dtype, void, m)
  voids = (0.0, -5.0) if dtype == np.float32 or c > 7 else (0.0,)
  for output_void in voids:
    label = f'{rid} borders output void {output_void}'
    want_np = warp_np.project_to_feat(coords, feats, h, w, S.DEPTH_SCALE, void, output_void)
    want_c = warp_c.project_to_feat(coords, feats, h, w, S.DEPTH_SCALE, void, output_void)
    got = point_cloud_utils._splat('generic', t(coords), None, t(feats), h, w, S.DEPTH_SCALE, void,
                                   output_void, with_mask=True, mask_void=output_void)
    compare(rid, label, got, want_c, want_np, notes, output_void)
    d_p, f_p = point_cloud_utils.project_to_feat(t(coords), t(feats), h, w, S.DEPTH_SCALE, void, output_void)
    assert torch.equal(d_p, got[0]) and torch.equal(f_p, got[1]), label


_OLD = dict(SE3DS_SPLAT_PACKED='0')
_SORT = dict(SE3DS_SPLAT_SORT='2')
@pytest.mark.parametrize('env_extra', [
    dict(SE3DS_SPLAT_SLICE='48'),
    dict(_OLD, SE3DS_SPLAT_SLICE='48'),
    dict(_SORT, SE3DS_SPLAT_PTS='16'),
    dict(_SORT, SE3DS_SPLAT_PTS='8'),
    dict(_SORT, SE3DS_SPLAT_PTS='4'),
    dict(_SORT, SE3DS_SPLAT_SUPERPX='4096'),
    dict(_SORT, SE3DS_SPLAT_SUPERPX='512'),
], ids=['packed-banded', 'three-pass-banded', 'sorted-16pt', 'sorted-8pt', 'sorted-4pt', 'sorted-4096px',
        'sorted-512px'])
def test_constructed_clouds_in_child_processes_under_route_switches(env_extra):
  """The 48 x 96 rows of this module again, in a child process under each switch set of
  test_warp_gpu.py::test_splat_banded_tiles_bit_exact (the switches are read once per process):
  the 20-byte three-pass path, banded slices of the packed and binned resolves, and every template
  variant of the sort kernel meet the same clouds."""
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = dict(os.environ, PYTHONPATH=root, **env_extra)
  env.pop('SE3DS_SPLAT_SCATTER', None)
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(root, 'tests', 'test_splat_cases_gpu.py'),
                      '-q', '-x', '-m', 'gpu', '-k', '48x96 and not child'],
                     env=env, cwd=root, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
  assert ' passed' in r.stdout
