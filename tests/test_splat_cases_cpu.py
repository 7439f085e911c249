"""The constructed splat clouds (tests/_splat_cases.py) on the CPU: every case builds at every row
of the route table with its preconditions holding on the oracle's own view, the two oracles
(oracle/warp_np.py, NumPy scatters and libm; oracle/warp_c.py, the plain-C twin) agree bit for bit
on them, and both return the values the cases state for the planted pixels and the sink.  This
guards the builder: tests/test_splat_cases_gpu.py compares the kernels with the same clouds."""
import numpy as np
import pytest

from oracle import warp_c
from oracle import warp_np
import _splat_cases as S

F32 = np.float32


def oracles(case, row, variant, output_void=0.0):
  """(inputs, notes, depth, feats) of a case: both oracles, asserted equal."""
  _, n, h, w, dtype, c, void, m = row
  if case == 'borders':
    coords, feats, notes = S.build(case, n, h, w, c, dtype, void, m, variant)
    d_n, f_n = warp_np.project_to_feat(coords, feats, h, w, S.DEPTH_SCALE, void, output_void)
    d_c, f_c = warp_c.project_to_feat(coords, feats, h, w, S.DEPTH_SCALE, void, output_void)
    inputs = (coords, feats)
  else:
    xyz1, feats, offset, notes = S.build(case, n, h, w, c, dtype, void, m, variant)
    rel = (xyz1 - np.concatenate([offset, np.zeros((n, 1), F32)], 1)[:, :, None]).astype(F32)
    d_n, f_n = warp_np.project_feats_to_equirectangular(feats, rel, h, w, void, S.DEPTH_SCALE)
    d_c, f_c = warp_c.project_feats_to_equirectangular(feats, xyz1, h, w, void, S.DEPTH_SCALE, offset=offset)
    inputs = (xyz1, feats, offset)
  label = f'{row[0]} {case} {S.variant_id(notes["variant"])}'
  np.testing.assert_array_equal(d_c, d_n, err_msg=label)
  np.testing.assert_array_equal(f_c, f_n, err_msg=label)
  return inputs, notes, d_n, f_n


@pytest.mark.parametrize('case,row', S.CASE_ROWS, ids=S.CASE_ROW_IDS)
def test_equirect_cases_build_and_the_oracles_return_the_stated_values(case, row):
  _, n, h, w, dtype, c, void, m = row
  for variant in S.variants(case, n, m):
    (xyz1, feats, offset), notes, depth, out = oracles(case, row, variant)
    assert xyz1.shape == (n, 4, m) and feats.shape == (n, m, c) and feats.dtype == dtype
    assert xyz1.dtype == F32 and offset.shape == (n, 3)
    S.check_expected(notes, depth, out, 'oracle ' + row[0])


@pytest.mark.parametrize('row', S.ROWS, ids=S.ROW_IDS)
def test_border_case_builds_and_the_oracles_agree(row):
  _, n, h, w, dtype, c, void, m = row
  for output_void in (0.0, -5.0):
    (coords, feats), notes, depth, out = oracles('borders', row, {}, output_void)
    assert coords.shape == (n, 4, m) and feats.shape == (n, m, c) and feats.dtype == dtype
    S.check_expected(notes, depth, out, 'oracle ' + row[0])
    assert depth.min() == 0.0 and depth.max() == 1.0
    # pixels no point reaches hold the output void
    reached = np.zeros(n * h * w, bool)
    reached[notes['flat'].reshape(-1)] = True
    assert (out.reshape(-1, c)[~reached] == F32(output_void)).all()


def test_planted_z_scan_hits_the_edge_and_its_predecessor():
  """The scan of point_with_z: both fl(z0 + 0.1f) and its predecessor are reachable as oracle radii
  inside one pixel, here and at the image's last pixel."""
  for h, w, v, u in ((48, 96, 20, 30), (48, 96, 47, 95), (256, 512, 255, 511), (32, 64, 8, 0)):
    for z0 in (F32(0.37), F32(2.0), F32(7.9), F32(S.DEPTH_SCALE)):
      edge = F32(z0 + S.TOL)
      for target in (edge, np.nextafter(edge, F32(0), dtype=F32)):
        p = S.point_with_z(h, w, v, u, target)
        idx, z = S.equirect_view(p[None], h, w)
        assert z[0] == target and idx[0] == v * w + u


def test_variants_reach_every_position_image_and_tile():
  for _, n, _, _, _, _, _, m in S.ROWS:
    vs = S.variants('sink_feat', n, m)
    assert {v['idx'] for v in vs} == set(S.sink_positions(m))
    assert {v['image'] for v in vs} == {0, n - 1}
    assert {(v['image'], v['tile']) for v in vs} == {(i, t) for i in {0, n - 1} for t in ('first', 'last')}
    assert sum(v['p0'] for v in vs) == 1
  assert S.sink_positions(20001) == [0, 20000, 10000, 2047, 2048, 4095, 4096, 8191, 8192]
