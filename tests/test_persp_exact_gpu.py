"""The perspective and pano-rotation half of csrc/geom.hip on an MI355X, bit for bit.

Entry points: se3ds_rotate_coords, se3ds_perspective_coords, se3ds_persp_from_equirect_coords,
se3ds_perspective_to_pointcloud, se3ds_perspective_guidance, and the wrappers of
se3ds_amd/utils/pano_utils.py above them.  The yardstick is the pinned-order statement of
tests/_persp_ref.py: oracle/warp_np.py with every 3-term product written as ((a*b + c*d) + e*f), the
order geom.hip's comments state.  tests/test_persp_ref_cpu.py anchors that statement to the matmul
oracle, shows that its transcendentals equal the kernels' on every input used here, and that these
cases notice errors the 99.5 % bar of tests/test_warp_gpu.py lets through.

Every comparison is equality of bit patterns on every element; NaN must be NaN at the same place.
No query is excluded.  Direct calls write into a window of a larger buffer: the window starts as a
NaN with a payload no arithmetic produces, so an element that was never written is reported as
such, and the bands on both sides must keep their sentinel.  The cases (tests/_persp_cases.py) are
the smallest that cross each boundary: q in {1, 255, 256, 257} around the block of 256, one case
above 4096 x 256 queries per looping kernel (a thread's second trip through the grid-stride loop),
non-square views and sources both ways, n = 3 with three matrices, every flag value."""
import numpy as np
import pytest
import torch

from oracle import warp_np as W
from se3ds_amd import _lib
from se3ds_amd.utils import pano_utils
import _persp_cases as C
import _persp_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32 = np.float32
E_BADSHAPE = _lib.ABI['SE3DS_E_BADSHAPE']
GUARD = 64                     # elements on each side of a window
SENTINEL = 0x5EDA5EDA          # the guard bands
UNWRITTEN = 0x7FD5A5A5         # a quiet NaN with a payload: the window before the call

REACHED = {}


def reach(case_or_entry, classes=None, detail=''):
  entry = case_or_entry.entry if classes is None else case_or_entry
  for cls in (case_or_entry.classes if classes is None else classes):
    REACHED.setdefault((entry, cls), detail or getattr(case_or_entry, 'name', ''))


def host(a):
  """A writable copy for the wrappers (the cases' arrays are read-only)."""
  return None if a is None else np.array(a)


def t(a):
  return None if a is None else torch.from_numpy(np.array(a, order='C')).to(DEV)


class Window:
  """`shape` elements of 4 bytes inside a larger device buffer."""

  def __init__(self, shape, dtype=np.float32):
    self.shape, self.dtype = tuple(shape), dtype
    self.n = int(np.prod(shape))
    self.flat = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    self.flat[GUARD:GUARD + self.n] = UNWRITTEN

  def ptr(self):
    return self.flat.data_ptr() + 4 * GUARD

  def result(self, what):
    torch.cuda.synchronize()
    host = self.flat.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), f'{what}: guard band overwritten'
    body = host[GUARD:GUARD + self.n]
    skipped = np.flatnonzero(body == UNWRITTEN)
    assert skipped.size == 0, f'{what}: {skipped.size} of {self.n} elements never written, first at {int(skipped[0])}'
    return body.view(self.dtype).reshape(self.shape)


def same_bits(got, want, what):
  bad = C.first_mismatch(got, want)
  assert bad is None, f'{what}: {bad}'


def ids(cases):
  return [c.name for c in cases]


def grouped(entry, count):
  """The non-looped cases of `entry`, grouped by their first `count` classes after the trip."""
  groups = {}
  for c in C.cases_of(entry):
    if 'looped' not in c.classes:
      key = '-'.join([cls for cls in c.classes if cls != 'single trip'][:count]).replace(' = ', '').replace(' ', '-')
      groups.setdefault(key, []).append(c)
  return groups


def looped(entry):
  return [c for c in C.cases_of(entry) if 'looped' in c.classes]


# ------------------------------------------------------------------ coordinate kernels, direct
@pytest.mark.parametrize('case', C.cases_of('rotate_coords'), ids=ids(C.cases_of('rotate_coords')))
def test_rotate_coords_direct(case):
  """n = 3 with three matrices in one call, a source panorama that is not the ray grid, arbitrary
  unit rays; the scaled matrix drives |y| > 1 into acos: NaN, at the statement's places."""
  inp = case.inputs
  rays, matrix = t(inp['rays']), t(inp['matrix'])
  n, q = matrix.shape[0], rays.shape[1]
  out = Window((n, q, 2))
  rc = _lib.lib().se3ds_rotate_coords(rays.data_ptr(), matrix.data_ptr(), n, q, inp['src_h'], inp['src_w'],
                                      out.ptr(), _lib.stream())
  assert rc == 0, rc
  got = out.result(case.id)
  same_bits(got, case.want(), case.id)
  assert C.first_mismatch(got[2], got[0]) is not None, 'batch 2 has its own values'
  reach(case)
  reach('rotate_coords', ['guard bands'], case.name)


@pytest.mark.parametrize('case', C.cases_of('perspective_coords'), ids=ids(C.cases_of('perspective_coords')))
def test_perspective_coords_direct(case):
  """Both roundings and both `add` values; exact k + 0.5 ties of both parities and signs; z of
  +0, -0, negative and denormal (the -1 branch, -1 + add after the addition)."""
  inp = case.inputs
  rays, w2i = t(inp['rays']), t(inp['world_to_image'])
  q = rays.shape[1]
  out = Window((q, 2))
  rc = _lib.lib().se3ds_perspective_coords(rays.data_ptr(), w2i.data_ptr(), q, int(inp['round_to_nearest']),
                                           float(inp['add']), out.ptr(), _lib.stream())
  assert rc == 0, rc
  same_bits(out.result(case.id), case.want(), case.id)
  reach(case)
  reach('perspective_coords', ['guard bands'], case.name)


@pytest.mark.parametrize('case', C.cases_of('persp_from_equirect_coords'),
                         ids=ids(C.cases_of('persp_from_equirect_coords')))
def test_persp_from_equirect_coords_direct(case):
  """Views 1 x 1, one row, one thin column, wide and tall; fx != fy, cx != cy."""
  inp = case.inputs
  kinv_t, rot = t(inp['kinv_t']), t(inp['rotation_matrix'])
  out = Window((inp['height'] * inp['width'], 2))
  rc = _lib.lib().se3ds_persp_from_equirect_coords(kinv_t.data_ptr(), rot.data_ptr(), inp['height'], inp['width'],
                                                   inp['eq_h'], inp['eq_w'], out.ptr(), _lib.stream())
  assert rc == 0, rc
  same_bits(out.result(case.id), case.want(), case.id)
  reach(case)
  reach('persp_from_equirect_coords', ['guard bands'], case.name)


# ---------------------------------------------------------------------------------- wrappers
@pytest.mark.parametrize('case', C.cases_of('rotate_pano'), ids=ids(C.cases_of('rotate_pano')))
def test_rotate_pano(case):
  inp = case.inputs
  got = pano_utils.rotate_pano(t(inp['pano']), t(inp['matrix'])).cpu().numpy()
  same_bits(got, case.want(), case.id)
  reach(case)


_PROJECT = grouped('project_perspective_image', 2)


@pytest.mark.parametrize('group', list(_PROJECT))
def test_project_perspective_image(group):
  """Sources 17 x 24 and 24 x 17, outputs 16 and 33 rows, all three pad modes (constant 0 and
  0.25), both roundings, intrinsics and fov + rotations."""
  assert len(_PROJECT[group]) == 32
  for case in _PROJECT[group]:
    inp = {k: host(v) if isinstance(v, np.ndarray) else v for k, v in case.inputs.items()}
    image = t(inp.pop('image'))
    got = pano_utils.project_perspective_image(image, inp.pop('fov'), inp.pop('output_height'), **inp).cpu().numpy()
    same_bits(got, case.want(), case.id)
    reach(case)


@pytest.mark.parametrize('case', C.cases_of('get_perspective_from_equirectangular_image'),
                         ids=ids(C.cases_of('get_perspective_from_equirectangular_image')))
def test_get_perspective_from_equirectangular_image(case):
  inp = case.inputs
  got = pano_utils.get_perspective_from_equirectangular_image(
      t(inp['image']), host(inp['camera_intrinsics']), host(inp['rotation_matrix']), inp['height'],
      inp['width']).cpu().numpy()
  same_bits(got, case.want(), case.id)
  reach(case)


# ------------------------------------------------------------------------------ fused kernels
def _pointcloud(case):
  """One cell-15 case through the raw entry point (windows, the oracle's rays and angle tables)
  and through the wrapper."""
  inp = case.inputs
  image, depth = t(inp['image01']), t(inp['depth01'])
  ih, iw, c = image.shape
  h = inp['eq_height']
  w = 2 * h
  want_xyz, want_feats = case.want()
  rays = t(W.equirectangular_pixel_rays(h))
  w2i = t(W.get_world_to_image_transform((ih, iw), None, camera_intrinsics=inp['camera_intrinsics'],
                                         rotation_matrix=inp['rotation_matrix']))
  tables = [t(a) for a in W.equirect_angle_tables(h, w)]
  position = t(inp['position'])
  xyz1, feats = Window((1, 4, h * w)), Window((1, h * w, c), np.int32)
  rc = _lib.lib().se3ds_perspective_to_pointcloud(
      image.data_ptr(), depth.data_ptr(), ih, iw, c, rays.data_ptr(), w2i.data_ptr(), int(inp['round_to_nearest']),
      float(inp['pad_value']), *[a.data_ptr() for a in tables], _lib.ptr(position), h, w, float(inp['void_class']),
      float(inp['depth_scale']), xyz1.ptr(), feats.ptr(), _lib.stream())
  assert rc == 0, rc
  same_bits(xyz1.result(case.id), want_xyz, f'{case.id} xyz1')
  same_bits(feats.result(case.id), want_feats, f'{case.id} feats')
  got_xyz, got_feats = pano_utils.perspective_to_pointcloud(
      image, depth, h, inp['void_class'], inp['depth_scale'], camera_intrinsics=host(inp['camera_intrinsics']),
      rotation_matrix=host(inp['rotation_matrix']), pad_value=inp['pad_value'],
      round_to_nearest=inp['round_to_nearest'],
      position=None if position is None else position[None])
  same_bits(got_xyz.cpu().numpy(), want_xyz, f'{case.id} wrapper xyz1')
  same_bits(got_feats.cpu().numpy(), want_feats, f'{case.id} wrapper feats')
  reach(case)
  reach('perspective_to_pointcloud', ['guard bands'], case.name)


_POINTCLOUD = grouped('perspective_to_pointcloud', 2)


@pytest.mark.parametrize('group', list(_POINTCLOUD))
def test_perspective_to_pointcloud(group):
  """Sources 17 x 24 and 24 x 17 with 1 to 4 channels onto 16 x 32 and 128 x 256: position or
  none, both roundings, padding 0 and 0.25, void class -1; the source depths hold exact 0 and 1."""
  assert len(_POINTCLOUD[group]) == 16
  for case in _POINTCLOUD[group]:
    _pointcloud(case)


def test_perspective_to_pointcloud_second_trip():
  """725 x 1450 > 4096 x 256 points: every thread of the capped grid takes a second trip."""
  (case,) = looped('perspective_to_pointcloud')
  assert case.inputs['eq_height'] * 2 * case.inputs['eq_height'] > C.ONE_TRIP
  _pointcloud(case)


@pytest.mark.parametrize('case', C.cases_of('perspective_guidance'), ids=ids(C.cases_of('perspective_guidance')))
def test_perspective_guidance(case):
  """Hand-placed taps (depth exactly 0 and 1, a zero channel, RGB above 255), the oracle's splat of
  the notebook chain, and 1024 x 1025 views for the second trip; all three outputs, raw and wrapped."""
  inp = case.inputs
  rgb, depth = t(inp['pred_rgb']), t(inp['pred_depth'])
  eh, ew = depth.shape
  h, w = inp['pers_height'], inp['pers_width']
  want = case.want()
  kinv_t, rot = t(R.inverse_intrinsics_t(inp['camera_intrinsics'])), t(inp['new_rotation_matrix'])
  outs = [Window((1, h, w, 3)), Window((1, h, w, 1)), Window((1, h, w, 1))]
  rc = _lib.lib().se3ds_perspective_guidance(rgb.data_ptr(), depth.data_ptr(), eh, ew, kinv_t.data_ptr(),
                                             rot.data_ptr(), h, w, *[o.ptr() for o in outs], _lib.stream())
  assert rc == 0, rc
  names = ('proj_image', 'proj_depth', 'proj_mask')
  for name, o, b in zip(names, outs, want):
    same_bits(o.result(f'{case.id} {name}'), b, f'{case.id} {name}')
  got = pano_utils.perspective_guidance(rgb, depth, host(inp['camera_intrinsics']),
                                       host(inp['new_rotation_matrix']), h, w)
  for name, a, b in zip(names, got, want):
    same_bits(a.cpu().numpy(), b, f'{case.id} wrapper {name}')
  reach(case)
  reach('perspective_guidance', ['guard bands'], case.name)


# --------------------------------------------------------------------------------- refusals
def test_refusals_return_badshape():
  """Each entry point refuses an empty or impossible shape before it launches anything: valid
  pointers, windows that must stay untouched."""
  L = _lib.lib()
  s = _lib.stream()
  buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
  p = buf.data_ptr()
  out = Window((64,))
  o = out.ptr()
  calls = {
      'rotate_coords': [('q = 0', lambda: L.se3ds_rotate_coords(p, p, 1, 0, 8, 16, o, s)),
                        ('n = 0', lambda: L.se3ds_rotate_coords(p, p, 0, 4, 8, 16, o, s))],
      'perspective_coords': [('q = 0', lambda: L.se3ds_perspective_coords(p, p, 0, 1, 1.0, o, s))],
      'persp_from_equirect_coords': [
          ('height = 0', lambda: L.se3ds_persp_from_equirect_coords(p, p, 0, 4, 8, 16, o, s)),
          ('width = 0', lambda: L.se3ds_persp_from_equirect_coords(p, p, 4, 0, 8, 16, o, s))],
      'perspective_to_pointcloud': [
          ('channels = 5', lambda: L.se3ds_perspective_to_pointcloud(p, p, 4, 4, 5, p, p, 1, 0.0, p, p, p, p, None, 2,
                                                                     4, -1.0, 20.0, o, o, s)),
          ('channels = 0', lambda: L.se3ds_perspective_to_pointcloud(p, p, 4, 4, 0, p, p, 1, 0.0, p, p, p, p, None, 2,
                                                                     4, -1.0, 20.0, o, o, s)),
          ('width != 2 height', lambda: L.se3ds_perspective_to_pointcloud(p, p, 4, 4, 3, p, p, 1, 0.0, p, p, p, p,
                                                                          None, 2, 5, -1.0, 20.0, o, o, s)),
          ('source height = 0', lambda: L.se3ds_perspective_to_pointcloud(p, p, 0, 4, 3, p, p, 1, 0.0, p, p, p, p,
                                                                          None, 2, 4, -1.0, 20.0, o, o, s))],
      'perspective_guidance': [
          ('eq_h = 1', lambda: L.se3ds_perspective_guidance(p, p, 1, 16, p, p, 2, 2, o, o, o, s)),
          ('height = 0', lambda: L.se3ds_perspective_guidance(p, p, 8, 16, p, p, 0, 2, o, o, o, s))],
  }
  for entry, refusals in calls.items():
    for what, call in refusals:
      assert call() == E_BADSHAPE, (entry, what)
    reach(entry, ['BADSHAPE'], ', '.join(w for w, _ in refusals))
  torch.cuda.synchronize()
  host = out.flat.cpu().numpy()
  assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
  assert (host[GUARD:-GUARD] == UNWRITTEN).all(), 'a refused call wrote to its output'


# --------------------------------------------------------------------------- coverage table
def test_reached_classes():
  """Prints which classes each entry point was driven through; the table must be complete (run the
  whole module: every test fills it)."""
  expected = {e: list(c) for e, c in C.EXPECTED_CLASSES.items()}
  for entry in ('rotate_coords', 'perspective_coords', 'persp_from_equirect_coords', 'perspective_to_pointcloud',
                'perspective_guidance'):
    expected[entry] += ['guard bands', 'BADSHAPE']
  for (entry, cls), detail in sorted(REACHED.items()):
    print(f'{entry:44s} {cls:20s} {detail}')
  missing = [(e, c) for e, classes in expected.items() for c in classes if (e, c) not in REACHED]
  assert not missing, f'classes not reached: {missing}'
