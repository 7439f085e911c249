"""The pinned-order statement of the perspective / rotation warps (tests/_persp_ref.py) and the
cases of tests/test_persp_exact_gpu.py (tests/_persp_cases.py), checked without a GPU.

a. Anchor.  The statement differs from oracle/warp_np.py in the order of its 3-term sums only, so
   the two agree closely on every query, the matrices of the GPU cases on the h = 32 and h = 64
   grids.  Measured (ANCHOR_MEASURED, asserted at 4 x, the margin for another BLAS):
     rotate_coords                     5.341e-05 px
     perspective_coords                1.351e-04 (|a - b| / max(1, |a|, |b|): the quotient x / z
                                       is unbounded towards the image plane's horizon)
     perspective_from_equirect_coords  1.526e-05 px
   Excepted, and counted from the two references alone: heading-seam queries (the two heading
   coordinates more than half the source width apart), pole queries whose x and z are both exact
   zeros in the pinned statement and whose headings differ (atan2 of two zeros follows their
   signs, and those follow the summation order), queries that one reference maps to NaN
   (|y| > 1 under the scaled matrix) or to the `z <= 0` branch and the other does not.  Measured
   share 0.187 % for rotate_coords and 0 for the other two; asserted <= 0.5 %, the share the bar tests of tests/test_warp_gpu.py allow.
b. The 48 signed permutation matrices with power-of-two intrinsics make every product exact, so
   both statements agree bit for bit wherever no rotated component is an exact zero (a zero takes
   its sign from the summation order).  On the h = 64 grid the excluded share is 1 / 64 = 1.5625 %
   for the two ray-grid functions (the pitch-0 row, where sin(0) = 0: 6144 of 393 216 queries; a
   grid of fewer than 50 rows would spend more than 2 % on that row alone) and 0 of 72 816 for the
   37 x 41 view; asserted <= 2 %.
c. On the arguments that every GPU case hands to atan2, acos and asin, warp_np's binary64-evaluated
   functions equal oracle.warp_c's, the C twin of the kernels' header, on every element
   (5 281 246 atan2, 3 165 886 acos and 2 115 360 asin arguments here, no disagreement).
d. Planted errors.  Each is put into one named step of the statement.  Its verdict under the bar
   of tests/test_warp_gpu.py (> 99.5 % within 1e-4, the old square shapes and seeds, against
   warp_np) is asserted as found, and the exact comparison on the new cases must notice it:
     decode-swap      width / height exchanged in the pixel decode        passes the bar (square views)
     tap-stride-swap  ih / iw exchanged in the fused tap address           passes the bar (square source)
     batch-matrix-0   batch element b given matrix 0                       FAILS the bar: the n = 2
                      rotate_pano test uses two different matrices, so half its pixels move
     last-unwritten   the last query left unwritten                        passes the bar (1 pixel)
     half-away        ties rounded away from zero, not to even             passes the bar (no tie occurs)
     inside-off-by-1  right / bottom in-bounds test `<` for `<=`           FAILS the bar on the covered
                      pixels (a 64 x 64 source loses 1 / 32 of them), passes on all pixels
     z-ge-0           `z >= 0` for `z > 0`                                 passes the bar (no exact zero)
e. Every case's preconditions: ties, NaN, signed zeros and denormals, exact depths, coverage."""
import contextlib

import numpy as np
import pytest

from oracle import warp_c
from oracle import warp_np as W
import _persp_cases as C
import _persp_ref as R

F32 = np.float32
ANCHOR_MEASURED = {'rotate_coords': 5.341e-05, 'perspective_coords': 1.351e-04,
                   'perspective_from_equirect_coords': 1.526e-05}
ANCHOR_MARGIN = 4.0
EXCEPTED_SHARE = 0.005


# -------------------------------------------------------------------------------- a. anchor
def _anchor_pairs():
  """(function, pinned (Q,2), warp_np (Q,2), heading column or None, source width, queries whose
  heading is undefined: x and z both exact zeros in the pinned statement, or None)."""
  out = []
  ks = (C.K_ODD, C.intrinsics(32, 32, 32, 32))
  for h, k, view in ((32, ks[0], 24), (64, ks[1], 64)):
    rays = W.equirectangular_pixel_rays(h)
    mats = np.stack(list(C.MATS.values()))
    pinned = R.rotate_coords(mats, rays, h, 2 * h)
    oracle = W.rotate_coords(mats, h, 2 * h, h)
    pole = np.stack([(x == 0) & (z == 0) for x, _, z in (R.mat_times_columns(m, rays) for m in mats)])
    out.append(('rotate_coords', pinned.reshape(-1, 2), oracle.reshape(-1, 2), 1, 2 * h, pole.reshape(-1)))
    for m in C.MATS.values():
      w2i = np.matmul(k, m).astype(F32)
      out.append(('perspective_coords', R.perspective_coords(w2i, rays), W.perspective_coords(w2i, h), None, 0, None))
      out.append(('perspective_from_equirect_coords',
                  R.perspective_from_equirect_coords(R.inverse_intrinsics_t(k), m, view, view, h, 2 * h),
                  W.perspective_from_equirect_coords(k, m, view, view, (h, 2 * h)), 0, 2 * h, None))
  return out


def _anchor_measure():
  worst = {k: 0.0 for k in ANCHOR_MEASURED}
  excepted = {k: [0, 0] for k in ANCHOR_MEASURED}
  for fn, a, b, heading, width, pole in _anchor_pairs():
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    nan = np.isnan(a64).any(-1) | np.isnan(b64).any(-1)
    exc = np.isnan(a64).any(-1) != np.isnan(b64).any(-1)
    with np.errstate(invalid='ignore'):
      if heading is not None:
        exc |= ~nan & (np.abs(a64[:, heading] - b64[:, heading]) > 0.5 * width)
        if pole is not None:
          exc |= pole & (a64[:, heading] != b64[:, heading])
        err = np.abs(a64 - b64).max(-1)
      else:
        behind_a, behind_b = np.all(a == F32(-1), -1), np.all(b == F32(-1), -1)
        exc |= behind_a != behind_b
        err = (np.abs(a64 - b64) / np.maximum(1.0, np.maximum(np.abs(a64), np.abs(b64)))).max(-1)
    keep = ~exc & ~nan
    worst[fn] = max(worst[fn], float(err[keep].max()))
    excepted[fn][0] += int(exc.sum())
    excepted[fn][1] += exc.size
  return worst, {k: v[0] / v[1] for k, v in excepted.items()}


def test_pinned_statement_is_anchored_to_the_matmul_oracle():
  worst, share = _anchor_measure()
  for fn in ANCHOR_MEASURED:
    print(f'{fn:34s} worst difference {worst[fn]:.3e} (recorded {ANCHOR_MEASURED[fn]:.3e}), '
          f'excepted share {share[fn]:.5f}')
  for fn in ANCHOR_MEASURED:
    assert share[fn] <= EXCEPTED_SHARE, (fn, share[fn])
    assert worst[fn] <= ANCHOR_MARGIN * ANCHOR_MEASURED[fn], (fn, worst[fn], ANCHOR_MEASURED[fn])


# ------------------------------------------------------------------ b. signed permutations
def test_signed_permutations_agree_bit_for_bit():
  h = 64
  k = C.intrinsics(16, 16, 0.5, 0.5)            # focal length and centre: powers of two
  rays = W.equirectangular_pixel_rays(h)
  perms = C.signed_permutations()
  assert len(perms) == 48 and len({m.tobytes() for m in perms}) == 48
  excluded = {'rays': [0, 0], 'view': [0, 0]}
  for m in perms:
    x, y, z = R.mat_times_columns(m, rays)
    nz = (x != 0) & (y != 0) & (z != 0)
    excluded['rays'][0] += int((~nz).sum())
    excluded['rays'][1] += nz.size
    a = R.rotate_coords(m[None], rays, C.SRC_H, C.SRC_W)[0]
    b = W.rotate_coords(m[None], h, C.SRC_W, C.SRC_H)[0]
    assert C.first_mismatch(a[nz], b[nz]) is None, C.first_mismatch(a[nz], b[nz])
    w2i = np.matmul(k, m).astype(F32)
    for rnd in (False, True):
      # the statement's components are those of w2i here; a zero ray component can still make one zero
      xw, yw, zw = R.mat_times_columns(w2i, rays)
      nzw = nz & (xw != 0) & (yw != 0) & (zw != 0)
      a = R.perspective_coords(w2i, rays, rnd)
      b = W.perspective_coords(w2i, h, rnd)
      assert C.first_mismatch(a[nzw], b[nzw]) is None, C.first_mismatch(a[nzw], b[nzw])
    kinv_t = R.inverse_intrinsics_t(k)
    px, py = R._pixel_decode(37 * 41, 37, 41)
    comp = R.rows_times_mat(*R.rows_times_mat(px, py, np.ones_like(px), kinv_t), m)
    nzv = (comp[0] != 0) & (comp[1] != 0) & (comp[2] != 0)
    excluded['view'][0] += int((~nzv).sum())
    excluded['view'][1] += nzv.size
    a = R.perspective_from_equirect_coords(kinv_t, m, 37, 41, 37, 75)
    b = W.perspective_from_equirect_coords(k, m, 37, 41, (37, 75))
    assert C.first_mismatch(a[nzv], b[nzv]) is None, C.first_mismatch(a[nzv], b[nzv])
  for name, (bad, total) in excluded.items():
    print(f'excluded ({name}): {bad} of {total} = {bad / total:.5f}')
    assert bad / total <= 0.02, (name, bad, total)


# --------------------------------------------------------------------- c. transcendentals
@pytest.fixture(scope='module')
def transcendental_log():
  """Forms every case's expected outputs with atan2 / acos / asin replaced by versions that also
  evaluate the C twin and count where the two differ.  The values are warp_np's own."""
  log = {'atan2': [0, 0], 'acos': [0, 0], 'asin': [0, 0]}
  orig = {'_atan2_32': W._atan2_32, '_acos32': W._acos32, '_asin32': W._asin32}
  twin = {'_atan2_32': warp_c.atan2f, '_acos32': warp_c.acosf, '_asin32': warp_c.asinf}

  def checking(name, key):
    def f(*args):
      want = orig[name](*args)
      got = twin[name](*[np.broadcast_to(np.asarray(a, F32), np.shape(want)) for a in args]).reshape(np.shape(want))
      differ = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
      log[key][0] += want.size
      log[key][1] += int(differ.sum())
      return want
    return f

  saved = [(mod, name, getattr(mod, name)) for mod in (W, R) for name in orig]
  try:
    for mod, name, _ in saved:
      setattr(mod, name, checking(name, {'_atan2_32': 'atan2', '_acos32': 'acos', '_asin32': 'asin'}[name]))
    for case in C.build_all_cases():
      case._want = case.compute()
  finally:
    for mod, name, fn in saved:
      setattr(mod, name, fn)
  return log


def test_transcendentals_equal_the_c_twin_on_every_case_input(transcendental_log):
  for name, (count, bad) in transcendental_log.items():
    print(f'{name}: {count} elements, {bad} disagreements')
    assert count > 0 and bad == 0, (name, count, bad)
  assert transcendental_log['atan2'][0] > 2 * C.Q_LOOP


# ------------------------------------------------------------------- d. planted errors
LAST_SENTINEL = np.int32(0x7FC00000)


def _blank_last(entry, result):
  """What a kernel that skips its last query leaves: the NaN (for int32, the sentinel) the output
  buffer was filled with."""
  res = [np.array(a, copy=True) for a in C.outputs(result)]
  if entry in ('rotate_coords',):
    res[0][:, -1, :] = np.nan
  elif entry in ('perspective_coords', 'persp_from_equirect_coords'):
    res[0][-1, :] = np.nan
  elif entry == 'rotate_pano':
    res[0][:, -1, -1, :] = np.nan
  elif entry in ('project_perspective_image', 'get_perspective_from_equirectangular_image'):
    res[0][-1, -1, :] = np.nan
  elif entry == 'perspective_to_pointcloud':
    res[0][:, :, -1] = np.nan
    res[1][:, -1, :] = LAST_SENTINEL
  else:
    for a in res:
      a[:, -1, -1, :] = np.nan
  return tuple(res) if len(res) > 1 else res[0]


def _strided_wrong(grid, query_points, indexing='ij'):
  """tfa's gather with the row stride taken from the other dimension: tap (y, x) reads the element
  at y * H + x of the flattened (H, W) grid."""
  grid = np.asarray(grid, F32)
  b, h, w, c = grid.shape
  yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
  idx = np.clip(yy * h + xx, 0, h * w - 1).reshape(-1)
  return W.interpolate_bilinear(grid.reshape(b, h * w, c)[:, idx].reshape(b, h, w, c), query_points, indexing)


def _pad_short(image, value):
  """The last row and column of the image count as padding."""
  image = np.array(image, copy=True)
  image[:, -1, :, :] = value
  image[:, :, -1, :] = value
  return np.pad(image, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='constant', constant_values=value)


def _half_away(x):
  x64 = np.asarray(x, np.float64)
  return np.copysign(np.floor(np.abs(x64) + 0.5), x64).astype(F32)


_POST = None    # (entry, result) -> result, applied to a statement's outputs while an error is planted there


def _stmt(entry):
  f = getattr(R, C.STATEMENTS[entry])
  return f if _POST is None else (lambda *a, **k: _POST(entry, f(*a, **k)))


_ROTATE_ORIG = R.rotate_coords
_DECODE_ORIG = R._pixel_decode

# name -> (attributes of _persp_ref to replace, old bar checks it can touch, entries whose new cases must notice)
MUTATIONS = {
    'decode-swap': (lambda: {'_pixel_decode': lambda total, h, w: _DECODE_ORIG(total, w, h)},
                    ('get_perspective', 'cell17'),
                    ('persp_from_equirect_coords', 'get_perspective_from_equirectangular_image', 'perspective_guidance')),
    'tap-stride-swap': (lambda: {'interpolate_bilinear': _strided_wrong}, ('cell15',), ('perspective_to_pointcloud',)),
    'batch-matrix-0': (lambda: {'rotate_coords': lambda matrix, *a, **k: _ROTATE_ORIG(
        np.repeat(np.asarray(matrix, F32)[:1], len(matrix), axis=0), *a, **k)},
                       ('rotate_pano',), ('rotate_coords', 'rotate_pano')),
    'last-unwritten': (lambda: {'POST': _blank_last},
                       ('rotate_pano', 'project', 'get_perspective', 'cell15', 'cell17'), tuple(C.STATEMENTS)),
    'half-away': (lambda: {'_round': _half_away}, ('cell15',), ('perspective_coords',)),   # the tie cases
    'inside-off-by-1': (lambda: {'_pad': _pad_short}, ('cell15', 'project-mean'),
                        ('project_perspective_image', 'perspective_to_pointcloud')),
    'z-ge-0': (lambda: {'_in_front': lambda z: z >= 0}, ('project', 'cell15'), ('perspective_coords',)),
}
# the verdicts of the old bar, as found (True: the planted error passes it)
OLD_BAR_PASSES = {
    'decode-swap': True, 'tap-stride-swap': True, 'batch-matrix-0': False, 'last-unwritten': True,
    'half-away': True, 'inside-off-by-1': False, 'z-ge-0': True,
}


@contextlib.contextmanager
def planted(name):
  global _POST
  attrs = MUTATIONS[name][0]()
  post = attrs.pop('POST', None)
  saved = {k: getattr(R, k) for k in attrs}
  try:
    _POST = post
    for k, v in attrs.items():
      setattr(R, k, v)
    yield
  finally:
    _POST = None
    for k, v in saved.items():
      setattr(R, k, v)


@pytest.fixture(scope='module')
def old_bar():
  """The inputs and warp_np outputs of the bar tests of tests/test_warp_gpu.py: their shapes (h = 32,
  24 x 24, 64 x 64 to eq_h = 128) and their seeds."""
  rng = np.random.default_rng(18)
  rng.standard_normal((2, 17, 23, 3)); rng.uniform(-2, 25, (2, 500, 2))   # the draws that come first
  pano = rng.uniform(0, 1, (2, 32, 64, 3)).astype(F32)
  def rot(a, b):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return (np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @
            np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])).astype(F32)
  mats = np.stack([rot(0.3, -1.1), rot(-0.2, 2.0)])
  img = rng.uniform(0, 1, (24, 24, 3)).astype(F32)
  fov = np.array([np.pi / 2, np.pi / 2], F32)
  rots = np.array([0.1, 0.4], F32)
  k24 = C.intrinsics(12, 12, 11.5, 11.5)
  rng23 = np.random.default_rng(23)      # the mean-padding image follows these draws
  rng23.integers(0, 256, (2, 24, 48, 3)); rng23.uniform(0, 1, (2, 24, 48)); rng23.uniform(size=(2, 24, 48))
  rng23.integers(0, 256, (1, 10, 14, 2)); rng23.uniform(0, 1, (2, 32, 64, 3))
  img_mean = rng23.uniform(0, 1, (24, 24, 3)).astype(F32)
  eq_h = 128
  rng70 = np.random.default_rng(70 + eq_h)
  k64 = C.intrinsics(32, 32, 32, 32)
  rgb01 = (rng70.integers(1, 256, (64, 64, 3)).astype(F32) / F32(255)).astype(F32)
  depth = rng70.uniform(0.02, 0.2, (64, 64)).astype(F32)
  xyz_o, f_o = W.notebook_cell15_pointcloud(rgb01, depth, k64, C.NOTEBOOK_ROT, eq_h)
  d_o, r_o = warp_c.project_feats_to_equirectangular(f_o, xyz_o, eq_h, 2 * eq_h, -1, 20.0,
                                                     offset=np.array([[0.0, 0.01, 0.0]], F32))
  near = lambda a, b: np.abs(a - b).max(-1) <= 1e-4

  def rotate_pano():
    ok = np.isfinite(W.rotate_coords(mats, 32, 64, 32)).all(-1).reshape(2, 32, 64)
    return near(_stmt('rotate_pano')(pano, mats), W.rotate_pano(pano, mats))[ok].mean() > 0.995

  def project(image=img, mode='constant'):
    return near(_stmt('project_perspective_image')(image, fov, 16, rotations=rots, pad_mode=mode),
                W.project_perspective_image(image, fov, 16, rotations=rots, pad_mode=mode)).mean() > 0.995

  def get_perspective():
    return near(_stmt('get_perspective_from_equirectangular_image')(pano[0], k24, mats[0], 24, 24),
                W.get_perspective_from_equirectangular_image(pano[0], k24, mats[0], 24, 24)).mean() > 0.995

  def cell15():
    xyz, f = _stmt('perspective_to_pointcloud')(rgb01, depth, k64, C.NOTEBOOK_ROT, eq_h)
    same = np.all(xyz == xyz_o, axis=1)[0] & np.all(f == f_o, axis=-1)[0]
    covered = f_o[0, :, 0] >= 0
    return bool(same.mean() > 0.995 and same[covered].mean() > 0.995)

  def cell17():
    want = W.notebook_cell17_guidance(r_o[0], d_o[0], k64, C.NOTEBOOK_NEW_ROT, 64, 64)
    got = _stmt('perspective_guidance')(r_o[0], d_o[0], k64, C.NOTEBOOK_NEW_ROT, 64, 64)
    return all(near(a, b).mean() > 0.995 for a, b in zip(got, want))

  return {'rotate_pano': rotate_pano, 'project': project, 'project-mean': lambda: project(img_mean, 'mean'),
          'get_perspective': get_perspective, 'cell15': cell15, 'cell17': cell17}


def test_the_unplanted_statement_passes_the_old_bar(old_bar):
  for name, check in old_bar.items():
    assert check(), name


@pytest.mark.parametrize('name', list(MUTATIONS))
def test_planted_error_old_bar_verdict_and_exact_cases_notice(name, old_bar, transcendental_log):
  _, bar_checks, entries = MUTATIONS[name]
  with planted(name):
    verdicts = {c: bool(old_bar[c]()) for c in bar_checks}
    noticed, silent = {}, {}
    for case in C.build_all_cases():
      if case.entry not in entries or 'looped' in case.classes:
        continue
      got, want = C.outputs(_stmt(case.entry)(**case.inputs)), C.outputs(case.want())
      diff = any(C.first_mismatch(g, w) is not None for g, w in zip(got, want))
      (noticed if diff else silent).setdefault(case.entry, []).append(case.name)
  print(f'{name}: old bar {verdicts}; noticed by ' +
        ', '.join(f'{e}: {len(noticed.get(e, []))} of {len(noticed.get(e, [])) + len(silent.get(e, []))}' for e in entries))
  assert all(verdicts.values()) == OLD_BAR_PASSES[name], verdicts
  for entry in entries:
    assert noticed.get(entry), f'{name}: no exact case of {entry} notices'
  if name == 'last-unwritten':
    assert not silent, silent


# ---------------------------------------------------------------------- e. admissibility
def test_every_gpu_case_is_admissible(transcendental_log):
  cases = C.build_all_cases()
  assert len({c.id for c in cases}) == len(cases)
  dets = {int(round(float(np.linalg.det(C.MATS[f'perm{i}'].astype(np.float64))))) for i in C._PERM_PICK}
  assert dets == {1, -1}, 'proper and improper permutations'
  for m in (C.MATS[n] for n in C.ROTATIONS):
    assert np.abs(m.astype(np.float64) @ m.astype(np.float64).T - np.eye(3)).max() < 1e-5
  seen = set()
  for case in cases:
    inp, want = case.inputs, C.outputs(case.want())
    seen.update((case.entry, cls) for cls in case.classes)
    if case.entry == 'rotate_coords':
      q = inp['rays'].shape[1]
      assert ('looped' in case.classes) == (q > C.ONE_TRIP) and want[0].shape == (3, q, 2)
      assert len({m.tobytes() for m in inp['matrix']}) == 3
      assert C.first_mismatch(want[0][2], want[0][0]) is not None and C.first_mismatch(want[0][2], want[0][1]) is not None
      nan = np.isnan(want[0])
      if 'NaN pitch' in case.classes:
        assert nan[2, :, 0].any() or q == 1, case.id
        assert not nan[:2].any() and not nan[..., 1].any()
      else:
        assert not nan.any(), case.id
    if case.entry == 'perspective_coords':
      assert not np.isnan(want[0]).any() or 'z <= 0' in case.classes
      if 'ties' in case.classes:
        v = R.perspective_coords(inp['world_to_image'], inp['rays'], False)
        k = np.floor(v)
        assert np.all(v - k == F32(0.5)), 'exact k + 0.5'
        for col in (0, 1):
          kk = k[:, col].astype(np.int64)
          assert ((kk % 2 == 0) & (kk > 0)).any() and ((kk % 2 == 1) & (kk > 0)).any()
          assert ((kk % 2 == 0) & (kk < 0)).any() and ((kk % 2 == 1) & (kk < 0)).any()
        assert {0.5, 1.0, 2.0} == set(np.unique(inp['rays'][2]).tolist())
      if 'z <= 0' in case.classes:
        z = inp['rays'][2]
        assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any() and (z < -0.1).any()
        tiny = np.finfo(F32).tiny
        assert ((z > 0) & (z < tiny)).any() and ((z < 0) & (z > -tiny)).any(), 'denormal z of both signs'
        behind = ~(z > 0)
        assert np.all(want[0][behind] == F32(-1.0 + inp['add']))
    if case.entry == 'persp_from_equirect_coords':
      assert want[0].shape == (inp['height'] * inp['width'], 2) and not np.isnan(want[0]).any()
    if case.entry == 'perspective_to_pointcloud':
      xyz1, feats = want
      covered = feats[0, :, 0] != C.VOID
      assert covered.mean() > 0.02, (case.id, covered.mean())
      assert (~covered).any() or inp['pad_value'] != 0, case.id   # void_class is written somewhere
      d = np.asarray(inp['depth01'])
      assert (d == 0).any() and (d == 1).any()
      if inp['round_to_nearest'] and inp['eq_height'] >= 128:   # (a 16 x 32 grid takes too few samples to be sure)
        proj = R.project_perspective_image(d[..., None], None, inp['eq_height'],
                                           camera_intrinsics=inp['camera_intrinsics'],
                                           rotation_matrix=inp['rotation_matrix'], pad_value=inp['pad_value'],
                                           round_to_nearest=True)
        assert (proj == 1).any(), (case.id, 'a source pixel of depth exactly 1 is sampled')
        if inp['pad_value'] != 0:
          assert (proj == 0).any(), (case.id, 'a source pixel of depth exactly 0 is sampled')
    if case.entry == 'perspective_guidance':
      image, depth, mask = want
      assert mask.mean() > 0.05 and mask.mean() < 1.0, (case.id, mask.mean())
      if 'hand-placed taps' in case.classes:
        rgb, dep = np.asarray(inp['pred_rgb']), np.asarray(inp['pred_depth'])
        eh, ew = dep.shape
        uv = R.perspective_from_equirect_coords(R.inverse_intrinsics_t(inp['camera_intrinsics']),
                                                inp['new_rotation_matrix'], inp['pers_height'],
                                                inp['pers_width'], eh, ew)
        fx = np.clip(np.floor(uv[:, 0]), 0, ew - 2).astype(np.int64)
        fy = np.clip(np.floor(uv[:, 1]), 0, eh - 2).astype(np.int64)
        taps_d = np.stack([dep[fy + a, fx + b] for a in (0, 1) for b in (0, 1)])
        taps_rgb = np.stack([rgb[fy + a, fx + b] for a in (0, 1) for b in (0, 1)])
        assert (taps_d == 0).any() and (taps_d == 1).any()
        assert (taps_rgb[..., 1] == 0).any() and (taps_rgb > 255).any()
        raw = R.get_perspective_from_equirectangular_image(rgb, inp['camera_intrinsics'],
                                                           inp['new_rotation_matrix'], inp['pers_height'],
                                                           inp['pers_width'], uv=uv)
        assert ((raw > 255).any(-1) & (mask[0, ..., 0] == 1)).any(), (case.id, 'the clip engages under the mask')
        assert (image == 1.0).any()
  missing = [(e, c) for e, classes in C.EXPECTED_CLASSES.items() for c in classes if (e, c) not in seen]
  assert not missing, missing
