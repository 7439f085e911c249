"""The cases of tests/test_persp_exact_gpu.py, built once and shared with
tests/test_persp_ref_cpu.py, which checks their preconditions and shows that they notice planted
errors.  A case holds NumPy inputs and the pinned-order statement's outputs (tests/_persp_ref.py);
nothing here looks at the code under test.  Inputs and expected outputs are formed on first use and
kept; nobody may write into them."""
import itertools
import zlib

import numpy as np

from oracle import warp_c
import _persp_ref as R

F32 = np.float32
KBLOCK, GRID_CAP = 256, 4096
ONE_TRIP = KBLOCK * GRID_CAP          # above this many queries a thread takes a second trip
Q_SET = (1, 255, 256, 257)
Q_LOOP = ONE_TRIP + 77
SRC_H, SRC_W = 37, 91                 # a source panorama that is not the ray grid
DEPTH_SCALE = 20.0
VOID = -1


# ----------------------------------------------------------------------------------- matrices
def signed_permutations():
  """The 48 matrices with one +-1 per row and column."""
  out = []
  for perm in itertools.permutations(range(3)):
    for signs in itertools.product((1.0, -1.0), repeat=3):
      m = np.zeros((3, 3), F32)
      for i in range(3):
        m[i, perm[i]] = signs[i]
      out.append(m)
  return out


def _qr_rotation(seed):
  rng = np.random.default_rng(seed)
  q, r = np.linalg.qr(rng.standard_normal((3, 3)))
  q = q * np.sign(np.diag(r))[None, :]
  if np.linalg.det(q) < 0:
    q[:, 2] = -q[:, 2]
  return q.astype(F32)


NOTEBOOK_ROT = np.array([[0.99992853, -0.01185191, 0.00158339], [0.01187317, 0.9998291, -0.01416931],
                         [-0.00141519, 0.01418709, 0.9998984]], F32)
_ANG = 15.0 / 180.0 * np.pi
NOTEBOOK_NEW_ROT = (NOTEBOOK_ROT.astype(np.float64) @ np.array(
    [[np.cos(_ANG), 0, np.sin(_ANG)], [0, 1, 0], [-np.sin(_ANG), 0, np.cos(_ANG)]])).astype(F32)
_PERM_PICK = (1, 7, 12, 18, 25, 31, 38, 44)


def matrices():
  """name -> (3,3) fp32, in a fixed order: identity, eight signed permutations, the notebook's
  two, three seeded rotations, one scaled (non-orthogonal) matrix."""
  sp = signed_permutations()
  out = {'identity': np.eye(3, dtype=F32)}
  for i in _PERM_PICK:
    out[f'perm{i}'] = sp[i]
  out['rot'] = NOTEBOOK_ROT
  out['new_rot'] = NOTEBOOK_NEW_ROT
  for s in range(3):
    out[f'qr{s}'] = _qr_rotation(900 + s)
  out['scaled'] = (out['qr0'] * F32(1.25)).astype(F32)
  return out


MATS = matrices()
MAT_NAMES = list(MATS)
ROTATIONS = [n for n in MAT_NAMES if n != 'scaled']


def intrinsics(fx, fy, cx, cy):
  return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)


K_ODD = intrinsics(12, 14, 11.5, 8.5)     # fx != fy, cx != cy
K_POW2 = intrinsics(16, 16, 8, 8)


def view_intrinsics(height, width):
  """fx != fy; the centre is the middle of a (height, width) image, so cx != cy off the square."""
  return intrinsics(12, 14, 0.5 * (width - 1), 0.5 * (height - 1))


# -------------------------------------------------------------------------------------- cases
class Case:
  def __init__(self, entry, name, classes, make):
    self.entry, self.name, self.classes, self._make = entry, name, tuple(classes), make
    self._inputs = self._want = None

  @property
  def id(self):
    return f'{self.entry}:{self.name}'

  def rng(self):
    return np.random.default_rng(zlib.crc32(self.id.encode()))

  @property
  def inputs(self):
    if self._inputs is None:
      self._inputs = self._make(self)
      for v in self._inputs.values():
        if isinstance(v, np.ndarray):
          v.setflags(write=False)
    return self._inputs

  def compute(self):
    """The pinned statement on this case's inputs, afresh (test_persp_ref_cpu.py calls this with an
    error planted); want() keeps the unplanted result."""
    return getattr(R, STATEMENTS[self.entry])(**self.inputs)

  def want(self):
    if self._want is None:
      self._want = self.compute()
    return self._want


def _trip(q):
  return 'looped' if q > ONE_TRIP else 'single trip'


def _shape_class(h, w):
  return 'square' if h == w else ('wide' if w > h else 'tall')


def _unit_rays(rng, q):
  v = rng.standard_normal((3, q))
  return (v / np.linalg.norm(v, axis=0, keepdims=True)).astype(F32)


def _rotate_cases():
  out = []
  triples = [MAT_NAMES[i:i + 3] for i in range(0, 15, 3)]
  for q in Q_SET:
    for names in triples:
      def make(case, q=q, names=names):
        return dict(matrix=np.stack([MATS[n] for n in names]), rays=_unit_rays(case.rng(), q),
                    src_h=SRC_H, src_w=SRC_W)
      cls = ['single trip', 'n = 3', 'src != ray grid'] + (['NaN pitch'] if 'scaled' in names else [])
      out.append(Case('rotate_coords', f'q{q}-' + '+'.join(names), cls, make))
  def make_loop(case):
    return dict(matrix=np.stack([MATS[n] for n in ('qr1', 'rot', 'perm12')]),
                rays=_unit_rays(case.rng(), Q_LOOP), src_h=SRC_H, src_w=SRC_W)
  out.append(Case('rotate_coords', f'q{Q_LOOP}-loop', ['looped', 'n = 3', 'src != ray grid'], make_loop))
  return out


def _w2i(k, name):
  return np.matmul(k, MATS[name]).astype(F32)


def tie_rays():
  """Rays whose x / z and y / z are exactly k + 0.5, k even and odd, positive and negative, with
  dyadic z: (k + 0.5) z is exact, and so is the quotient."""
  ks = np.arange(-6, 7, dtype=np.float64) + 0.5
  rows = [((kx * z), (ky * z), z) for z in (0.5, 1.0, 2.0) for kx in ks for ky in ks]
  return np.ascontiguousarray(np.array(rows, F32).T)


def behind_rays():
  """z in {+0, -0, negative, negative and positive denormal} against x, y of both signs, zero and
  denormal: the `-1` branch everywhere but at the positive denormal."""
  zs = np.array([0.0, -0.0, -1.0, -0.25, -1e-40, 1e-40, 2e-40], F32)
  xs = np.array([0.0, -0.0, 1.0, -1.0, 0.375, -2.5, 3e-40, -1e-40], F32)
  rows = [(x, y, z) for z in zs for x in xs for y in xs[::-1]]
  return np.ascontiguousarray(np.array(rows, F32).T)


def _perspective_coords_cases():
  out = []
  combos = list(itertools.product((0, 1), (0.0, 1.0)))
  i = 0
  for q in Q_SET:
    for rnd, add in combos:
      name = MAT_NAMES[i % len(MAT_NAMES)]
      k = K_ODD if i % 2 else K_POW2
      i += 1
      def make(case, q=q, rnd=rnd, add=add, name=name, k=k):
        return dict(world_to_image=_w2i(k, name), rays=_unit_rays(case.rng(), q),
                    round_to_nearest=bool(rnd), add=add)
      out.append(Case('perspective_coords', f'q{q}-round{rnd}-add{add:g}-{name}',
                      ['single trip', f'round {rnd}', f'add {add:g}'], make))
  for rnd, add in combos:
    out.append(Case('perspective_coords', f'ties-round{rnd}-add{add:g}',
                    ['single trip', 'ties', f'round {rnd}', f'add {add:g}'],
                    lambda case, rnd=rnd, add=add: dict(world_to_image=np.eye(3, dtype=F32), rays=tie_rays(),
                                                        round_to_nearest=bool(rnd), add=add)))
    out.append(Case('perspective_coords', f'behind-round{rnd}-add{add:g}',
                    ['single trip', 'z <= 0', f'round {rnd}', f'add {add:g}'],
                    lambda case, rnd=rnd, add=add: dict(world_to_image=np.eye(3, dtype=F32), rays=behind_rays(),
                                                        round_to_nearest=bool(rnd), add=add)))
  out.append(Case('perspective_coords', f'q{Q_LOOP}-loop', ['looped', 'round 1', 'add 1'],
                  lambda case: dict(world_to_image=_w2i(K_ODD, 'qr2'), rays=_unit_rays(case.rng(), Q_LOOP),
                                    round_to_nearest=True, add=1.0)))
  return out


VIEWS = ((1, 1), (1, 300), (18, 24), (24, 18), (257, 3))
EQ_SHAPES = ((32, 64), (37, 75))


def _from_equirect_cases():
  out = []
  i = 0
  for (h, w) in VIEWS:
    for (eh, ew) in EQ_SHAPES:
      for kname, k in (('odd', K_ODD), ('pow2', K_POW2)):
        name = MAT_NAMES[i % len(MAT_NAMES)]
        i += 1
        out.append(Case('persp_from_equirect_coords', f'{h}x{w}-from-{eh}x{ew}-K{kname}-{name}',
                        [_trip(h * w), _shape_class(h, w), 'fx != fy' if kname == 'odd' else 'power-of-two K'],
                        lambda case, h=h, w=w, eh=eh, ew=ew, k=k, name=name: dict(
                            kinv_t=R.inverse_intrinsics_t(k), rotation_matrix=MATS[name], height=h,
                            width=w, eq_h=eh, eq_w=ew)))
  out.append(Case('persp_from_equirect_coords', '1024x1025-loop', ['looped', 'wide', 'fx != fy'],
                  lambda case: dict(kinv_t=R.inverse_intrinsics_t(intrinsics(500, 520, 512, 511.5)),
                                    rotation_matrix=MATS['qr1'], height=1024, width=1025, eq_h=37, eq_w=75)))
  return out


def _rotate_pano_cases():
  out = []
  pairs = (('rot', 'new_rot'), ('qr0', 'perm7'), ('qr1', 'identity'), ('qr2', 'perm18'))
  for (h, c), names in zip(itertools.product((5, 32), (3, 1)), pairs):
    out.append(Case('rotate_pano', f'h{h}-c{c}-' + '+'.join(names), ['n = 2', f'C = {c}', f'h = {h}'],
                    lambda case, h=h, c=c, names=names: dict(
                        pano=case.rng().uniform(0, 1, (2, h, 2 * h, c)).astype(F32),
                        matrix=np.stack([MATS[n] for n in names]))))
  return out


SOURCES = ((17, 24), (24, 17))
PADS = (('constant', 0.0), ('constant', 0.25), ('mean', 0.0), ('reflect', 0.0))


def _project_cases():
  out = []
  i = 0
  for (ih, iw), c, oh, (mode, pv), rnd, form in itertools.product(SOURCES, (1, 3), (16, 33), PADS, (0, 1),
                                                                  ('K', 'fov')):
    name = ROTATIONS[i % len(ROTATIONS)]
    i += 1
    def make(case, ih=ih, iw=iw, c=c, oh=oh, mode=mode, pv=pv, rnd=rnd, form=form, name=name):
      d = dict(image=case.rng().uniform(0.01, 1, (ih, iw, c)).astype(F32), output_height=oh, pad_mode=mode,
               pad_value=pv, round_to_nearest=bool(rnd))
      if form == 'K':
        d.update(fov=None, camera_intrinsics=view_intrinsics(ih, iw), rotation_matrix=MATS[name])
      else:
        d.update(fov=np.array([np.pi / 3, np.pi / 2], F32), rotations=np.array([0.1, 0.4], F32))
      return d
    pad = mode if mode != 'constant' else f'constant {pv:g}'
    out.append(Case('project_perspective_image', f'{ih}x{iw}x{c}-to-{oh}-{pad.replace(" ", "")}-round{rnd}-{form}'
                    + (f'-{name}' if form == 'K' else ''),
                    [_shape_class(ih, iw) + ' source', f'C = {c}', f'H = {oh}', f'pad {pad}', f'round {rnd}',
                     'intrinsics' if form == 'K' else 'fov + rotations'], make))
  return out


def _get_perspective_cases():
  out = []
  i = 0
  for (h, w), eh, c in itertools.product(((18, 24), (24, 18)), (32, 37), (1, 3)):
    name = ROTATIONS[(3 * i + 1) % len(ROTATIONS)]
    i += 1
    out.append(Case('get_perspective_from_equirectangular_image', f'{h}x{w}-from-{eh}x{2 * eh}x{c}-{name}',
                    [_shape_class(h, w) + ' view', f'C = {c}', f'eq_h = {eh}'],
                    lambda case, h=h, w=w, eh=eh, c=c, name=name: dict(
                        image=case.rng().uniform(0, 1, (eh, 2 * eh, c)).astype(F32),
                        camera_intrinsics=view_intrinsics(h, w), rotation_matrix=MATS[name], height=h, width=w)))
  return out


def source_image_and_depth(rng, ih, iw, c):
  """image (ih,iw,c) on the k / 255 lattice without zeros; depth in (0, 1) with exact 0 and exact 1
  at hand-placed pixels."""
  image = (rng.integers(1, 256, (ih, iw, c)).astype(F32) / F32(255)).astype(F32)
  depth = rng.uniform(0.02, 0.9, (ih, iw)).astype(F32)
  depth[::4, ::5] = 0.0
  depth[1::4, 2::5] = 1.0
  return image, depth


def _pointcloud_cases():
  out = []
  i = 0
  for (ih, iw), c, eq_h, pos, rnd, pv in itertools.product(SOURCES, (1, 2, 3, 4), (16, 128), (0, 1), (1, 0),
                                                           (0.0, 0.25)):
    name = ('rot', 'qr0', 'identity', 'new_rot', 'qr2')[i % 5]
    i += 1
    def make(case, ih=ih, iw=iw, c=c, eq_h=eq_h, pos=pos, rnd=rnd, pv=pv, name=name):
      rng = case.rng()
      image, depth = source_image_and_depth(rng, ih, iw, c)
      return dict(image01=image, depth01=depth, camera_intrinsics=view_intrinsics(ih, iw),
                  rotation_matrix=MATS[name], eq_height=eq_h, void_class=VOID, depth_scale=DEPTH_SCALE,
                  position=np.array([0.3, -1.25, 2.0], F32) if pos else None, pad_value=pv,
                  round_to_nearest=bool(rnd))
    out.append(Case('perspective_to_pointcloud',
                    f'{ih}x{iw}x{c}-to-{eq_h}-pos{pos}-round{rnd}-pad{pv:g}-{name}',
                    ['single trip', _shape_class(ih, iw) + ' source', f'C = {c}', f'eq_h = {eq_h}',
                     'position' if pos else 'no position', f'round {rnd}', f'pad {pv:g}'], make))
  def make_loop(case):
    image, depth = source_image_and_depth(case.rng(), 17, 24, 3)
    return dict(image01=image, depth01=depth, camera_intrinsics=view_intrinsics(17, 24),
                rotation_matrix=MATS['rot'], eq_height=725, void_class=VOID, depth_scale=DEPTH_SCALE,
                position=np.array([0.3, -1.25, 2.0], F32), pad_value=0.0, round_to_nearest=True)
  out.append(Case('perspective_to_pointcloud', '17x24x3-to-725-loop',
                  ['looped', 'wide source', 'C = 3', 'position', 'round 1', 'pad 0'], make_loop))
  return out


def hand_placed_prediction(rng, eq_h=32, eq_w=64):
  """A splat output with, at fixed places: depth exactly 0 and exactly 1, a zero green channel,
  and 2 x 2 blocks of RGB 300 (above 255: the clip)."""
  rgb = rng.integers(1, 256, (eq_h, eq_w, 3)).astype(F32)
  depth = rng.uniform(0.05, 0.95, (eq_h, eq_w)).astype(F32)
  depth[::5, ::7] = 0.0
  depth[2::5, 3::7] = 1.0
  rgb[1::6, 1::5, 1] = 0.0
  for dy in (3, 4):
    for dx in (2, 3):
      rgb[dy::8, dx::9] = 300.0
  return rgb, depth


def splat_prediction(eq_h=128):
  """The notebook chain of the existing bar test: a 64 x 64 view unprojected by the cell-15
  statement, moved, and splatted by the oracle."""
  rng = np.random.default_rng(70 + eq_h)
  k = intrinsics(32, 32, 32, 32)
  rgb01 = (rng.integers(1, 256, (64, 64, 3)).astype(F32) / F32(255)).astype(F32)
  depth = rng.uniform(0.02, 0.2, (64, 64)).astype(F32)
  xyz, feats = R.cell15_pointcloud(rgb01, depth, k, NOTEBOOK_ROT, eq_h)
  d, r = warp_c.project_feats_to_equirectangular(feats, xyz, eq_h, 2 * eq_h, VOID, DEPTH_SCALE,
                                                 offset=np.array([[0.0, 0.01, 0.0]], F32))
  return r[0], d[0], k


def _guidance_cases():
  out = []
  for (h, w), name in (((18, 24), 'new_rot'), ((24, 18), 'qr1')):
    def make(case, h=h, w=w, name=name):
      rgb, depth = hand_placed_prediction(case.rng())
      return dict(pred_rgb=rgb, pred_depth=depth, camera_intrinsics=view_intrinsics(h, w),
                  new_rotation_matrix=MATS[name], pers_height=h, pers_width=w)
    out.append(Case('perspective_guidance', f'{h}x{w}-from-32x64-{name}',
                    ['single trip', _shape_class(h, w) + ' view', 'hand-placed taps'], make))
  def make_splat(case):
    rgb, depth, k = splat_prediction(128)
    return dict(pred_rgb=rgb, pred_depth=depth, camera_intrinsics=k, new_rotation_matrix=NOTEBOOK_NEW_ROT,
                pers_height=64, pers_width=64)
  out.append(Case('perspective_guidance', '64x64-from-128x256-splat', ['single trip', 'square view', 'splat output'],
                  make_splat))
  def make_loop(case):
    rgb, depth = hand_placed_prediction(case.rng())
    return dict(pred_rgb=rgb, pred_depth=depth, camera_intrinsics=intrinsics(500, 520, 512, 511.5),
                new_rotation_matrix=MATS['qr0'], pers_height=1024, pers_width=1025)
  out.append(Case('perspective_guidance', '1024x1025-from-32x64-loop', ['looped', 'wide view', 'hand-placed taps'],
                  make_loop))
  return out


STATEMENTS = {    # entry -> the statement's name in _persp_ref, looked up at call time
    'rotate_coords': 'rotate_coords',
    'perspective_coords': 'perspective_coords',
    'persp_from_equirect_coords': 'perspective_from_equirect_coords',
    'rotate_pano': 'rotate_pano',
    'project_perspective_image': 'project_perspective_image',
    'get_perspective_from_equirectangular_image': 'get_perspective_from_equirectangular_image',
    'perspective_to_pointcloud': 'cell15_pointcloud',
    'perspective_guidance': 'cell17_guidance',
}

# what the cases must drive each entry point through (the GPU module adds the refusals)
EXPECTED_CLASSES = {
    'rotate_coords': ['single trip', 'looped', 'n = 3', 'src != ray grid', 'NaN pitch'],
    'perspective_coords': ['single trip', 'looped', 'round 0', 'round 1', 'add 0', 'add 1', 'ties', 'z <= 0'],
    'persp_from_equirect_coords': ['single trip', 'looped', 'square', 'wide', 'tall', 'fx != fy', 'power-of-two K'],
    'rotate_pano': ['n = 2', 'C = 1', 'C = 3', 'h = 5', 'h = 32'],
    'project_perspective_image': ['wide source', 'tall source', 'C = 1', 'C = 3', 'H = 16', 'H = 33',
                                  'pad constant 0', 'pad constant 0.25', 'pad mean', 'pad reflect', 'round 0',
                                  'round 1', 'intrinsics', 'fov + rotations'],
    'get_perspective_from_equirectangular_image': ['wide view', 'tall view', 'C = 1', 'C = 3', 'eq_h = 32',
                                                   'eq_h = 37'],
    'perspective_to_pointcloud': ['single trip', 'looped', 'wide source', 'tall source', 'C = 1', 'C = 2', 'C = 3',
                                  'C = 4', 'eq_h = 16', 'eq_h = 128', 'position', 'no position', 'round 0',
                                  'round 1', 'pad 0', 'pad 0.25'],
    'perspective_guidance': ['single trip', 'looped', 'wide view', 'tall view', 'square view', 'hand-placed taps',
                             'splat output'],
}

_ALL = None


def build_all_cases():
  """Every GPU case, in a fixed order; the same objects on every call."""
  global _ALL
  if _ALL is None:
    _ALL = (_rotate_cases() + _perspective_coords_cases() + _from_equirect_cases() + _rotate_pano_cases() +
            _project_cases() + _get_perspective_cases() + _pointcloud_cases() + _guidance_cases())
    ids = [c.id for c in _ALL]
    assert len(set(ids)) == len(ids), 'case ids must be unique'
  return _ALL


def cases_of(entry):
  return [c for c in build_all_cases() if c.entry == entry]


def first_mismatch(got, want):
  """None when `got` and `want` have the same dtype, shape and bit patterns -- NaN counts as equal
  to NaN at the same place, whatever its payload -- else a description of the first difference."""
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  if got.dtype != want.dtype or got.shape != want.shape:
    return f'got {got.dtype} {got.shape}, expected {want.dtype} {want.shape}'
  if got.dtype == F32:
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
  else:
    bad = got != want
  if not bad.any():
    return None
  first = tuple(int(v) for v in np.argwhere(bad)[0])
  return (f'{int(bad.sum())} of {got.size} differ, first at {first}: got {got[first]!r} '
          f'expected {want[first]!r}')


def outputs(result):
  """A statement's result as a tuple of arrays."""
  return tuple(result) if isinstance(result, tuple) else (result,)
