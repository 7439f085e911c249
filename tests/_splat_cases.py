"""Constructed point clouds for the z-buffer splat (test helper; NumPy only, no GPU).

Random clouds leave three parts of oracle/warp_np.py::project_to_feat unexamined: the strict fp32
tolerance `z < fl(zmin + 0.1f)` (no random point lies within a few ulp of its pixel's edge), the
sink (flat pixel 0 of image 0 collects every invalid and every culled point; with random byte
features it saturates at 255 whatever a route drops) and points of which only SOME channels are
void.  The clouds built here plant those situations and nothing else:

  fillers  one point per pixel at most, on the ray through the pixel's centre (the half-pixel
           grids of warp_np.equirect_angle_tables; warp_np.equirectangular_pixel_rays is the
           reference's OTHER convention, whose rays the splat does not map to its pixel grid),
           radius in [1, 3], features 1 .. 100.  No filler is occluded, none goes to a planted
           pixel, none to pixel (0, 0) of image 0 unless the case asks for it.  They pad every
           cloud to exactly m points per image, so the kernel route does not depend on the case.
  plants   the points a case is about, at stated indices of the point array.

build() returns the oracle's view of every point (flat index, valid flag, z after
warp_np.equirect_project_coords / splat_indices) in `notes`, asserts the case's preconditions on
it -- a case that cannot be built is an error -- and states the values the case expects at the
planted pixels and at the sink, so that a failure names the case and not only an index.

One point of the definition (reference point_cloud_utils.py:168-176, restated by both oracles):
the tolerance decides only WHERE a point's features go.  A culled point and an invalid point both
end at flat index 0 and take part in the sink's per-channel maximum whatever their z.  So the
partially void points that lie 0.1 behind the sink's minimum DO show at the sink; the
`partial_void` case has them quiet (features <= 100) in all variants but one, `loud`, where they
carry 255 and the sink must show 255.

Register stashes of the resolve kernels (se3ds_amd/csrc/geom.hip; not exported): the sorted
resolve keeps kRStash = 12 records per thread of kRThreads = 512, the packed resolve 4 per thread
of 256.  `pile` needs more than twice that in ONE pixel: 2 * 12 * 512 = 12288 < 20001 on the
sorted rows, 2 * 4 * 256 = 2048 < 4099 on the packed rows; the m of the route table serves.
"""
import functools
import itertools

import numpy as np

from oracle import warp_np

F32 = np.float32
DEPTH_SCALE = 20.0
TOL = F32(0.1)

# The rows of test_splat_exact_size_workspace_guard: the smallest shapes that reach each route with
# no switch set (tools/splat_layout_host_check.cpp pins them).  int32 with <= 3 channels is promised
# the byte range by the wrapper.  (id, n, h, w, dtype, c, void, m)
ROWS = [
    ('sorted-u8c3-256x512', 1, 256, 512, np.uint8, 3, 0, 20001),
    ('sorted-i32c3-256x512', 1, 256, 512, np.int32, 3, -1, 20001),
    ('packed-u8c3-48x96', 2, 48, 96, np.uint8, 3, 0, 4099),
    ('packed-i32c3-48x96', 2, 48, 96, np.int32, 3, -1, 4099),
    ('packed-u8c1-48x96', 2, 48, 96, np.uint8, 1, 0, 4099),
    ('binned-f32c3-48x96', 2, 48, 96, np.float32, 3, -1, 4099),
    ('binned-i32c5-48x96', 2, 48, 96, np.int32, 5, -1, 4099),
    ('scatter-i32c9-32x64', 2, 32, 64, np.int32, 9, -1, 2047),
]
ROW_IDS = [r[0] for r in ROWS]
EQUIRECT_CASES = ('edge', 'sink_feat', 'sink_z', 'partial_void', 'pile')
OFFSET = np.array([0.25, -0.5, 0.125], F32)   # exactly representable: (0, 0.5, 0) + OFFSET - OFFSET is exact
PTILE_Y, PTILE_X = 16, 32                     # the packed route's tile (kPTileY x kPTileX)


def has_case(case, row):
  """partial_void needs channels that are NOT void next to the one that is: three channels."""
  return case != 'partial_void' or row[5] >= 3


CASE_ROWS = [(case, row) for case in EQUIRECT_CASES for row in ROWS if has_case(case, row)]
CASE_ROW_IDS = [f'{case}-{row[0]}' for case, row in CASE_ROWS]


def sink_positions(m):
  """Point indices a single deciding point is placed at: both ends, the middle, and both sides of
  every chunk cut (2048-point chunks of the 4-points-per-thread sort, 4096 and 8192 of the others
  and of the binned / packed cut)."""
  pos = [0, m - 1, m // 2]
  for k in (1, 2, 4):
    pos += [2048 * k - 1, 2048 * k]
  out = []
  for p in pos:
    if 0 <= p < m and p not in out:
      out.append(p)
  return out


def variants(case, n, m):
  """The variants of a case at n images of m points (dicts; build(..., variant=v))."""
  if case in ('sink_feat', 'sink_z', 'partial_void'):
    images = [0] if n == 1 else [0, n - 1]
    out = []
    for i, pos in enumerate(sink_positions(m)):
      for img in images:
        out.append(dict(idx=pos, image=img, tile='first' if (i + img) % 2 == 0 else 'last', p0=False,
                        loud=False))
    out.append(dict(idx=m // 2, image=images[-1], tile='last', p0=True, loud=False))
    if case == 'partial_void':
      out.append(dict(idx=m // 2, image=images[-1], tile='first', p0=False, loud=True))
    return out
  if case == 'pile':
    return [dict(order='min_last'), dict(order='min_first')]
  return [dict()]


def variant_id(v):
  return ','.join(f'{k}={v[k]}' for k in sorted(v)) or 'only'


# ------------------------------------------------------------------------------ the oracle's view
def _f32_next(x, direction):
  return np.nextafter(F32(x), F32(direction), dtype=F32)


@functools.lru_cache(maxsize=None)
def _tables(h, w):
  return warp_np.equirect_angle_tables(h, w)


def pixel_dirs(h, w, v, u):
  """Unit directions (.., 3) through the centres of pixels (v, u) of the H x W target grid."""
  sin_el, cos_el, sin_hd, cos_hd = _tables(h, w)
  v = np.asarray(v)
  u = np.asarray(u)
  return np.stack([sin_el[v] * cos_hd[u], sin_el[v] * sin_hd[u], cos_el[v]], axis=-1).astype(F32)


def equirect_view(rel, h, w):
  """rel (K, 3) relative coordinates -> (pixel index or -1, z) as the oracle computes them for
  points with non-void features."""
  k = rel.shape[0]
  xyz1 = np.concatenate([rel.T, np.ones((1, k), F32)], 0)[None].astype(F32)
  proj = warp_np.equirect_project_coords(xyz1)
  flat, valid, z = warp_np.splat_indices(proj, np.ones((1, k, 1), F32), h, w, -7.0)
  return np.where(valid[0], flat[0], -1), z[0]


def point_with_z(h, w, v, u, target):
  """A point (3,) of pixel (v, u) whose oracle z equals `target` bit for bit.  The radius
  fl(sqrt(fl(fl(x^2 + y^2) + z^2))) cannot be set directly: fix a direction of norm slightly below
  1 and scan consecutive floats of the scale around target / |d|.  Where the roundings of the three
  squares step over the target (near the poles one component carries the whole radius), the next
  direction -- another norm, a slight lean toward the neighbouring pixel's centre -- is tried."""
  target = F32(target)
  pix = v * w + u
  centre = pixel_dirs(h, w, v, u)
  lean_u = pixel_dirs(h, w, v, u + 1 if u + 1 < w else u - 1) - centre
  lean_v = pixel_dirs(h, w, v + 1 if v + 1 < h else v - 1, u) - centre
  for attempt in range(96):
    d = ((centre + F32(0.02 * (attempt % 4)) * lean_u + F32(0.013 * (attempt % 12)) * lean_v) *
         F32(0.999 - 0.0007 * (attempt // 12))).astype(F32)
    s0 = F32(np.float64(target) / np.linalg.norm(d.astype(np.float64)))
    scales = (s0.view(np.int32) + np.arange(-32, 33, dtype=np.int32)).view(F32)
    pts = (d[None, :] * scales[:, None]).astype(F32)
    idx, z = equirect_view(pts, h, w)
    hit = np.nonzero((z == target) & (idx == pix))[0]
    if hit.size:
      return pts[hit[0]]
  raise AssertionError(f'no scale gives z == {target!r} in pixel ({v}, {u}) of {h} x {w}')


class _Cloud:
  """n images of m points: relative coordinates, features, which indices are taken."""

  def __init__(self, n, h, w, c, dtype, void, m, seed):
    self.n, self.h, self.w, self.c, self.dtype, self.void, self.m = n, h, w, c, dtype, void, m
    self.rng = np.random.default_rng(seed)
    self.rel = np.zeros((n, m, 3), F32)
    self.feats = np.zeros((n, m, c), np.float64)
    self.taken = np.zeros((n, m), bool)
    self.plant_px = [set() for _ in range(n)]   # pixels no filler may go to
    self.plant_px[0].add(0)                      # the sink stays free unless a case fills it

  def put(self, b, idx, xyz, feat3):
    assert not self.taken[b, idx], (b, idx)
    self.taken[b, idx] = True
    self.rel[b, idx] = xyz
    f = self.rng.integers(1, 101, self.c).astype(np.float64)   # channels beyond the third: fillers
    k = min(self.c, 3)
    f[:k] = feat3[:k]
    self.feats[b, idx] = f

  def free_indices(self, b):
    return np.nonzero(~self.taken[b])[0]

  def fill(self, make_point):
    """Fillers on every index not taken: one per pixel, never a planted pixel."""
    n, h, w = self.n, self.h, self.w
    for b in range(n):
      free = self.free_indices(b)
      pool = np.array([p for p in range(h * w) if p not in self.plant_px[b]])
      assert free.size <= pool.size, f'{free.size} fillers for {pool.size} free pixels'
      px = self.rng.permutation(pool)[:free.size]
      rad = self.rng.uniform(1.0, 3.0, free.size).astype(F32)
      self.rel[b, free] = make_point(px // w, px % w, rad)
      self.feats[b, free] = self.rng.integers(1, 101, (free.size, self.c))
      self.taken[b, free] = True
    assert self.taken.all()

  def feats_typed(self):
    return self.feats.astype(self.dtype)


def _notes_equirect(xyz1, offset, feats, h, w, void):
  n = xyz1.shape[0]
  rel = (xyz1 - np.concatenate([offset, np.zeros((n, 1), F32)], 1)[:, :, None]).astype(F32)
  proj = warp_np.equirect_project_coords(rel)
  flat, valid, z = warp_np.splat_indices(proj, feats.astype(F32), h, w, void)
  return dict(flat=flat, valid=valid, z=z)


def _keep(notes, n, h, w):
  """The oracle's tolerance verdict per point, from its (flat, z) view."""
  flat = notes['flat'].reshape(-1)
  z = notes['z'].reshape(-1)
  zmin = np.full(n * h * w, F32(DEPTH_SCALE), F32)
  np.minimum.at(zmin, flat, z)
  return (z < (zmin[flat] + TOL).astype(F32)).reshape(notes['flat'].shape), zmin


def _check_fillers(notes, filler_mask, n, h, w):
  """No filler is occluded or invalid, and at most one goes to a pixel."""
  keep, _ = _keep(notes, n, h, w)
  assert notes['valid'][filler_mask].all(), 'an invalid filler'
  assert keep[filler_mask].all(), 'an occluded filler'
  fl = notes['flat'][filler_mask]
  assert np.unique(fl).size == fl.size, 'two fillers in one pixel'


def _tile_pixel(h, w, which, k=0):
  """A pixel (not pixel 0) in the first / last packed tile of the image; k picks among a few."""
  if which == 'first':
    return (1 + k % 3, 1 + k % 5)
  return (h - 2 - k % 3, w - 2 - k % 5)


# ------------------------------------------------------------------------------------ the cases
def _edge_pixels(h, w, rng, count=32):
  """Planted pixels of `edge`: the image's last pixel, pixels 255 and 256 of packed tile 0 (the
  record's ninth pixel bit), the first and the last pixel of tile (0, 1), random ones up to `count`."""
  must = [(h - 1, w - 1), (7, 31), (8, 0), (0, PTILE_X), (PTILE_Y - 1, 2 * PTILE_X - 1),
          (0, 1), (0, w - 1), (h - 1, 0)]
  flat = [v * w + u for v, u in must]
  assert all(0 < p < h * w for p in flat) and len(set(flat)) == len(flat)
  pool = np.setdiff1d(np.arange(1, h * w), flat)
  return flat + list(rng.permutation(pool)[:count - len(flat)])


def _build_edge(cl, variant):
  n, h, w, m = cl.n, cl.h, cl.w, cl.m
  expect = []
  culled3 = [np.zeros(3)]
  front, edge, surv = (10, 10, 10), (200, 20, 20), (30, 100, 30)
  perms = list(itertools.permutations(range(3)))
  for b in range(n):
    px = _edge_pixels(h, w, cl.rng, 32 + 8 + 4)
    tri, pairs, singles = px[:32], px[32:40], px[40:44]
    need = 3 * len(tri) + 2 * len(pairs) + len(singles)
    slots = list(cl.rng.permutation(m)[:need])
    # 32 pixels: front z0, a point ON the edge fl(z0 + 0.1f) (culled), its predecessor (survives)
    for i, p in enumerate(tri):
      v, u = divmod(int(p), w)
      cl.plant_px[b].add(int(p))
      z0_want = F32(np.exp(cl.rng.uniform(np.log(0.3), np.log(12.0))))   # several binades of z0 + 0.1f
      p0 = (pixel_dirs(h, w, v, u) * z0_want).astype(F32)
      _, z0 = equirect_view(p0[None], h, w)
      z0 = z0[0]
      z_edge = F32(z0 + TOL)
      z_surv = _f32_next(z_edge, 0)
      pts = [p0, point_with_z(h, w, v, u, z_edge), point_with_z(h, w, v, u, z_surv)]
      fts = [front, edge, surv]
      three = sorted(slots[3 * i:3 * i + 3])
      for slot, which in zip(three, perms[i % 6]):   # front / edge / survivor in every array order
        cl.put(b, slot, pts[which], fts[which])
      culled3.append(np.array(edge))
      expect.append(dict(b=b, v=v, u=u, feat=(30, 100, 30), depth=F32(z0 / F32(DEPTH_SCALE)),
                         what=f'edge: z0={z0!r}, fl(z0+0.1f)={z_edge!r} culled, its predecessor kept'))
    at = 3 * len(tri)
    # 8 pixels: two points of identical z; both survive, each channel takes its own maximum
    for i, p in enumerate(pairs):
      v, u = divmod(int(p), w)
      cl.plant_px[b].add(int(p))
      pt = (pixel_dirs(h, w, v, u) * F32(cl.rng.uniform(0.5, 6.0))).astype(F32)
      _, z0 = equirect_view(pt[None], h, w)
      cl.put(b, slots[at + 2 * i], pt, (50, 1, 1))
      cl.put(b, slots[at + 2 * i + 1], pt, (1, 60, 1))
      expect.append(dict(b=b, v=v, u=u, feat=(50, 60, 1), depth=F32(z0[0] / F32(DEPTH_SCALE)),
                         what='edge: two points of identical z, both kept'))
    at += 2 * len(pairs)
    # 4 pixels, one point each, around the untouched z-buffer value depth_scale
    ds = F32(DEPTH_SCALE)
    far = [ds, _f32_next(ds, np.inf), F32(ds + TOL), _f32_next(F32(ds + TOL), 0)]
    for i, (p, zt) in enumerate(zip(singles, far)):
      v, u = divmod(int(p), w)
      cl.plant_px[b].add(int(p))
      cl.put(b, slots[at + i], point_with_z(h, w, v, u, zt), (40, 41, 42))
      gone = i == 2
      if gone:
        culled3.append(np.array((40, 41, 42)))
      expect.append(dict(b=b, v=v, u=u, feat=(0, 0, 0) if gone else (40, 41, 42), depth=F32(1.0),
                         what=f'edge: a single point at z={zt!r} against the initial depth_scale'))
  sink = dict(feat=tuple(np.max(culled3, axis=0)), depth=F32(1.0))
  return expect, sink, None


def _build_sink(cl, variant, case):
  n, h, w, m = cl.n, cl.h, cl.w, cl.m
  b, idx = variant['image'], variant['idx']
  void3 = (cl.void,) * 3
  expect = []
  if case == 'sink_feat':
    # the ONE occluded valid point of the call: 0.5 behind a front point of its pixel
    v, u = _tile_pixel(h, w, variant['tile'], idx)
    cl.plant_px[b].add(v * w + u)
    d = pixel_dirs(h, w, v, u)
    front_idx = (idx + 1) % m if idx % 2 == 0 else (idx - 1) % m   # before and behind it in the array
    cl.put(b, idx, (d * F32(2.0)).astype(F32), (201, 202, 203))
    cl.put(b, front_idx, (d * F32(1.5)).astype(F32), (11, 12, 13))
    expect.append(dict(b=b, v=v, u=u, feat=(11, 12, 13), depth=None, what='sink_feat: the occluder'))
    sink = dict(feat=(201, 202, 203), depth=F32(1.0))
  else:
    # the uniquely nearest point of the call, invalid: rel = (0, 0.5, 0), z = 0.5 exactly
    first = void3 if case == 'sink_z' else (cl.void, 250, 240)
    cl.put(b, idx, np.array([0, 0.5, 0], F32), first)
    sink = dict(feat=(0, 0, 0) if case == 'sink_z' else (None, 250, 240), depth=F32(F32(0.5) / F32(DEPTH_SCALE)))
    if case == 'partial_void':
      # 16 more partially void points, 0.1 and more behind the minimum.  They are invalid, so they
      # reach the sink's maximum whatever their z (module docstring): quiet unless the variant is loud.
      loud = variant['loud']
      for j in range(16):
        bj = j % n
        slot = int(cl.rng.choice(cl.free_indices(bj)))
        v, u = int(cl.rng.integers(0, h)), int(cl.rng.integers(0, w))
        rad = F32(0.6) if j == 0 else F32(cl.rng.uniform(0.6, 5.0))
        cl.put(bj, slot, (pixel_dirs(h, w, v, u) * rad).astype(F32),
               (cl.void, 255, 255) if loud else (cl.void, 100 - j, 90 - j))
      if loud:
        sink['feat'] = (None, 255, 255)
  p0 = None
  if variant['p0']:
    # a valid, unoccluded filler ON the sink pixel: it shares depth and features with the sink
    cl.plant_px[0].add(0)
    slot = int(cl.free_indices(0)[len(cl.free_indices(0)) // 3])
    rad = F32(1.25)
    cl.put(0, slot, (pixel_dirs(h, w, 0, 0) * rad).astype(F32), (60, 70, 80))
    p0 = dict(rad=rad, feat=(60, 70, 80))
  return expect, sink, p0


def _build_pile(cl, variant):
  """All m points of an image in ONE pixel (not pixel 0).  7 survive: the minimum z0, 5 within
  0.05 of it and the predecessor of fl(z0 + 0.1f); a point ON that edge stands at the far end of the
  array from the minimum and is culled; everything else lies 0.2 and more behind.  The culled
  points carry features 101 .. 255 and must show at the sink only."""
  n, h, w, m = cl.n, cl.h, cl.w, cl.m
  expect = []
  sink3 = np.zeros(3)
  for b in range(n):
    v, u = (h // 2 + b, w // 3 + 2 * b)
    cl.plant_px[b].add(v * w + u)
    d = pixel_dirs(h, w, v, u)
    zmin = 2.0 + 0.25 * b
    step = 10.0 / m
    rad = np.array([zmin + 0.01 * k for k in range(6)] + [0.0] +          # kept: < z0 + 0.1
                   [zmin + 0.2 + step * j for j in range(m - 8)] + [0.0])  # culled: < 12.5 < depth_scale
    pts = (d[None, :] * rad.astype(F32)[:, None]).astype(F32)
    _, z0 = equirect_view(pts[:1], h, w)
    z_edge = F32(z0[0] + TOL)
    pts[6] = point_with_z(h, w, v, u, _f32_next(z_edge, 0))
    pts[m - 1] = point_with_z(h, w, v, u, z_edge)
    f = np.zeros((m, 3))
    for k in range(7):                                             # every channel's maximum from another point
      f[k] = (10 + (3 * k) % 7, 20 + (5 * k) % 7, 30 + k)
    f[7:] = cl.rng.integers(101, 254, (m - 7, 3))
    f[m - 1] = (255, 254, 255)
    if cl.dtype == np.float32:
      f[7:] += 0.5
    order = np.arange(m)[::-1] if variant['order'] == 'min_last' else np.arange(m)
    for slot, src in enumerate(order):
      cl.put(b, slot, pts[src], f[src])
    expect.append(dict(b=b, v=v, u=u, feat=tuple(f[:7].max(0)), depth=F32(z0[0] / F32(DEPTH_SCALE)),
                       what=f'pile: {m} points in one pixel, 7 survive, fl(z0+0.1f)={z_edge!r} culled '
                            f'({variant["order"]})'))
    sink3 = np.maximum(sink3, f[7:].max(0))
  return expect, dict(feat=tuple(sink3), depth=F32(1.0)), None


def build(case, n, h, w, c, dtype, void, m, variant=None, seed=0):
  """Returns (xyz1 (n,4,m), feats (n,m,c), offset (n,3), notes) for the equirect entry, or
  (coords (n,4,m), feats, notes) for case 'borders' (the perspective entry).  notes: per point the
  oracle's flat index / valid flag / z, `expect` (planted pixels: b, v, u, first three features,
  depth or None, what), `sink` (features, None where only the oracle can say; depth),
  `quiet` (no output feature outside the sink exceeds 100) and case-specific counts."""
  if case == 'borders':
    return _build_borders(n, h, w, c, dtype, void, m, variant or {}, seed)
  variant = variant if variant is not None else variants(case, n, m)[0]
  cl = _Cloud(n, h, w, c, dtype, void, m, seed * 1000 + h + 7 * c + m)
  if case == 'edge':
    expect, sink, p0 = _build_edge(cl, variant)
  elif case in ('sink_feat', 'sink_z', 'partial_void'):
    expect, sink, p0 = _build_sink(cl, variant, case)
  elif case == 'pile':
    expect, sink, p0 = _build_pile(cl, variant)
  else:
    raise ValueError(case)
  planted = cl.taken.copy()
  cl.fill(lambda v, u, rad: (pixel_dirs(h, w, v, u) * rad[:, None]).astype(F32))
  # exact z is planted on the relative coordinates: `edge` and `pile` render from the origin; the
  # other cases move the cloud by an exactly representable offset that the splat takes off again
  offset = np.zeros((n, 3), F32) if case in ('edge', 'pile') else np.tile(OFFSET, (n, 1))
  xyz = (cl.rel + offset[:, None, :]).astype(F32)
  xyz1 = np.ascontiguousarray(np.concatenate([xyz.transpose(0, 2, 1), np.ones((n, 1, m), F32)], 1))
  feats = cl.feats_typed()
  notes = _notes_equirect(xyz1, offset, feats, h, w, void)
  keep, _ = _keep(notes, n, h, w)
  _check_fillers(notes, ~planted, n, h, w)
  valid = notes['valid']
  notes.update(expect=expect, sink=sink, quiet=case != 'pile' and case != 'edge' and not
               (variant.get('loud')), planted=planted, case=case, variant=variant)
  # ---- preconditions, on the oracle's own view
  if p0 is not None:
    _, zp = equirect_view((pixel_dirs(h, w, 0, 0) * p0['rad']).astype(F32)[None], h, w)
    if sink['depth'] > F32(zp[0] / F32(DEPTH_SCALE)):
      sink['depth'] = F32(zp[0] / F32(DEPTH_SCALE))
    sink['feat'] = tuple(None if s is None else max(s, f) for s, f in zip(sink['feat'], p0['feat']))
    assert (notes['flat'][0][valid[0]] == 0).sum() == 1, 'the filler on the sink pixel'
  else:
    assert not (valid & (notes['flat'] == 0)).any(), 'a valid point on the sink pixel'
  occluded = valid & ~keep
  if case == 'edge':
    assert occluded.sum() == n * 33 and (~valid).sum() == 0
    for e in expect:
      at = valid[e['b']] & (notes['flat'][e['b']] == e['b'] * h * w + e['v'] * w + e['u'])
      assert at.sum() in (1, 2, 3), e
  elif case == 'sink_feat':
    assert occluded.sum() == 1 and (~valid).sum() == 0, (occluded.sum(), (~valid).sum())
    assert occluded[variant['image'], variant['idx']]
    assert cl.feats[~occluded][:, :3].max() <= 100
  elif case in ('sink_z', 'partial_void'):
    z = notes['z']
    b, idx = variant['image'], variant['idx']
    assert z[b, idx] == F32(0.5) and not valid[b, idx]
    others = np.delete(z.reshape(-1), b * m + idx)
    assert others.min() >= (F32(0.6) if case == 'partial_void' else F32(1.0)), others.min()
    # (the filler on the sink pixel lies 0.1 behind the invalid minimum that shares its pixel: the
    #  tolerance sends it to flat index 0, where it is already)
    assert occluded.sum() == (1 if variant['p0'] else 0)
    assert (~valid).sum() == (17 if case == 'partial_void' else 1)
  elif case == 'pile':
    assert valid.all() and (keep.sum(1) == 7).all(), keep.sum(1)
    assert all(np.unique(notes['flat'][b]).size == 1 and notes['flat'][b, 0] != 0 for b in range(n))
  return xyz1, feats, offset, notes


# ------------------------------------------------------------------ perspective entry: borders
def _v_for_fx(fx, size):
  """View coordinates v (fp32) for a wanted pixel coordinate fx: [(v, fx)] where the oracle's chain
  fl(fl(fl(v + 1) / 2) * size) gives fx exactly; where no v does (fx = -1 at a size that is no
  power of two: fl(v + 1) moves in steps of 2^-23 there), the two v whose chain values bracket fx
  most closely -- one on either side of the border."""
  fx = F32(fx)
  v0 = F32(2.0 * np.float64(fx) / size - 1.0)
  cand = (v0.view(np.int32) + np.arange(-8, 9, dtype=np.int32)).view(F32) if v0 != 0 else np.array([v0], F32)
  got = ((cand + F32(1)) / F32(2) * F32(size)).astype(F32)
  hit = np.nonzero(got == fx)[0]
  if hit.size:
    return [(cand[hit[0]], fx)]
  below, above = got < fx, got > fx
  assert below.any() and above.any(), (fx, size)
  lo = np.nonzero(below)[0][np.argmax(got[below])]
  hi = np.nonzero(above)[0][np.argmin(got[above])]
  return [(cand[lo], got[lo]), (cand[hi], got[hi])]


def border_coords(size):
  """(v, fx, valid) of the planted view coordinates along one axis of `size` pixels.  The oracle
  truncates toward zero: fx = -0.5 is pixel 0 and valid, fx = size is not.  (fx = -0.0 cannot be
  planted: fl(v + 1) is +0 for v = -1 under round-to-nearest; the signed zero enters as v = -0.0,
  i.e. x = -0.0, which lands on size / 2.)"""
  wanted = [-1.0, -0.5, 0.0, 5.0, 7.5, float(size - 1), float(_f32_next(size, 0)), float(size)]
  out = [(v, fx, bool(-1.0 < fx < size)) for want in wanted for v, fx in _v_for_fx(want, size)]
  return out + [(F32(-0.0), F32(size / 2), True)]


def _build_borders(n, h, w, c, dtype, void, m, variant, seed):
  rng = np.random.default_rng(seed * 1000 + 31 * h + c)
  coords = np.zeros((n, 4, m), F32)
  coords[:, 3] = 1
  feats = np.zeros((n, m, c), np.float64)
  taken = np.zeros((n, m), bool)
  want_valid = np.zeros((n, m), bool)
  xs, ys = border_coords(w), border_coords(h)
  zs = [F32(0.5), F32(1), F32(2), F32(4), F32(8), F32(1), F32(2.0 ** -3)]
  fmax = 256 if dtype != np.float32 else 250

  def feat():
    f = rng.integers(1, fmax, c).astype(np.float64)
    if dtype == np.float32:
      f = f * 0.5 - 4.0          # negatives above the output void -5; never the input void -1
      f[f == void] = 0.25
    return f

  for b in range(n):
    plants = []
    for i, ((vx, _, okx), (vy, _, oky)) in enumerate(itertools.product(xs, ys)):
      z = zs[(i + b) % len(zs)]                    # a power of two: x = v * z and x / z are exact
      plants.append((vx * z, vy * z, z, feat(), okx and oky))
    for i in range(6):                              # behind the camera: invalid, the sink's minimum goes negative
      plants.append((F32(0.25) * i, F32(-0.5), F32(-1), feat(), False))
    for z in (F32(0.0), F32(-0.0)):                 # div_no_nan: view coordinates 0, z > 0 fails
      plants.append((F32(3), F32(-2), z, feat(), False))
      plants.append((F32(0), F32(0), z, feat(), False))
    pv = feat()                                     # void features on a point that is in view
    pv[0] = void
    plants.append((F32(0.1), F32(0.1), F32(1), pv, False))
    slots = rng.permutation(m)[:len(plants)]
    for slot, (x, y, z, f, ok) in zip(slots, plants):
      coords[b, 0, slot], coords[b, 1, slot], coords[b, 2, slot] = x, y, z
      feats[b, slot] = f
      taken[b, slot] = True
      want_valid[b, slot] = ok
  planted = taken.copy()
  flat_p, valid_p, _ = warp_np.splat_indices(coords, feats.astype(dtype).astype(F32), h, w, void)
  for b in range(n):
    busy = set((flat_p[b][valid_p[b] & planted[b]] - b * h * w).tolist()) | ({0} if b == 0 else set())
    free = np.nonzero(~taken[b])[0]
    pool = np.array([p for p in range(h * w) if p not in busy])
    assert free.size <= pool.size
    px = rng.permutation(pool)[:free.size]
    z = rng.uniform(1.0, 3.0, free.size).astype(F32)
    vx = ((2.0 * (px % w) + 1.0) / w - 1.0).astype(F32)
    vy = ((2.0 * (px // w) + 1.0) / h - 1.0).astype(F32)
    coords[b, 0, free], coords[b, 1, free], coords[b, 2, free] = vx * z, vy * z, z
    feats[b, free] = rng.integers(1, 101, (free.size, c))
    taken[b, free] = True
    want_valid[b, free] = True
  feats = feats.astype(dtype)
  flat, valid, z = warp_np.splat_indices(coords, feats.astype(F32), h, w, void)
  notes = dict(flat=flat, valid=valid, z=z, planted=planted, case='borders', variant=variant,
               expect=[], sink=dict(feat=(None, None, None), depth=F32(0.0)), quiet=False)
  # ---- preconditions: the oracle's valid flags are the stated ones; fillers alone in their pixels
  np.testing.assert_array_equal(valid, want_valid)
  _check_fillers(notes, ~planted, n, h, w)
  for b in range(n):   # the corner and border pixels are hit
    got = set((flat[b][valid[b] & planted[b]] - b * h * w).tolist())
    assert {w - 1, (h - 1) * w, h * w - 1, 5 * w + 7, (h // 2) * w + w // 2} <= got | {0}, sorted(got)[:8]
  return coords, feats, notes


# ------------------------------------------------------------------------- what a result must show
def check_expected(notes, depth, out, label):
  """The stated values at the planted pixels and at the sink, on outputs depth (n,h,w), out
  (n,h,w,c) of either an oracle or the device."""
  c = out.shape[-1]
  k = min(c, 3)
  msg = f'{label} [{notes["case"]} {variant_id(notes["variant"])}]'
  for e in notes['expect']:
    got = out[e['b'], e['v'], e['u'], :k]
    assert tuple(got) == tuple(F32(x) for x in e['feat'][:k]), f'{msg}: {e["what"]}: features {got} at {e["b"], e["v"], e["u"]}, expected {e["feat"][:k]}'
    if e['depth'] is not None:
      assert depth[e['b'], e['v'], e['u']] == e['depth'], f'{msg}: {e["what"]}: depth {depth[e["b"], e["v"], e["u"]]!r}, expected {e["depth"]!r}'
  sink = notes['sink']
  assert depth[0, 0, 0] == sink['depth'], f'{msg}: sink depth {depth[0, 0, 0]!r}, expected {sink["depth"]!r}'
  for ch in range(k):
    if sink['feat'][ch] is not None:
      assert out[0, 0, 0, ch] == F32(sink['feat'][ch]), f'{msg}: sink channel {ch} is {out[0, 0, 0, ch]}, expected {sink["feat"][ch]}'
  if notes['quiet']:
    rest = out.reshape(-1, c)[1:]
    assert rest.max() <= 100, f'{msg}: {rest.max()} outside the sink'
