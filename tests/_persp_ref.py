"""The pinned-order statement of the perspective and pano-rotation warps: the yardstick of
tests/test_persp_ref_cpu.py and tests/test_persp_exact_gpu.py.  Nothing here looks at the code
under test.

It is oracle/warp_np.py's statement with ONE difference: every 3-term product is spelled out as
((a*b + c*d) + e*f) on elementwise fp32 arrays, one rounding per operation -- `@`, matmul and
einsum never appear, so the summation order is defined.  That is the order csrc/geom.hip's comments
state.  There are two such products:

  matrix times column      (m0*r0 + m1*r1) + m2*r2          rotate_coords, perspective_coords
  row vector times matrix  (p0*k0 + p1*k3) + p2*k6          [px, py, 1] . K^-T, then . R

Everything else -- the pixel rays, the binary64-evaluated once-rounded transcendentals, the
lon/lat <-> uv maps, tfa's bilinear gather, the equirect unprojection and the 3x3 host transform --
is imported from oracle.warp_np and used as is.

The small named steps (_pixel_decode, _round, _in_front, _pad and the imported
interpolate_bilinear) are module attributes so that test_persp_ref_cpu.py can plant an error in
one of them and show which cases notice."""
import numpy as np

from oracle.warp_np import (  # noqa: F401  (re-exported: the parts used as they are)
    PI32, TWO_PI32, _acos32, _asin32, _atan2_32, _lonlat_to_uv, _xyz_to_lonlat,
    equirectangular_pixel_rays, equirectangular_to_pointcloud, get_world_to_image_transform,
    interpolate_bilinear)

F32 = np.float32


def _f(x):
  return np.asarray(x, F32)


def _prod3(a, b, c, d, e, f):
  """((a*b + c*d) + e*f), every operation rounded to fp32."""
  ab = (_f(a) * _f(b)).astype(F32)
  cd = (_f(c) * _f(d)).astype(F32)
  ef = (_f(e) * _f(f)).astype(F32)
  return ((ab + cd).astype(F32) + ef).astype(F32)


def mat_times_columns(m, rays):
  """m (3,3), rays (3,Q) -> x, y, z (Q,): row i of m with the column, in the pinned order."""
  m, rays = _f(m), _f(rays)
  r0, r1, r2 = rays[0], rays[1], rays[2]
  return tuple(_prod3(m[i, 0], r0, m[i, 1], r1, m[i, 2], r2) for i in range(3))


def rows_times_mat(p0, p1, p2, m):
  """row vectors (p0, p1, p2) (Q,) times m (3,3) -> three (Q,) components, pinned order."""
  m = _f(m)
  return tuple(_prod3(p0, m[0, j], p1, m[1, j], p2, m[2, j]) for j in range(3))


# ------------------------------------------------------------------------- the named steps
def _pixel_decode(total, height, width):
  """Query i of a (height, width) view is the pixel (x, y) = (i % width, i // width)."""
  i = np.arange(total, dtype=np.int64)
  return (i % width).astype(F32), (i // width).astype(F32)


def _round(x):
  """tf.math.round: half to even."""
  return np.round(x).astype(F32)


def _in_front(z):
  return z > 0


def _pad(image, value):
  """One pixel of `value` around a (1, h, w, C) image."""
  return np.pad(image, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='constant', constant_values=value)


# ------------------------------------------------------------------- coordinate functions
def rotate_coords(matrix, rays, src_h, src_w):
  """matrix (N,3,3), rays (3,Q) -> (N,Q,2) [pitch_px, heading_px] (warp_np.rotate_coords)."""
  matrix = _f(matrix)
  out = []
  for m in matrix:
    x, y, z = mat_times_columns(m, rays)
    pitch = _acos32((-y).astype(F32))
    heading = _atan2_32(x, z)
    hp = ((heading / TWO_PI32).astype(F32) + F32(0.5)).astype(F32)
    hp = (hp * F32(src_w - 1)).astype(F32)
    pp = ((pitch / PI32).astype(F32) * F32(src_h - 1)).astype(F32)
    out.append(np.stack([pp, hp], axis=-1))
  return np.stack(out).astype(F32)


def perspective_coords(world_to_image, rays, round_to_nearest=False, add=None):
  """world_to_image (3,3), rays (3,Q) -> (Q,2) (warp_np.perspective_coords); `add`, when given,
  is added last, as the C entry point does."""
  x, y, z = mat_times_columns(world_to_image, rays)
  front = _in_front(z)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    cx = np.where(front, (x / z).astype(F32), F32(-1)).astype(F32)
    cy = np.where(front, (y / z).astype(F32), F32(-1)).astype(F32)
  coords = np.stack([cx, cy], axis=-1)
  if round_to_nearest:
    coords = _round(coords)
  if add is not None:
    coords = (coords + F32(add)).astype(F32)
  return coords.astype(F32)


def inverse_intrinsics_t(camera_intrinsics):
  """K^-T as warp_np forms it: the binary64 inverse, rounded once, transposed."""
  return np.ascontiguousarray(np.linalg.inv(np.asarray(camera_intrinsics, np.float64)).astype(F32).T)


def perspective_from_equirect_coords(kinv_t, rotation_matrix, height, width, eq_h, eq_w):
  """(height*width, 2) = (u, v) (warp_np.perspective_from_equirect_coords)."""
  px, py = _pixel_decode(int(height) * int(width), int(height), int(width))
  pz = np.ones_like(px)
  a0, a1, a2 = rows_times_mat(px, py, pz, kinv_t)
  x, y, z = rows_times_mat(a0, a1, a2, rotation_matrix)
  xyz = np.stack([x, y, z], axis=-1).astype(F32)
  with np.errstate(divide='ignore', invalid='ignore'):
    uv = _lonlat_to_uv(_xyz_to_lonlat(xyz), (eq_h, eq_w))
  return uv.reshape(-1, 2).astype(F32)


# ------------------------------------------------------------------------------ composites
def rotate_pano(pano, matrix):
  """warp_np.rotate_pano."""
  pano = _f(pano)
  n, h, w, c = pano.shape
  coords = rotate_coords(matrix, equirectangular_pixel_rays(h), h, w)
  return interpolate_bilinear(pano, coords).reshape(n, h, w, c)


def project_perspective_image(image, fov, output_height, camera_intrinsics=None, rotations=None,
                              rotation_matrix=None, pad_mode='constant', pad_value=0.0,
                              round_to_nearest=False):
  """warp_np.project_perspective_image: image (h, w, C) -> (H, 2H, C), all three pad modes."""
  assert pad_mode in {'reflect', 'constant', 'mean'}
  image = _f(image)[None]
  w2i = get_world_to_image_transform((image.shape[1], image.shape[2]), fov,
                                     camera_intrinsics=camera_intrinsics, rotations=rotations,
                                     rotation_matrix=rotation_matrix)
  coords = perspective_coords(w2i, equirectangular_pixel_rays(output_height), round_to_nearest)
  if pad_mode != 'reflect':
    cv = F32(np.mean(image.astype(np.float64))) if pad_mode == 'mean' else F32(pad_value)
    image = _pad(image, cv)
    coords = (coords + F32(1.0)).astype(F32)
  out = interpolate_bilinear(image, coords[None], indexing='xy')
  return out.reshape(output_height, 2 * output_height, -1)


def get_perspective_from_equirectangular_image(image, camera_intrinsics, rotation_matrix, height,
                                               width, uv=None):
  """warp_np.get_perspective_from_equirectangular_image; `uv` reuses coordinates already formed
  for the same view (they depend on the shapes and matrices only)."""
  image = np.asarray(image)
  eh, ew, c = image.shape
  if uv is None:
    uv = perspective_from_equirect_coords(inverse_intrinsics_t(camera_intrinsics), rotation_matrix,
                                          height, width, eh, ew)
  out = interpolate_bilinear(image.astype(F32)[None], uv[None], indexing='xy')
  return out.reshape(height, width, c)


def cell15_pointcloud(image01, depth01, camera_intrinsics, rotation_matrix, eq_height, void_class=-1,
                      depth_scale=20.0, position=None, pad_value=0.0, round_to_nearest=True):
  """warp_np.notebook_cell15_pointcloud with the fused kernel's further arguments: image01
  (h,w,C), C = 1..4, depth01 (h,w); `pad_value` pads both; `position` (3,) is added to x, y, z of
  every point, as models.py does after the unprojection.  -> xyz1 (1,4,P), feats (1,P,C) int32."""
  kw = dict(camera_intrinsics=camera_intrinsics, rotation_matrix=rotation_matrix,
            pad_value=pad_value, round_to_nearest=round_to_nearest)
  img_t = project_perspective_image(image01, None, eq_height, **kw)
  depth_t = project_perspective_image(_f(depth01)[..., None], None, eq_height, **kw)
  proj_depth = depth_t[None, ..., 0]
  proj_feats = (img_t[None] * F32(255)).astype(F32).astype(np.int32)   # tf.cast truncates
  xyz1, feats = equirectangular_to_pointcloud(proj_feats, proj_depth, void_class, depth_scale)
  if position is not None:
    pos = _f(position).reshape(3)
    xyz1 = xyz1.copy()
    xyz1[:, :3] = (xyz1[:, :3] + pos[None, :, None]).astype(F32)
  return xyz1.astype(F32), feats


def cell17_guidance(pred_rgb, pred_depth, camera_intrinsics, new_rotation_matrix, pers_height,
                    pers_width):
  """warp_np.notebook_cell17_guidance: -> proj_image (1,h,w,3), proj_depth, proj_mask (1,h,w,1)."""
  pred_rgb, pred_depth = _f(pred_rgb), _f(pred_depth)
  eh, ew = pred_depth.shape
  uv = perspective_from_equirect_coords(inverse_intrinsics_t(camera_intrinsics), new_rotation_matrix,
                                        pers_height, pers_width, eh, ew)
  g = lambda img: get_perspective_from_equirectangular_image(img, camera_intrinsics,
                                                             new_rotation_matrix, pers_height,
                                                             pers_width, uv=uv)
  rgb_g = np.clip((g(pred_rgb) / F32(255)).astype(F32), 0, 1)[None]
  depth_g = g(pred_depth[..., None])[None]
  m = ((pred_depth != 1.0) & (pred_depth != 0.0) & np.all(pred_rgb != 0.0, axis=-1)).astype(F32)
  mask_g = (g(m[..., None])[None] == 1.0).astype(F32)
  return (mask_g * rgb_g).astype(F32), (mask_g * depth_g).astype(F32), mask_g
