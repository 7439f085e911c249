"""Oracle and inputs of the .ply tests (tests/test_ply_cpu.py, tests/test_ply_gpu.py).

The oracle is the host loop of SE3DSModel.write_memory_as_pointcloud as it stood before
se3ds_amd/utils/ply.py existed, written out again here so that the tests do not compare the module
with itself: one '{}'.format per value, Python's own text of np.float32 / np.int32 / np.uint8
scalars."""
import numpy as np

HEADER_ASCII = ('ply\nformat ascii 1.0 \nelement vertex %d\nproperty float x\nproperty float y\n'
                'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
HEADER_BINARY = ('ply\nformat binary_little_endian 1.0 \nelement vertex %d\nproperty float x\nproperty float y\n'
                 'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
RECORD = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])

COLOURS_I32 = (-2147483648, -1, 0, 9, 10, 99, 100, 255, 256, 2147483647)
COLOURS_U8 = (0, 9, 10, 99, 100, 255)


def ascii_body(xyz, rgb) -> bytes:
  """xyz (M, 3) float32, rgb (M, 3) int32 or uint8, host arrays -> the lines of the host loop."""
  lines = []
  for i in range(xyz.shape[0]):
    lines.append('{} {} {} {} {} {} \n'.format(xyz[i, 0], xyz[i, 1], xyz[i, 2], rgb[i, 0], rgb[i, 1], rgb[i, 2]))
  return ''.join(lines).encode('ascii')


def ascii_file(coords, rgb) -> bytes:
  """coords (3 or 4, M) float32 as the model keeps them, rgb (M, 3): the whole file."""
  xyz = np.asarray(coords)[0:3].T
  return (HEADER_ASCII % xyz.shape[0]).encode('ascii') + ascii_body(xyz, np.asarray(rgb))


def binary_file(coords, rgb) -> bytes:
  xyz = np.asarray(coords)[0:3]
  rec = np.zeros((xyz.shape[1],), RECORD)
  rec['x'], rec['y'], rec['z'] = xyz[0], xyz[1], xyz[2]
  rec['red'], rec['green'], rec['blue'] = (np.asarray(rgb)[:, k] for k in range(3))
  return (HEADER_BINARY % xyz.shape[1]).encode('ascii') + rec.tobytes()


def _bits(x) -> int:
  return int(np.array(x, np.float32).view(np.uint32))


def adversarial_bits() -> np.ndarray:
  """fp32 bit patterns at which a formatter goes wrong, each with both signs: zeros, 0.1f, both
  neighbours of 1e-4 and of 1e16 (the positional / scientific switch) and the nearest values
  themselves, 2^24, 123456792, the largest finite value, the smallest normal and subnormal, every
  2^k (k = -149 .. 127) with both neighbouring patterns, quiet and signalling NaNs, infinities."""
  pos = [0, _bits(0.1), _bits(16777216.0), _bits(123456792.0), 0x7f7fffff, 0x00800000, 0x00000001,
         0x7fc00000, 0x7f800001, 0x7fffffff, 0x7fc12345, 0x7f800000]
  for edge in (1e-4, 1e16):
    b = _bits(edge)
    pos += [b - 1, b, b + 1]
  for k in range(-149, 128):
    b = 1 << (k + 149) if k < -126 else (k + 127) << 23
    pos += [b - 1, b, b + 1]
  out = []
  for b in pos:
    out += [b, b | 0x80000000]
  return np.array(out, dtype=np.uint32)


def inputs(m, seed, colour_dtype=np.int32):
  """coords (3, m) float32 and rgb (m, 3): every second value walks the adversarial set (all of it
  once 3 m / 2 reaches its length), the others are N(0, 0.3) coordinates; likewise the colours."""
  rng = np.random.default_rng(seed)
  adv = adversarial_bits()
  bits = rng.normal(0.0, 0.3, 3 * m).astype(np.float32).view(np.uint32).copy()
  at = np.arange(0, 3 * m, 2)
  bits[at] = adv[(at // 2 + seed) % len(adv)]
  coords = bits.view(np.float32).reshape(m, 3).T.copy()   # consecutive values share a line
  edge = np.array(COLOURS_I32 if colour_dtype == np.int32 else COLOURS_U8, dtype=np.int64)
  rgb = rng.integers(0, 256, 3 * m)
  rgb[at] = edge[(at // 2 + seed) % len(edge)]
  return coords, rgb.astype(colour_dtype).reshape(m, 3)
