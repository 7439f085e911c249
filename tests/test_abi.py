"""CPU test: libse3ds_hip.so builds for gfx950, loads, and exports every symbol that
include/se3ds_hip.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

from se3ds_amd import _lib
from se3ds_amd.csrc import build as hip_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
  text = open(os.path.join(ROOT, 'include', 'se3ds_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(se3ds_[a-z0-9_]+)\s*\(', text)))


def test_library_builds_and_exports_every_declared_symbol():
  so = hip_build.build()
  assert os.path.exists(so)
  lib = ctypes.CDLL(so)
  names = _declared()
  assert len(names) >= 10
  for name in names:
    assert hasattr(lib, name), f'{name} declared in include/se3ds_hip.h but not exported'
  assert lib.se3ds_version
  lib.se3ds_version.restype = ctypes.c_char_p
  assert b'gfx950' in lib.se3ds_version()


def test_python_binding_table_matches_header():
  """_lib derives its table from the header; _declared() finds the names with an expression of its
  own, so a declaration the parser skipped shows here."""
  assert _lib.declared_symbols() == _declared()
  L = _lib.lib()  # binds every signature; AttributeError if one is missing
  for name in _declared():
    assert getattr(L, name).argtypes is not None, name


c_int, c_i64, c_f, c_p, c_sz, c_d = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_double)
c_u32 = ctypes.c_uint32
# Rows of the hand-written tables that the header parser replaced: every scalar type, both special
# returns and the widest calls.
PINNED = {
    'se3ds_version': (ctypes.c_char_p, []),
    'se3ds_debug_conv_route_name': (ctypes.c_char_p, [c_int]),
    'se3ds_splat_workspace_bytes': (c_sz, [c_int, c_i64, c_int, c_int, c_int]),
    'se3ds_ply_max_points': (c_i64, []),
    'se3ds_project_equirect': (c_int, [c_p, c_p, c_p, c_int, c_int, c_i64, c_int, c_int, c_int,
                                       c_f, c_f, c_f, c_p, c_p, c_p, c_f, c_p, c_sz, c_p]),
    'se3ds_warp_views_to_target': (c_int, [c_p, c_int, c_p, c_p, c_int, c_int, c_int, c_int, c_int,
                                           c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_p,
                                           c_int, c_int, c_f, c_p, c_p, c_p, c_f, c_p, c_sz, c_p]),
    'se3ds_conv2d_fwd_stats': (c_int, [c_p, c_p, c_p, c_int] + [c_int] * 13 + [c_p, c_int, c_p, c_p,
                                                                            c_p, c_p, c_int, c_f, c_p,
                                                                            c_p]),
    'se3ds_norm_bwd_cg': (c_int, [c_p, c_p, c_int, c_i64, c_int, c_p, c_p, c_p, c_f, c_int, c_f, c_p,
                                  c_p, c_p, c_int, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    'se3ds_multi_clip_adam_keras_ema': (c_int, [c_p, c_p, c_p, c_p, c_p, c_i64, c_p, c_f, c_p, c_f, c_f,
                                                c_f, c_f, c_i64, c_p, c_f, c_p]),
    'se3ds_f64_gemm': (c_int, [c_p, c_p, c_p, c_int, c_d, c_d, c_p]),
    'se3ds_sqrt_trace': (c_int, [c_p, c_int, c_int, c_d, c_p, c_p, c_sz, c_p, c_p]),
    'se3ds_adler32_combine': (c_u32, [c_u32, c_u32, c_i64]),
    'se3ds_fastdiv_host': (c_u32, [c_u32, c_u32]),
    'se3ds_nn_inpaint': (c_int, [c_p, c_int, c_u32, c_int, c_int, c_int, c_p, c_p, c_p, c_sz,
                                 c_int, c_p]),
}


def test_pinned_signatures():
  L = _lib.lib()
  assert [len(PINNED[n][1]) for n in ('se3ds_warp_views_to_target', 'se3ds_conv2d_fwd_stats',
                                      'se3ds_norm_bwd_cg')] == [30, 27, 25]
  for name, (res, args) in PINNED.items():
    assert _lib._SIGS[name] == (res, args), name
    fn = getattr(L, name)
    assert fn.restype is res and list(fn.argtypes) == args, name


def test_parser_reads_the_declaration_forms_of_the_header():
  sigs, abi = _lib.parse_header('''
      /* se3ds_in_a_comment(long x); */
      #ifdef __cplusplus
      extern "C" {
      #endif
      #define SE3DS_GUARD_
      #define SE3DS_A 7
      #define SE3DS_B (-3)
      #  define SE3DS_C 0x1F  /* trailing comment */
      int se3ds_split(const void* a,
                      int64_t n,
          size_t bytes);
      int se3ds_commented(float x, /* between */ double y,  // to the end of the line
                          uint32_t z);
      const char* se3ds_name(void);
      size_t se3ds_tables(const float* const* p, int n);
      #ifdef __cplusplus
      }
      #endif
      ''')
  assert sigs == {
      'se3ds_split': (c_int, [c_p, c_i64, c_sz]),
      'se3ds_commented': (c_int, [c_f, c_d, c_u32]),
      'se3ds_name': (ctypes.c_char_p, []),
      'se3ds_tables': (c_sz, [c_p, c_int]),
  }
  assert abi == {'SE3DS_A': 7, 'SE3DS_B': -3, 'SE3DS_C': 31}


def test_parser_refuses_what_it_has_no_rule_for():
  import pytest
  for params in ('long n', 'unsigned n', 'int dims[4]', 'void (*cb)(int)', 'struct S s', 'int n, ...',
                 'const float* rows[4]', ''):
    with pytest.raises(ValueError, match=r'\bse3ds_bad\b'):
      _lib.parse_header(f'int se3ds_ok(int n);\nint se3ds_bad(void* p, {params});\n')
  for text in ('long se3ds_bad(int n);', 'void* se3ds_bad(void);', 'int se3ds_bad(int n) { return n; }',
               'int (*se3ds_bad(int n))(void);'):
    with pytest.raises(ValueError, match=r'\bse3ds_bad\b'):
      _lib.parse_header(text)
  with pytest.raises(ValueError, match='SE3DS_BAD'):
    _lib.parse_header('#define SE3DS_BAD (1 << 3)\n')


def _defined():
  text = open(os.path.join(ROOT, 'include', 'se3ds_hip.h')).read()
  return {k: int(v, 0) for k, v in re.findall(r'#define\s+(SE3DS_\w+)\s+\(?(-?\w+)\)?\s*$', text, re.M)}


def test_abi_constants_come_from_the_header():
  from se3ds_amd.utils import inception_utils, point_cloud_utils, utils
  defined = _defined()
  assert len(defined) >= 19 and _lib.ABI == defined
  legacy = {
      'SE3DS_F32': _lib.F32, 'SE3DS_I32': _lib.I32, 'SE3DS_U8': _lib.U8, 'SE3DS_BF16': _lib.BF16,
      'SE3DS_FEAT_BYTE_RANGE': point_cloud_utils.FEAT_BYTE_RANGE,
      'SE3DS_XYZ1_ONES_PRESET': point_cloud_utils.XYZ1_ONES_PRESET,
      'SE3DS_SEQ_IOU': utils._SEQ_IOU, 'SE3DS_SEQ_ACCURACY': utils._SEQ_ACCURACY,
      'SE3DS_SEQ_IOU_LABELS': utils._SEQ_IOU_LABELS,
      'SE3DS_SQRT_CONVERGED': inception_utils.SQRT_CONVERGED,
      'SE3DS_SQRT_CAP_REACHED': inception_utils.SQRT_CAP_REACHED,
      'SE3DS_SQRT_NONFINITE': inception_utils.SQRT_NONFINITE,
  }
  for name, value in legacy.items():
    assert value == _lib.ABI[name] == defined[name], name
  # the values the kernels were built with, as the hand-written copies had them
  assert [_lib.F32, _lib.I32, _lib.U8, _lib.BF16] == [0, 1, 2, 3]
  assert (point_cloud_utils.FEAT_BYTE_RANGE, point_cloud_utils.XYZ1_ONES_PRESET) == (0x100, 0x200)


def test_check_names_the_error_code():
  import pytest
  errors = {k: v for k, v in _lib.ABI.items() if k.startswith('SE3DS_E_')}
  assert sorted(errors.values()) == [-5, -4, -3, -2, -1]
  for name, code in errors.items():
    with pytest.raises(_lib.Se3dsHipError) as e:
      _lib.check(code, 'se3ds_probe')
    assert str(e.value).startswith(f'se3ds_probe failed: {name} '), str(e.value)
  with pytest.raises(_lib.Se3dsHipError) as e:
    _lib.check(-77, 'se3ds_probe')
  assert str(e.value).startswith('se3ds_probe failed: SE3DS_E_-77 ')
  _lib.check(_lib.ABI['SE3DS_OK'], 'se3ds_probe')


def test_no_cpu_fallback():
  import pytest
  import torch
  from se3ds_amd.utils import pano_utils
  with pytest.raises(_lib.Se3dsHipError):
    pano_utils.mask_pano(torch.zeros((1, 8, 16, 3)))


def test_fastdiv_matches_integer_division():
  """The conv kernels turn a tile row into (image, row, column) with host-made multipliers instead of
  divisions (csrc/conv.hip FastDiv: q = (t + ((n - t) >> s1)) >> s2, t = mulhi(n, m)).  The same
  arithmetic evaluated on the host (se3ds_fastdiv_host) must equal n // d for every divisor class:
  1, powers of two, odd, the image sizes of the configs, large -- at the edges of the 32-bit range."""
  import random
  import se3ds_amd.hipops  # noqa: F401
  L = _lib.lib()
  rng = random.Random(5)
  divisors = [1, 2, 3, 5, 7, 16, 17, 31, 32, 33, 64, 129, 255, 256, 257, 512, 513, 1024, 2048, 32 * 64,
              129 * 257, 512 * 1024, 1024 * 2048, 1000003, 2 ** 20 + 1, 2 ** 30, 2 ** 31 - 1, 2 ** 31,
              2 ** 32 - 1] + [rng.randrange(1, 2 ** 31) for _ in range(40)]
  for d in divisors:
    ns = [0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    ns += [k * d + r for k in (3, 1000, 65535) for r in (-1, 0, 1)]
    ns += [rng.randrange(0, 2 ** 32) for _ in range(200)]
    for n in ns:
      if 0 <= n < 2 ** 32:
        assert L.se3ds_fastdiv_host(n, d) == n // d, (n, d)


def test_conv_route_report_names_are_unique_and_end_with_null():
  """se3ds_debug_conv_route_name enumerates the convolution family's kernel instantiations (host
  only); tests/test_conv_lattice_gpu.py keeps one bit-exact case per name.  Before any launch of the
  calling thread the report is -1, as is a look further back than the ring remembers."""
  import se3ds_amd.hipops  # noqa: F401
  L = _lib.lib()
  names, i = [], 0
  while L.se3ds_debug_conv_route_name(i) is not None:
    names.append(L.se3ds_debug_conv_route_name(i).decode())
    i += 1
  assert len(names) == len(set(names)) >= 60
  assert L.se3ds_debug_conv_route_name(-1) is None and L.se3ds_debug_conv_route_name(len(names)) is None
  for family in ('halo256_fwd_m16', 'big128_dgrad_bn_m32', 'glds_f32_fwd', 'igemm_bf16_dgrad',
                 'wgrad_taps3_m16', 'wgrad_reduce_multi', 'thin_cout_wgrad_t5', 'weight_prep_multi'):
    assert family in names
  assert L.se3ds_debug_conv_route_history(8) == -1 and L.se3ds_debug_conv_route_history(-1) == -1
  # a fresh process has launched nothing: the report is -1
  import subprocess
  import sys
  code = ('import se3ds_amd.hipops; from se3ds_amd import _lib; L = _lib.lib(); '
          'print(L.se3ds_debug_last_conv_route(), L.se3ds_debug_conv_route_history(0))')
  r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, check=True)
  assert r.stdout.split() == ['-1', '-1'], r.stdout
