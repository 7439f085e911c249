"""ctypes binding of libse3ds_hip.so, derived from include/se3ds_hip.h: the header is the only
signature table and the only list of ABI constants.  There is NO fallback: if the library is
missing or a GPU entry point fails, the caller gets an exception."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SE3DS_LIB: another build of the library for this process (the A/B scripts under tools/probes/ compare
# two builds on one box; they used to copy over the in-tree file and a killed job left the wrong one
# behind -- ADVICE r5).  Unset: the in-tree build, the only one the tests and the bench ever load.
SO_PATH = os.environ.get('SE3DS_LIB') or os.path.join(_HERE, 'csrc', 'libse3ds_hip.so')
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'se3ds_hip.h')

c_int, c_i64, c_f, c_p, c_sz = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                ctypes.c_size_t)
c_d = ctypes.c_double
_SCALARS = {'int': c_int, 'int64_t': c_i64, 'size_t': c_sz, 'float': c_f, 'double': c_d,
            'uint32_t': ctypes.c_uint32}
_DECL = re.compile(r'([\w\s*]+?)\b(se3ds_\w+)\s*\(([^()]*)\)')
_INT = re.compile(r'\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?')


def _ctype(decl, name, is_param):
  """ctypes class of one parameter (type and optional name) or of a return type."""
  words = [w for w in decl.split() if w != 'const']
  if re.fullmatch(r'[\w\s*]+', decl):   # no array, function-pointer or variadic declarator
    if is_param and '*' in decl:
      return c_p
    if not is_param and ''.join(words) == 'char*':
      return ctypes.c_char_p
    if 1 <= len(words) <= 1 + is_param and words[0] in _SCALARS:
      return _SCALARS[words[0]]
  raise ValueError(f'include/se3ds_hip.h: {name}: no ctypes rule for `{decl}`')


def parse_header(text):
  """(signatures, constants) of a header in the style of include/se3ds_hip.h: name -> (restype,
  argtypes) for every `<ret> se3ds_<name>(<params>);` and SE3DS_<NAME> -> int for every integer
  #define.  A pointer parameter is c_void_p, a scalar its ctypes twin, `const char*` returns
  c_char_p; anything the rules do not cover is a ValueError, never a skipped line."""
  text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
  abi = {}
  for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SE3DS_\w+)[ \t]+(\S.*?)[ \t]*$', text, re.M):
    m = _INT.fullmatch(value)
    if not m:
      raise ValueError(f'include/se3ds_hip.h: #define {name}: `{value}` is not an integer literal')
    abi[name] = int(m.group(1), 0)
  text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', ' ', text, flags=re.M)
  sigs = {}
  for stmt in text.split(';'):
    named = re.search(r'\bse3ds_\w+(?=\s*\()', stmt)
    if not named:
      continue
    name, m = named.group(0), _DECL.fullmatch(' '.join(stmt.split()))
    if not m or m.group(2) != name:
      raise ValueError(f'include/se3ds_hip.h: {name}: not a plain `<ret> {name}(<params>);` declaration')
    params = m.group(3).strip()
    args = [] if params == 'void' else [_ctype(p.strip(), name, True) for p in params.split(',')]
    sigs[name] = (_ctype(m.group(1).strip(), name, False), args)
  return sigs, abi


with open(HEADER_PATH) as _f:
  _SIGS, ABI = parse_header(_f.read())   # name -> (restype, argtypes); SE3DS_<NAME> -> int

F32, I32, U8, BF16 = ABI['SE3DS_F32'], ABI['SE3DS_I32'], ABI['SE3DS_U8'], ABI['SE3DS_BF16']
_DTYPE_CODE = {torch.float32: F32, torch.int32: I32, torch.uint8: U8, torch.bfloat16: BF16}
_ERROR_NAMES = {v: k for k, v in ABI.items() if k.startswith('SE3DS_E_')}

_lib = None


class Se3dsHipError(RuntimeError):
  pass


def declared_symbols():
  return sorted(_SIGS)


def lib():
  global _lib
  if _lib is None:
    if not os.path.exists(SO_PATH):
      raise Se3dsHipError(
          f'{SO_PATH} not found: build it with `python -m se3ds_amd.csrc.build` '
          '(__graft_entry__.build()).  There is no CPU fallback for the SE3DS hot path.')
    l = ctypes.CDLL(SO_PATH)
    for name, (res, args) in _SIGS.items():
      fn = getattr(l, name)  # AttributeError if the .so lacks a declared symbol
      fn.restype = res
      fn.argtypes = args
    _lib = l
  return _lib


def dtype_code(t):
  try:
    return _DTYPE_CODE[t.dtype]
  except KeyError:
    raise ValueError(f'unsupported dtype {t.dtype}')


def ptr(t):
  return None if t is None else t.data_ptr()


def stream():
  return torch.cuda.current_stream().cuda_stream


def require_cuda(*tensors):
  for t in tensors:
    if t is not None and not t.is_cuda:
      raise Se3dsHipError('SE3DS hot-path ops need tensors on an MI355X (cuda) device; got a '
                          f'{t.device} tensor.  There is no CPU fallback.')


def check(rc, what):
  if rc != 0:
    msg = lib().se3ds_last_error().decode()
    raise Se3dsHipError(f'{what} failed: {_ERROR_NAMES.get(rc, f"SE3DS_E_{rc}")} {msg}')
