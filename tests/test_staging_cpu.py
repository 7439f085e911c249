"""utils/_staging.py on the host: the 16-byte layout rule against the loop the record writer's flush
used to spell out, and the device check's message."""
import pytest

from se3ds_amd import _lib
from se3ds_amd.utils import _staging

SIZE_LISTS = ([0], [1], [16], [17, 0, 15, 16, 1], [])


def _flush_loop(sizes, at=0):
  """The loop of R2RRecordWriter.flush before the layout had a home."""
  offsets = []
  for size in sizes:
    offsets.append(at)
    at = (at + size + 15) & ~15
  return offsets, at


@pytest.mark.parametrize('n,want', [(0, 0), (1, 16), (15, 16), (16, 16), (17, 32), (2**31 + 1, 2**31 + 16)])
def test_aligned(n, want):
  assert _staging.aligned(n) == want


@pytest.mark.parametrize('start', [0, 16, 5, 4096 + 1])
@pytest.mark.parametrize('sizes', SIZE_LISTS)
def test_layout_is_aligned_ordered_and_disjoint(sizes, start):
  offsets, total = _staging.layout(sizes, start)
  assert len(offsets) == len(sizes) and total % 16 == 0 and total >= start
  end = start
  for at, size in zip(offsets, sizes):
    assert at % 16 == 0 and at >= end   # behind `start` and behind every part before it
    assert at - end < 16                # at the NEXT boundary
    end = at + size
  assert end <= total < end + 16


@pytest.mark.parametrize('sizes', SIZE_LISTS)
def test_layout_equals_the_flush_loop(sizes):
  assert _staging.layout(sizes) == _flush_loop(sizes)
  assert _staging.layout(sizes, 48) == _flush_loop(sizes, 48)


def test_layout_of_the_mixed_list_in_numbers():
  assert _staging.layout([17, 0, 15, 16, 1]) == ([0, 32, 32, 48, 64], 80)   # the empty part: no advance
  assert _staging.layout([17, 0, 15, 16, 1], 3) == ([16, 48, 48, 64, 80], 96)
  assert _staging.layout([]) == ([], 0)


def test_cuda_device_refuses_the_cpu():
  with pytest.raises(_lib.Se3dsHipError) as e:
    _staging.cuda_device('cpu', 'x')
  for part in ('x computes on an MI355X (cuda) device; got cpu', 'There is no CPU fallback'):
    assert part in str(e.value)
  with pytest.raises(_lib.Se3dsHipError, match='x encodes on'):
    _staging.cuda_device('cpu', 'x', 'encodes')


def test_cuda_device_keeps_a_given_index():
  dev = _staging.cuda_device('cuda:3', 'x')   # no device is touched
  assert (dev.type, dev.index) == ('cuda', 3)
