"""bench.py on one MI355X at small sizes: a plain line carries the headline alone, `--steps` sets the
timed steps, and `--dump-outputs` writes what the last timed step computed, the same on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench(args, timeout=600):
  env = dict(os.environ, PYTHONPATH=ROOT)
  env.pop('WORLD_SIZE', None)
  env.pop('RANK', None)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, cwd=ROOT,
                     capture_output=True, text=True, timeout=timeout)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])


def test_warp_plain_line_and_repeatable_dump(tmp_path):
  args = ['--gpus', '1', '--workload', 'warp', '--warp-height', '64', '--steps', '4', '--warmup', '1']
  runs = [tmp_path / 'a', tmp_path / 'b']
  out = _bench(args + ['--dump-outputs', str(runs[0])])
  assert all(k in out for k in HEADLINE), out
  assert out['steps'] == 4 and out['warmup'] == 1 and out['ms_per_step'] > 0
  assert 'roofline' not in out and 'cpu_baseline' not in out, out
  _bench(args + ['--dump-outputs', str(runs[1])])
  shapes = {'depth': (1, 64, 128), 'feats': (1, 64, 128, 3), 'mask': (1, 64, 128)}
  for name, shape in shapes.items():
    a, b = (np.load(d / f'{name}.npy') for d in runs)
    assert a.dtype == np.float32 and a.shape == shape, (name, a.dtype, a.shape)
    assert np.isfinite(a).all() and np.array_equal(a, b), name   # seeded inputs, bit-exact warp


def test_gan_step_plain_line_and_dump(tmp_path):
  out = _bench(['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '1', '--image-size', '128',
                '--dump-outputs', str(tmp_path)], timeout=900)
  assert all(k in out for k in HEADLINE), out
  assert out['steps'] == 2 and out['ms_per_step'] > 0 and out['dtype'] == 'bf16'
  for k in ('roofline', 'warp', 'batch_max', 'fp32_step', 'shipped_schedule', 'cpu_baseline'):
    assert k not in out, k
  files = sorted(os.listdir(tmp_path))
  for name in ('gen_gen_gan_loss', 'dis_disc_loss', 'gen_grad_norm', 'generator_theta',
               'discriminator_theta', 'ema_generator_theta'):
    assert name + '.npy' in files, files
  total = 0
  for f in files:
    a = np.load(tmp_path / f)
    assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    total += a.nbytes
  assert total <= 64 << 20, total
  assert np.load(tmp_path / 'generator_theta.npy').size == 1 << 20
