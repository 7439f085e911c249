"""Throughput of the Inception-v3 evaluator on the device: images/s and TFLOP/s of
get_inception (gather + network) at batch 64 in fp32 and bf16 from 384 x 1024 frames, and the
time of one se3ds_feature_moments_accumulate over a (64, 2048) batch.  Random seeded weights.

  python tools/inception_bench.py [--batch 64] [--iters 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from se3ds_amd.utils import inception_utils as iu  # noqa: E402

DEV = torch.device('cuda:0')


def conv_flops():
  """2 * MACs of the 94 convolutions and the Dense layer for one 299 x 299 image."""
  s = iu._Specs()
  shapes = []
  orig = s.conv_bn

  def conv_bn(x, cout, kh, kw, stride=1, padding='same'):
    y = orig(x, cout, kh, kw, stride, padding)
    shapes.append((y[0] * y[1], x[2] * cout * kh * kw))
    return y

  s.conv_bn = conv_bn
  iu._architecture(s, (iu.INPUT_SIZE, iu.INPUT_SIZE, 3))
  return sum(2 * p * k for p, k in shapes) + 2 * iu.POOL_DIM * iu.NUM_CLASSES


def time_ms(fn, iters):
  fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--iters', type=int, default=5)
  a = ap.parse_args()
  flops = conv_flops() * a.batch
  frames = torch.rand((a.batch, 384, 1024, 3), device=DEV)
  crop = frames[:, 48:336].contiguous()
  for dtype in (torch.float32, torch.bfloat16):
    m = iu.inception_model(init='random', seed=0, dtype=dtype, device=DEV)
    ms = time_ms(lambda: iu.get_inception(crop, m), a.iters)
    print(f'get_inception {str(dtype)[6:]:8s} batch {a.batch}: {ms:8.2f} ms  {a.batch / ms * 1e3:8.1f} images/s  '
          f'{flops / ms / 1e9:6.1f} TFLOP/s')
  pools = torch.rand((a.batch, iu.POOL_DIM), device=DEV)
  mom = iu.FeatureMoments(device=DEV)
  ms = time_ms(lambda: mom.update(pools), a.iters)
  print(f'feature_moments_accumulate ({a.batch}, {iu.POOL_DIM}): {ms:.3f} ms')


if __name__ == '__main__':
  main()
