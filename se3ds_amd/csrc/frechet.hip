// The Frechet distance of the Inception evaluator on the device (utils/inception_utils.py
// frechet_distance_device, FeatureMoments.fid(method='device')), all in binary64:
//   * a square GEMM C = alpha * A B + diag * I on v_mfma_f64_16x16x4_f64, LDS staged;
//   * device moments (count, sum, upper-tile Gram) -> mean and the full symmetric covariance;
//   * tr sqrt(A) and sqrt(A) of a symmetric PSD matrix by the coupled Newton-Schulz iteration, queued
//     without a host synchronisation: a device flag freezes the iteration once the trace stops moving;
//   * |mu1 - mu2|^2, tr S1, tr S2.
// Every reduction has a fixed order and no atomics: the same input gives the same bits on every run.
// Compiled with -ffp-contract=off so the reductions and the epilogues round as written.
#include "common.h"

#include <math.h>

namespace se3ds {
namespace {

constexpr int kB = 256;

// ------------------------------------------------------------------------------ GEMM
// One 256-thread workgroup (2 x 2 waves) per 128 x 128 tile of C; a wave owns 64 x 64 = 4 x 4 MFMA
// tiles.  K advances 16 at a time: the next A (128 x 16) and B (16 x 128) tiles are loaded into
// registers while the MFMAs of the current ones run from LDS.  Rows and columns >= n load as zero and
// are not stored.
// v_mfma_f64_16x16x4_f64 operands: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; its
// four results are D[(l >> 4) + 4 r][l & 15], r = 0..3 (NOT the f32 map, which is 4 (l >> 4) + r).
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kGT = 128, kGK = 16;
constexpr int kAS = kGK + 1;    // As[m][k]: a fragment read walks m, the odd stride spreads the banks
constexpr int kBS = kGT + 16;   // Bs[k][n]: the four k rows of a fragment read start 16 doubles apart
constexpr int kGE = kGT * kGK / kB;   // elements of each operand tile per thread

__global__ void __launch_bounds__(kB)
f64_gemm_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                int n, double alpha, double diag, const int* __restrict__ done) {
  if (done != nullptr && *done != 0) return;
  __shared__ double As[kGT * kAS];
  __shared__ double Bs[kGK * kBS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lk = lane >> 4;
  const int row0 = blockIdx.y * kGT, col0 = blockIdx.x * kGT;
  f64x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double ra[kGE], rb[kGE];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < kGE; ++i) {
      const int e = t + kB * i;
      const int ar = row0 + (e >> 4), ak = k0 + (e & 15);
      ra[i] = (ar < n && ak < n) ? A[(int64_t)ar * n + ak] : 0.0;
      const int bk = k0 + (e >> 7), bc = col0 + (e & 127);
      rb[i] = (bk < n && bc < n) ? B[(int64_t)bk * n + bc] : 0.0;
    }
  };
  gload(0);
  for (int k0 = 0; k0 < n; k0 += kGK) {
    __syncthreads();   // the previous tile's fragment reads are done
#pragma unroll
    for (int i = 0; i < kGE; ++i) {
      const int e = t + kB * i;
      As[(e >> 4) * kAS + (e & 15)] = ra[i];
      Bs[(e >> 7) * kBS + (e & 127)] = rb[i];
    }
    __syncthreads();
    if (k0 + kGK < n) gload(k0 + kGK);
#pragma unroll
    for (int kk = 0; kk < kGK / 4; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[(wm * 64 + i * 16 + lr) * kAS + kk * 4 + lk];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs[(kk * 4 + lk) * kBS + wn * 64 + j * 16 + lr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + wm * 64 + i * 16 + lk + 4 * r;
      if (row >= n) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = col0 + wn * 64 + j * 16 + lr;
        if (col >= n) continue;
        double v = alpha * acc[i][j][r];
        if (row == col) v += diag;
        C[(int64_t)row * n + col] = v;
      }
    }
}

// ------------------------------------------------------------------------------ reductions
// Sum of the workgroup's 256 values in a fixed tree; every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// sum_i x[i * stride], i < count: thread t adds i = t, t + 256, ... in order, then the tree
__device__ __forceinline__ double block_strided_sum(const double* x, int64_t count, int64_t stride,
                                                    double* sh) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += kB) s += x[i * stride];
  return block_sum(s, sh);
}

// ------------------------------------------------------------------------------ moments -> statistics
// mean[j] = sum[j] / n, cov[i][j] = (gram[min(i,j)][max(i,j)] - sum[i] sum[j] / n) / (n - 1): the
// arithmetic of FeatureMoments.mean_cov().  moments_kernel (inception.hip) writes only the 64 x 64
// tiles with i-tile <= j-tile, so a 32 x 32 output tile below the diagonal reads its mirror tile
// through LDS and the whole matrix comes out exactly symmetric.
constexpr int kCT = 32;

__global__ void __launch_bounds__(kB)
mean_cov_kernel(const int64_t* __restrict__ count, const double* __restrict__ sum,
                const double* __restrict__ gram, int c, double* __restrict__ mean,
                double* __restrict__ cov) {
  __shared__ double s[kCT][kCT + 1];
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int si = ti < tj ? ti : tj, sj = ti < tj ? tj : ti;   // the source tile, si <= sj
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double n = (double)*count;
#pragma unroll
  for (int e = 0; e < kCT / 8; ++e) {
    const int li = ty + 8 * e;
    const int gi = si * kCT + li, gj = sj * kCT + tx;
    s[li][tx] = (gi < c && gj < c) ? gram[(int64_t)gi * c + gj] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kCT / 8; ++e) {
    const int li = ty + 8 * e, lj = tx;
    const int i = ti * kCT + li, j = tj * kCT + lj;
    if (i >= c || j >= c) continue;
    double g;
    if (ti < tj) g = s[li][lj];
    else if (ti > tj) g = s[lj][li];
    else g = li < lj ? s[li][lj] : s[lj][li];
    cov[(int64_t)i * c + j] = (g - sum[i] * sum[j] / n) / (n - 1.0);
    if (ti == 0 && li == 0) mean[j] = sum[j] / n;
  }
}

// ------------------------------------------------------------------------------ root and trace
// Coupled Newton-Schulz: c = ||A||_F, Y0 = A / c, Z0 = I; T = 1.5 I - 0.5 Z Y, Y <- Y T, Z <- T Z;
// Y -> sqrt(A / c).  The iteration stops when |tr Y_k - tr Y_{k-1}| <= tol |tr Y_k| (in the null
// space of a singular A, Z grows 1.5 x per iteration: without the stop it overflows).
struct SqrtState {
  double prev;   // tr Y of the newest iterate
  double c;      // ||A||_F
  int done;      // nonzero: the iterate is frozen, every later kernel returns at once
  int iters;     // iterations taken
  int status;    // SE3DS_SQRT_*
  int cur;       // which of the two Y buffers holds the newest iterate
};
constexpr int kNormBlocks = 256;
constexpr size_t kStateBytes = 4096;   // SqrtState, then kNormBlocks partial sums at byte 256

__global__ void __launch_bounds__(kB)
sumsq_partial_kernel(const double* __restrict__ a, int64_t n2, double* __restrict__ partials) {
  __shared__ double sh[kB];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kB)
    s += a[i] * a[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kB)
sqrt_init_kernel(const double* __restrict__ a, int n, const double* __restrict__ partials,
                 int nparts, SqrtState* __restrict__ st) {
  __shared__ double sh[kB];
  const double ss = block_sum((int)threadIdx.x < nparts ? partials[threadIdx.x] : 0.0, sh);
  const double tr = block_strided_sum(a, n, (int64_t)n + 1, sh);
  if (threadIdx.x == 0) {
    const double c = sqrt(ss);
    st->c = c;
    st->iters = 0;
    st->cur = 0;
    if (!isfinite(c) || !isfinite(tr)) {
      st->prev = tr;
      st->done = 1;
      st->status = SE3DS_SQRT_NONFINITE;
    } else if (c == 0.0) {   // A = 0: the root is 0
      st->prev = 0.0;
      st->done = 1;
      st->status = SE3DS_SQRT_CONVERGED;
    } else {
      st->prev = tr / c;
      st->done = 0;
      st->status = SE3DS_SQRT_CAP_REACHED;
    }
  }
}

__global__ void __launch_bounds__(kB)
sqrt_start_kernel(const double* __restrict__ a, int n, const SqrtState* __restrict__ st,
                  double* __restrict__ y, double* __restrict__ z) {
  const double c = st->c;
  const bool ok = isfinite(c) && c > 0.0;
  const int64_t n2 = (int64_t)n * n;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kB) {
    y[i] = ok ? a[i] / c : 0.0;
    z[i] = (i / n == i % n) ? 1.0 : 0.0;
  }
}

// After iteration k wrote its Y into y_new: the trace, the stop rule, the flag.
__global__ void __launch_bounds__(kB)
sqrt_trace_step_kernel(const double* __restrict__ y_new, int n, int k, int buf, double tol,
                       SqrtState* __restrict__ st) {
  if (st->done != 0) return;
  __shared__ double sh[kB];
  const double tr = block_strided_sum(y_new, n, (int64_t)n + 1, sh);
  if (threadIdx.x == 0) {
    const double prev = st->prev;
    st->prev = tr;
    st->iters = k;
    st->cur = buf;
    if (!isfinite(tr)) {
      st->done = 1;
      st->status = SE3DS_SQRT_NONFINITE;
    } else if (fabs(tr - prev) <= tol * fabs(tr)) {
      st->done = 1;
      st->status = SE3DS_SQRT_CONVERGED;
    }
  }
}

// result = (sqrt(c) tr Y, iterations, status, c); root = sqrt(c) Y (NULL: not wanted)
__global__ void __launch_bounds__(kB)
sqrt_finish_kernel(const SqrtState* __restrict__ st, const double* __restrict__ y0,
                   const double* __restrict__ y1, int n, double* __restrict__ root,
                   double* __restrict__ result) {
  const double c = st->c;
  const double sc = sqrt(c);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    result[0] = sc * st->prev;
    result[1] = (double)st->iters;
    result[2] = (double)st->status;
    result[3] = c;
  }
  if (root == nullptr) return;
  const double* y = st->cur ? y1 : y0;
  const int64_t n2 = (int64_t)n * n;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kB)
    root[i] = sc * y[i];
}

// out = (|mu1 - mu2|^2, tr S1, tr S2)
__global__ void __launch_bounds__(kB)
frechet_terms_kernel(const double* __restrict__ mu1, const double* __restrict__ mu2,
                     const double* __restrict__ s1, const double* __restrict__ s2, int n,
                     double* __restrict__ out) {
  __shared__ double sh[kB];
  double d = 0.0;
  for (int i = threadIdx.x; i < n; i += kB) {
    const double v = mu1[i] - mu2[i];
    d += v * v;
  }
  d = block_sum(d, sh);
  const double t1 = block_strided_sum(s1, n, (int64_t)n + 1, sh);
  const double t2 = block_strided_sum(s2, n, (int64_t)n + 1, sh);
  if (threadIdx.x == 0) {
    out[0] = d;
    out[1] = t1;
    out[2] = t2;
  }
}

constexpr int kMaxN = 16384;

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

inline void launch_gemm(const double* a, const double* b, double* c, int n, double alpha,
                        double diag, const int* done, hipStream_t s) {
  const unsigned g = (unsigned)ceil_div(n, kGT);
  hipLaunchKernelGGL(f64_gemm_kernel, dim3(g, g), dim3(kB), 0, s, a, b, c, n, alpha, diag, done);
}

}  // namespace
}  // namespace se3ds

using namespace se3ds;

extern "C" {

int se3ds_f64_gemm(const double* a, const double* b, double* c, int n, double alpha, double diag,
                   void* stream) {
  if (n < 1 || n > kMaxN || a == nullptr || b == nullptr || c == nullptr || misaligned(a) ||
      misaligned(b) || misaligned(c) || c == a || c == b)
    return SE3DS_E_BADSHAPE;
  launch_gemm(a, b, c, n, alpha, diag, nullptr, as_stream(stream));
  return check_launch("f64_gemm");
}

int se3ds_moments_mean_cov(const int64_t* count, const double* sum, const double* gram, int dim,
                           double* mean, double* cov, void* stream) {
  if (dim < 1 || dim > kMaxN || count == nullptr || sum == nullptr || gram == nullptr ||
      mean == nullptr || cov == nullptr || misaligned(count) || misaligned(sum) ||
      misaligned(gram) || misaligned(mean) || misaligned(cov) || cov == gram)
    return SE3DS_E_BADSHAPE;
  const unsigned g = (unsigned)ceil_div(dim, kCT);
  hipLaunchKernelGGL(mean_cov_kernel, dim3(g, g), dim3(kB), 0, as_stream(stream), count, sum, gram,
                     dim, mean, cov);
  return check_launch("moments_mean_cov");
}

size_t se3ds_sqrt_trace_workspace_bytes(int n) {
  if (n < 1 || n > kMaxN) return 0;
  return kStateBytes + (size_t)5 * n * n * sizeof(double);
}

int se3ds_sqrt_trace(const double* a, int n, int max_iters, double tol, double* root,
                     void* workspace, size_t workspace_bytes, double* result, void* stream) {
  if (n < 1 || n > kMaxN || max_iters < 0 || max_iters > 1024 || !(tol >= 0.0) || a == nullptr ||
      workspace == nullptr || result == nullptr || misaligned(a) || misaligned(root) ||
      misaligned(workspace) || misaligned(result) || root == a)
    return SE3DS_E_BADSHAPE;
  if (workspace_bytes < se3ds_sqrt_trace_workspace_bytes(n)) return SE3DS_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(workspace);
  SqrtState* st = reinterpret_cast<SqrtState*>(base);
  double* partials = reinterpret_cast<double*>(base + 256);
  const int64_t n2 = (int64_t)n * n;
  double* m = reinterpret_cast<double*>(base + kStateBytes);
  double* y[2] = {m, m + n2};
  double* z[2] = {m + 2 * n2, m + 3 * n2};
  double* t = m + 4 * n2;
  const int nparts = (int)(ceil_div(n2, kB) < kNormBlocks ? ceil_div(n2, kB) : kNormBlocks);
  const dim3 ge((unsigned)grid_for(n2, kB));
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nparts), dim3(kB), 0, s, a, n2, partials);
  hipLaunchKernelGGL(sqrt_init_kernel, dim3(1), dim3(kB), 0, s, a, n, partials, nparts, st);
  hipLaunchKernelGGL(sqrt_start_kernel, ge, dim3(kB), 0, s, a, n, st, y[0], z[0]);
  for (int k = 1; k <= max_iters; ++k) {
    const int cur = (k - 1) & 1, nxt = k & 1;
    launch_gemm(z[cur], y[cur], t, n, -0.5, 1.5, &st->done, s);
    launch_gemm(y[cur], t, y[nxt], n, 1.0, 0.0, &st->done, s);
    launch_gemm(t, z[cur], z[nxt], n, 1.0, 0.0, &st->done, s);
    hipLaunchKernelGGL(sqrt_trace_step_kernel, dim3(1), dim3(kB), 0, s, y[nxt], n, k, nxt, tol, st);
  }
  hipLaunchKernelGGL(sqrt_finish_kernel, root != nullptr ? ge : dim3(1), dim3(kB), 0, s, st, y[0],
                     y[1], n, root, result);
  return check_launch("sqrt_trace");
}

int se3ds_frechet_terms(const double* mu1, const double* mu2, const double* sigma1,
                        const double* sigma2, int n, double* out, void* stream) {
  if (n < 1 || n > kMaxN || mu1 == nullptr || mu2 == nullptr || sigma1 == nullptr ||
      sigma2 == nullptr || out == nullptr || misaligned(mu1) || misaligned(mu2) ||
      misaligned(sigma1) || misaligned(sigma2) || misaligned(out))
    return SE3DS_E_BADSHAPE;
  hipLaunchKernelGGL(frechet_terms_kernel, dim3(1), dim3(kB), 0, as_stream(stream), mu1, mu2, sigma1,
                     sigma2, n, out);
  return check_launch("frechet_terms");
}

}  // extern "C"
