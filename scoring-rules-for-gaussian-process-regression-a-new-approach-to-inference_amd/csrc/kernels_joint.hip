// Kernels of the joint test predictive (api_joint.hip): the covariance finisher, which turns the
// split-K slabs of S = VᵀV into the predictive covariance of a block of test rows
// (cal_mean_and_cov KF:121-126 / spgp_cal_mean_and_cov K20:76-83, all of it, not its diagonal),
// and the small vector kernels of its consumers (dss KF:103-108, the draws' mean).
// Fixed-order sums, no atomics: results are bitwise reproducible run to run.
#include "gps_internal.h"

namespace gps {

// ------------------------------------------------------------ covariance finisher
// One workgroup per lower 32-tile (r >= c) of the padded bp×bp block:
//   Sigma_ij = sf2·exp(−½‖(x_i − x_j)/ℓ‖²) + sn2·δ_ij − Σ_q slab_q[i][j]      (i, j < b)
//            = δ_ij                                                            (padding)
// K** is evaluated from the two tiles' features (staged in LDS, already divided by ℓ) and never
// stored; the slices are summed in slice order; the tile and — through a 33-column LDS image — its
// transpose are written in the same pass, so Sigma is symmetric bitwise and needs no mirror or
// padding launch.  A diagonal tile takes its upper half from its lower half the same way (the
// GEMM's diagonal tiles are whole but need not be symmetric to the last bit).  HBM-bound:
// ks·bp²/2 doubles read, bp² written, every global access a 16-byte one (two columns per thread,
// 16 threads per 256-byte tile row).
constexpr int JT = 32;

__global__ __launch_bounds__(256) void joint_cov_kernel(JointCovParams p) {
  extern __shared__ __attribute__((aligned(16))) double jsm[];
  double2* tab = reinterpret_cast<double2*>(jsm);  // exp table (exp_tab_stage): 64 pairs
  double* t = jsm + 128;                           // [32][33]
  const int dd = p.d | 1;                          // odd feature stride: the column reads of one
  double* xr = t + JT * (JT + 1);                  // half-wave fall on distinct banks
  double* xc = xr + JT * dd;
  const int blk = blockIdx.x;
  int r = (int)((sqrt(8.0 * (double)blk + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= blk) ++r;
  while (r * (r + 1) / 2 > blk) --r;
  const int c = blk - r * (r + 1) / 2;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  exp_tab_stage(tab);
  for (int e = tid; e < JT * p.d; e += 256) {
    const int i = e / p.d, k = e - i * p.d;
    const int gr = r * JT + i, gc = c * JT + i;
    xr[i * dd + k] = gr < p.b ? p.x[(int64_t)gr * p.d + k] * p.inv_ell[k] : 0.0;
    xc[i * dd + k] = gc < p.b ? p.x[(int64_t)gc * p.d + k] * p.inv_ell[k] : 0.0;
  }
  __syncthreads();
  double2 v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int li = ty + 16 * h, lj = 2 * tx;
    const int gi = r * JT + li, gj = c * JT + lj;
    const int64_t e = (int64_t)gi * p.bp + gj;
    double2 sum = *reinterpret_cast<const double2*>(p.slab + e);
    for (int q = 1; q < p.ks; ++q) {
      const double2 w = *reinterpret_cast<const double2*>(p.slab + q * p.stride + e);
      sum.x += w.x;
      sum.y += w.y;
    }
    double d0 = 0.0, d1 = 0.0;
    const double* a = xr + li * dd;
    const double* b0 = xc + lj * dd;
    const double* b1 = b0 + dd;
    for (int k = 0; k < p.d; ++k) {
      const double u0 = a[k] - b0[k], u1 = a[k] - b1[k];
      d0 = fma(u0, u0, d0);
      d1 = fma(u1, u1, d1);
    }
    double k0 = p.sf2 * exp_neg(-0.5 * d0, tab), k1 = p.sf2 * exp_neg(-0.5 * d1, tab);
    if (gi == gj) k0 += p.sn2;
    if (gi == gj + 1) k1 += p.sn2;
    k0 -= sum.x;
    k1 -= sum.y;
    if (gi >= p.b || gj >= p.b) k0 = gi == gj ? 1.0 : 0.0;
    if (gi >= p.b || gj + 1 >= p.b) k1 = gi == gj + 1 ? 1.0 : 0.0;
    v[h] = make_double2(k0, k1);
    t[li * (JT + 1) + lj] = k0;
    t[li * (JT + 1) + lj + 1] = k1;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int li = ty + 16 * h, lj = 2 * tx;
    const double2 m = make_double2(t[lj * (JT + 1) + li], t[(lj + 1) * (JT + 1) + li]);
    if (r == c) {  // the upper half of a diagonal tile is its lower half's image
      double2 o = v[h];
      if (lj > li) o.x = m.x;
      if (lj + 1 > li) o.y = m.y;
      *reinterpret_cast<double2*>(p.out + (int64_t)(r * JT + li) * p.bp + c * JT + lj) = o;
    } else {
      *reinterpret_cast<double2*>(p.out + (int64_t)(r * JT + li) * p.bp + c * JT + lj) = v[h];
      *reinterpret_cast<double2*>(p.out + (int64_t)(c * JT + li) * p.bp + r * JT + lj) = m;
    }
  }
}

hipError_t launch_joint_cov(const JointCovParams& p, hipStream_t s) {
  if (p.b < 1 || p.bp < p.b || p.bp % GPS_TILE || p.d < 1 || p.d > GPS_MAX_D || p.ks < 1)
    return hipErrorInvalidValue;
  const int64_t t32 = p.bp / JT;
  const size_t lds = (size_t)(128 + JT * (JT + 1) + 2 * JT * (p.d | 1)) * sizeof(double);
  hipLaunchKernelGGL(joint_cov_kernel, dim3((unsigned)(t32 * (t32 + 1) / 2)), dim3(256), lds, s, p);
  return hipGetLastError();
}

// ------------------------------------------------------------------ small
__global__ __launch_bounds__(256) void joint_resid_kernel(const double* __restrict__ y,
                                                          const double* __restrict__ mu, int b,
                                                          int bp, double* __restrict__ r) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < bp) r[i] = i < b ? y[i] - mu[i] : 0.0;
}
hipError_t launch_joint_resid(const double* y, const double* mu, int b, int bp, double* r,
                              hipStream_t s) {
  hipLaunchKernelGGL(joint_resid_kernel, dim3((bp + 255) / 256), dim3(256), 0, s, y, mu, b, bp, r);
  return hipGetLastError();
}

__global__ __launch_bounds__(1024) void joint_dss_kernel(const double* __restrict__ logdiag,
                                                         const double* __restrict__ t, int b,
                                                         double* __restrict__ out) {
  __shared__ double sh[2 * 16];
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < b; i += blockDim.x) {
    v[0] += logdiag[i];
    v[1] = fma(t[i], t[i], v[1]);
  }
  block_sum<2>(v, sh);
  if (threadIdx.x == 0) out[0] = 0.5 * b * 1.83787706640934548356 + v[0] + 0.5 * v[1];
}
hipError_t launch_joint_dss(const double* logdiag, const double* t, int b, double* out,
                            hipStream_t s) {
  hipLaunchKernelGGL(joint_dss_kernel, dim3(1), dim3(1024), 0, s, logdiag, t, b, out);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void sign_fill_kernel(double* __restrict__ dst, int npos, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = i < npos ? 1.0 : -1.0;
}
hipError_t launch_sign_fill(double* dst, int npos, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sign_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, npos, n);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void row_add_kernel(double* __restrict__ M, int64_t ld,
                                                      const double* __restrict__ mu, int rows,
                                                      int cols) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)rows * cols) return;
  const int i = (int)(e / cols), j = (int)(e - (int64_t)i * cols);
  M[(int64_t)i * ld + j] += mu[j];
}
hipError_t launch_row_add(double* M, int64_t ld, const double* mu, int rows, int cols,
                          hipStream_t s) {
  const int64_t tot = (int64_t)rows * cols;
  if (tot <= 0) return hipSuccess;
  hipLaunchKernelGGL(row_add_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, M, ld, mu,
                     rows, cols);
  return hipGetLastError();
}

}  // namespace gps
