// Device helpers shared by the batched FITC kernels, one workgroup of 256 threads per problem:
// kernels_batch_fitc.hip (every array in LDS, n <= 128), kernels_batch_fitc_tall.hip
// (the n-sized arrays in a device workspace, n <= 2048) and, through
// batch_fitc_tall_shared.h, kernels_batch_fitc_tall_block.hip (the block-LOO objectives, DESIGN
// §27).  Included once per kernel file; everything sits in that file's anonymous namespace.
#pragma once
#include "batch_driver.h"
#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

constexpr int FT = 256;                    // threads per workgroup
constexpr int FG = 2 + GPS_BATCH_MAX_D;    // gradient sums: ΣG∘K, ΣM_ii, per-dimension
constexpr int kThDoubles = 40;             // θ (<= 18) then 1/ℓ_k (<= 16) at th + 20
constexpr double kJitter = 1e-3;           // K20:36, inside K̃mm everywhere

__host__ __device__ constexpr int odd_ld(int m) { return m | 1; }  // conflict-free row strides

// lanes per column group: 256 / (m rounded up to a power of two), at most one wave
__device__ __forceinline__ int group_lanes(int cols) {
  int p = 1;
  while (p < cols) p <<= 1;
  const int c = FT / p;
  return c > 64 ? 64 : (c < 1 ? 1 : c);
}

// sum over the C adjacent lanes of a group (C a power of two <= 64): a fixed butterfly; every
// lane of the wave takes part
__device__ __forceinline__ double group_sum(double x, int C) {
  for (int o = C >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// block_sum of the first nv <= NV values per thread (the rest are left alone)
template <int NV>
__device__ __forceinline__ void block_sum_n(double (&v)[NV], int nv, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (q < nv) v[q] = wave_sum(v[q]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < NV; ++q)
      if (q < nv) sh[q * 16 + wave] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (q < nv) {
      double t = 0.0;
      for (int w = 0; w < FT / 64; ++w) t += sh[q * 16 + w];
      v[q] = t;
    }
  __syncthreads();
}

// W (m×m, lower triangle read) → L⁻¹ in its lower triangle, the strict upper triangle zeroed,
// piv[k] = L_kk.  One sweep over the pivots as kernels_batch.hip forward(): step k scales row k of
// X = L⁻¹, forms column k of L and applies the rank-one update to the rows below (the trailing
// Cholesky update right of column k, the forward substitution of the identity left of it).
// Returns 0, or the 1-based order of the leading minor whose pivot is not > 0 (NaN included) —
// the same value in every thread.  Call synchronised; ends synchronised.
__device__ __forceinline__ int chol_inv(double* W, int m, int ld, double* piv, double* wv,
                                        double* lc) {
  const int t = threadIdx.x;
  for (int k = 0; k < m; ++k) {
    const double dk = W[k * ld + k];
    if (!(dk > 0.0)) return k + 1;
    const double is = 1.0 / sqrt(dk);
    if (t < m) {
      if (t < k) {
        const double x = W[k * ld + t] * is;
        wv[t] = x;
        W[k * ld + t] = x;
      } else if (t == k) {
        wv[t] = is;
        piv[k] = dk * is;
      } else {
        const double l = W[t * ld + k] * is;
        wv[t] = l;
        lc[t] = l;
        W[t * ld + k] = 0.0;  // the update below then writes X_tk = 0 − L_tk/L_kk like any entry
      }
    }
    __syncthreads();
    if (t == 0) W[k * ld + k] = is;  // row k is not touched below, the next pivot is W[k+1][k+1]
    for (int e = t; e < m * m; e += FT) {
      const int i = e / m, j = e - i * m;
      if (i > k && j <= i) W[i * ld + j] = fma(-lc[i], wv[j], W[i * ld + j]);
    }
    __syncthreads();
  }
  for (int e = t; e < m * m; e += FT) {
    const int i = e / m, j = e - i * m;
    if (j > i) W[i * ld + j] = 0.0;
  }
  __syncthreads();
  return 0;
}

// BATCH_MODE_GRAD's end for the FITC pair: NaN for a failed problem, and info
__device__ __forceinline__ void fitc_grad_end(const BatchFitcParams p, int64_t pb, int t,
                                              int info) {
  const int m = p.m, d = p.d, nth = 2 + p.n_ell;
  if (info) {
    if (t < GPS_N_OBJ) p.obj[pb * GPS_N_OBJ + t] = batch_nan();
    if (t < nth) p.grad[pb * nth + t] = batch_nan();
    for (int e = t; e < m * d; e += FT) p.grad_z[pb * m * d + e] = batch_nan();
  }
  if (t == 0) p.info[pb] = info;
}

}  // namespace

}  // namespace gps
