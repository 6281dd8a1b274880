// The step driver the "one workgroup per problem" batch kernels share (kernels_batch.hip,
// kernels_batch_fitc.hip, kernels_batch_fitc_tall.hip, and through batch_full_tall_shared.h
// kernels_batch_full_tall.hip and kernels_batch_full_tall_block.hip):
// what a __global__ function there does around its own forward(), gradient() and test-row loop.
// The helpers take the params struct P (BatchParams or BatchFitcParams) BY VALUE, the thread
// index and raw pointers (th: θ in LDS, il = th + 20: 1/ℓ_k), the block size NT as a template
// constant, and know nothing of a kernel's Lds struct.  All are force-inlined, and a kernel uses
// one only where it compiles to the instructions it had with the text in place (the recipe and
// the list of what therefore stayed in the kernels are in DESIGN §25): pass p by value, t from the
// caller, and derive nth, d and m from p inside.  Included once per kernel file; everything sits
// in that file's anonymous namespace.  The FITC pair's own GRAD-mode end is in batch_fitc_shared.h.
// fold_begin is the fold geometry of the three block-LOO kernel files.
#pragma once
#include <type_traits>

#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

__device__ __forceinline__ double batch_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// fold f's first row: the block-LOO paths' folds are [⌊f·n/k⌋, ⌊(f+1)·n/k⌋) (KF:496-499)
__device__ __forceinline__ int fold_begin(int f, int n, int nfold) {
  return (int)((int64_t)f * n / nfold);
}

// A step's prologue, between two barriers: θ → sf², σ² and 1/ℓ_k into il (GPS_ARD: exp(−b_k);
// GPS_RBF: exp(−b/2); the FITC kernels pass GPS_ARD).  The final pass (fin) with stale_noise takes
// the σ² of the last training step's forward, which every other pass records in `stale`.
template <class P>
__device__ __forceinline__ void step_prologue(const P p, int t, const double* th, double* il,
                                              int kind, bool fin, double& stale, double& sf2,
                                              double& sn2) {
  const int d = p.d, nth = 2 + p.n_ell;
  __syncthreads();  // θ (and Z: loaded, or the previous step's update) is visible
  const double lsn = th[nth - 1];
  sf2 = exp(th[0]);
  sn2 = exp(fin && p.stale_noise ? stale : lsn);
  const double bq = t < d ? th[1 + (p.n_ell == 1 ? 0 : t)] : 0.0;
  if (t < d) il[t] = kind == GPS_ARD ? exp(-bq) : exp(-0.5 * bq);  // th + 20: never over θ
  __syncthreads();
  if (!fin) stale = lsn;
}

// BATCH_MODE_GRAD's end for the full-GP pair: info, and NaN for a failed problem
__device__ __forceinline__ void full_grad_end(const BatchParams p, int64_t pb, int t, int info) {
  const int nth = 2 + p.n_ell;
  if (t == 0) {
    p.info[pb] = info;
    if (info) {
      for (int q = 0; q < GPS_N_OBJ; ++q) p.obj[pb * GPS_N_OBJ + q] = batch_nan();
      for (int q = 0; q < nth; ++q) p.grad[pb * nth + q] = batch_nan();
    }
  }
}

// BATCH_MODE_TRAIN's end, after the step loop's closing barrier.  A failed problem (in this launch
// or an earlier one) gets NaN in the rest of its series; θ (and Z from zs, FITC only), the stale
// σ² and steps_done go back to device memory for the next launch of the call.  The kernel stores
// info itself, next to its do_final test.
template <int NT, class P>
__device__ __forceinline__ void train_write_back(const P p, int64_t pb, int t, const double* th,
                                                 const double* zs, int info, int done,
                                                 double stale) {
  const int nth = 2 + p.n_ell;
  if (info) {
    const int s0 = done > p.step0 ? done : p.step0;
    const int s1 = p.step0 + p.nsteps;
    for (int e = s0 + t; e < s1; e += NT) p.values[pb * p.itr + e] = batch_nan();
    for (int64_t e = (int64_t)s0 * nth + t; e < (int64_t)s1 * nth; e += NT)
      p.thetas[pb * p.itr * nth + e] = batch_nan();
  }
  if (t < nth) p.theta[pb * nth + t] = th[t];
  if constexpr (std::is_same<P, BatchFitcParams>::value) {
    const int m = p.m, d = p.d;
    for (int e = t; e < m * d; e += NT) p.z[pb * m * d + e] = zs[e];
  }
  if (t == 0) {
    p.stale[pb] = stale;
    p.steps_done[pb] = done;
  }
}

// The last launch's outputs before the test rows: the final objectives, or NaN for them, μ / var
// and the scores of a failed problem.  Returns whether the test predictive is still to be formed
// (no failure, test rows given).
template <int NT, class P>
__device__ __forceinline__ bool final_outputs(const P p, int64_t pb, int t, int info, bool pred,
                                              const double (&obj)[GPS_N_OBJ]) {
  if (info) {
    if (t < GPS_N_OBJ) p.obj[pb * GPS_N_OBJ + t] = batch_nan();
    if (pred) {
      for (int e = t; e < p.nt; e += NT) {
        p.mu[pb * p.nt + e] = batch_nan();
        p.var[pb * p.nt + e] = batch_nan();
      }
      if (p.yt && t < GPS_N_SC) p.sc[pb * GPS_N_SC + t] = batch_nan();
    }
    return false;
  }
  if (t == 0)
    for (int q = 0; q < GPS_N_OBJ; ++q) p.obj[pb * GPS_N_OBJ + q] = obj[q];
  return pred;
}

// one test row's six score terms added to sums, as score_rows_kernel forms them: CRPS, LogS, LogS
// minus the trivial model's, squared error, the trivial model's, 2σ coverage
__device__ __forceinline__ void score_row_add(double (&sums)[6], double mu, double c, double yv,
                                              double ymean, double yvar, double triv_c) {
  sums[0] += crps_term(mu, c, yv);
  const double ls = logs_term(mu, c, yv);
  sums[1] += ls;
  const double e0 = yv - ymean;
  sums[2] += ls - (triv_c + e0 * e0 / (2.0 * yvar));
  sums[3] += (mu - yv) * (mu - yv);
  sums[4] += e0 * e0;
  const double sd = sqrt(c);
  sums[5] += ((mu + 2.0 * sd - yv) > 0.0 && (yv - (mu - 2.0 * sd)) > 0.0) ? 1.0 : 0.0;
}

// the block's six sums → the problem's GPS_SC_* entries (one thread)
template <class P>
__device__ __forceinline__ void scores_store(const P p, int64_t pb, const double (&tot)[6]) {
  const double nt = (double)p.nt;
  double* sc = p.sc + pb * GPS_N_SC;
  sc[GPS_SC_CRPS] = tot[0] / nt;
  sc[GPS_SC_LOGS] = tot[1] / nt;
  sc[GPS_SC_MSLL] = tot[2] / nt;
  sc[GPS_SC_SMSE] = tot[3] / tot[4];
  sc[GPS_SC_MSE] = tot[3] / nt;
  sc[GPS_SC_COVER] = tot[5] / nt;
}

}  // namespace

}  // namespace gps
