// What the two tall FITC kernels with a validation set share (batch_fitc_tall_va_kernel in
// kernels_batch_fitc_tall.hip, batch_fitc_tall_block_va_kernel in kernels_batch_fitc_tall_block.hip,
// DESIGN §37): the row stream of the plain kernels' final pass as a function, the reduction of its
// six sums, the checkpoint and the NaN rows of a failed problem.  The plain kernels keep their own
// text of the loop (§25 (d), §34: sharing it moves their instructions); this is its second copy,
// expression for expression, so a row scored here carries the bits of the plain final pass at the
// same θ and Z.  L is either file's Lds: only zs, Lmi, Lbi, c, sh, th and ld are read, and after
// forward() returned 0 they hold all the stream needs.  Included once per kernel file, behind its
// Lds; everything sits in that file's anonymous namespace.
#pragma once
#include "batch_fitc_tall_shared.h"

namespace gps {

namespace {

// the problem's train-target mean and unbiased variance, in gps_fitc_set_data's order, and the
// trivial model's constant: once per launch
struct VaStats {
  double ymean, yvar, triv_c;
};

__device__ __forceinline__ VaStats va_target_stats(const double* __restrict__ y, int n) {
  double ysum = 0.0, yss = 0.0;
  for (int i = 0; i < n; ++i) ysum += y[i];
  const double ymean = ysum / n;
  for (int i = 0; i < n; ++i) yss += (y[i] - ymean) * (y[i] - ymean);
  const double yvar = yss / (n - 1);
  return {ymean, yvar, 0.5 * log(6.28318530717958647692 * yvar)};
}

// rows of ceil(itr / va_every) checkpoints and the final pass
__device__ __forceinline__ int64_t va_rows(int itr, int va_every) {
  return ((int64_t)itr + va_every - 1) / va_every + 1;
}

// nr rows xr [nr][d] streamed four at a time, one per wave: lane l < m holds k*_l and hands it round
// by shuffles; lanes a < 32 form (Lm⁻¹k*)_a, lanes 32 + a (Lb⁻¹k*)_a (rows a >= m count as zero);
// μ* = k*·c, var* = σ² + sf² − ‖Lm⁻¹k*‖² + ‖Lb⁻¹k*‖².  μ* and var* go to mu / var where given, the
// six score terms against yr (where given) into this wave's sums.  `on` is wave-uniform and covers
// the tail rows; every shuffle is executed by all lanes.
template <class L>
__device__ __forceinline__ void va_stream(const L& s, int m, int d, double sf2, double sn2,
                                          const double* __restrict__ xr,
                                          const double* __restrict__ yr, int nr, double* mu,
                                          double* var, const VaStats& st, double (&sums)[6]) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const double* il = s.th + 20;
  const int a = lane & 31;
  const bool hi = lane >= 32;
  const double* Lr = (hi ? s.Lbi : s.Lmi) + (a < m ? a : m - 1) * s.ld;
  const double cl = lane < m ? s.c[lane] : 0.0;
  for (int r0 = 0; r0 < nr; r0 += 4) {
    const int row = r0 + wave;
    const bool on = row < nr;
    double kv = 0.0;
    if (on && lane < m) {
      const double* xq = xr + (int64_t)row * d;
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (xq[k] - s.zs[lane * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      kv = sf2 * exp(-0.5 * r2);
    }
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc = fma(Lr[l], __shfl(kv, l), acc);
    const double sq = a < m ? acc * acc : 0.0;
    const double mv = wave_sum(kv * cl);
    const double q1 = wave_sum(hi ? 0.0 : sq);
    const double q2 = wave_sum(hi ? sq : 0.0);
    if (on) {
      const double c = (sn2 + sf2) - q1 + q2;
      if (mu && lane == 0) {
        mu[row] = mv;
        var[row] = c;
      }
      if (yr) score_row_add(sums, mv, c, yr[row], st.ymean, st.yvar, st.triv_c);
    }
  }
}

// the four waves' sums → the six GPS_SC_* entries of one row of nr targets, as scores_store forms
// them.  sh is free on entry (the caller is synchronised) and free again on return.
__device__ __forceinline__ void va_scores(double* sh, const double (&sums)[6], double* sc, int nr) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (lane == 0)
    for (int q = 0; q < 6; ++q) sh[q * 16 + wave] = sums[q];
  __syncthreads();
  if (t == 0) {
    double tot[6];
    for (int q = 0; q < 6; ++q) {
      double acc = 0.0;
      for (int w4 = 0; w4 < FT / 64; ++w4) acc += sh[q * 16 + w4];
      tot[q] = acc;
    }
    const double nt = (double)nr;
    sc[GPS_SC_CRPS] = tot[0] / nt;
    sc[GPS_SC_LOGS] = tot[1] / nt;
    sc[GPS_SC_MSLL] = tot[2] / nt;
    sc[GPS_SC_SMSE] = tot[3] / tot[4];
    sc[GPS_SC_MSE] = tot[3] / nt;
    sc[GPS_SC_COVER] = tot[5] / nt;
  }
  __syncthreads();
}

// row `row` of the problem's nva: the validation rows scored at what forward() left in LDS, and the
// problem's current Z where va_z is given.  Call synchronised, after forward() returned 0; ends
// synchronised, with s.sh free for the gradient's block_sum.
template <class L>
__device__ __forceinline__ void va_checkpoint(const L& s, const BatchVaParams& va, int64_t pb,
                                              int64_t row, int64_t nva, int m, int d, double sf2,
                                              double sn2, const VaStats& st) {
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  va_stream(s, m, d, sf2, sn2, va.xv + pb * va.nv * d, va.yv + pb * va.nv, va.nv, nullptr, nullptr,
            st, sums);
  va_scores(s.sh, sums, va.va_sc + (pb * nva + row) * GPS_N_SC, va.nv);
  if (va.va_z)
    for (int e = threadIdx.x; e < m * d; e += FT) va.va_z[(pb * nva + row) * m * d + e] = s.zs[e];
}

// NaN in rows [r0, r1) of a failed problem's va_sc and va_z
__device__ __forceinline__ void va_nan_rows(const BatchVaParams& va, int64_t pb, int64_t nva,
                                            int64_t r0, int64_t r1, int m, int d) {
  const int t = threadIdx.x;
  for (int64_t e = r0 * GPS_N_SC + t; e < r1 * GPS_N_SC; e += FT)
    va.va_sc[pb * nva * GPS_N_SC + e] = batch_nan();
  if (va.va_z)
    for (int64_t e = r0 * m * d + t; e < r1 * m * d; e += FT)
      va.va_z[pb * nva * m * d + e] = batch_nan();
}

// The end of a VA kernel, behind train_write_back and the store of info: a failed problem's NaN
// rows from the first step `vfrom` of this launch whose row was not written, the final pass's row
// nva − 1 at the final pass's parameters, then the test rows as the plain kernel streams them.
template <class L>
__device__ __forceinline__ void va_finish(const L& s, const BatchFitcParams& p,
                                          const BatchVaParams& va, int64_t pb, int info, int vfrom,
                                          double sf2, double sn2, const double (&obj)[GPS_N_OBJ],
                                          const VaStats& st) {
  const int m = p.m, d = p.d, t = threadIdx.x;
  const int64_t nva = va_rows(p.itr, va.va_every);
  if (info) {
    const int64_t ve = va.va_every, s1 = p.step0 + p.nsteps;
    va_nan_rows(va, pb, nva, (vfrom + ve - 1) / ve, p.do_final ? nva : (s1 + ve - 1) / ve, m, d);
  }
  if (!p.do_final) return;
  const bool pred = p.xt != nullptr && p.nt > 0;
  const bool more = final_outputs<FT>(p, pb, t, info, pred, obj);
  if (info) return;
  va_checkpoint(s, va, pb, nva - 1, nva, m, d, sf2, sn2, st);
  if (!more) return;
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  va_stream(s, m, d, sf2, sn2, p.xt + pb * p.nt * d, p.yt ? p.yt + pb * p.nt : nullptr, p.nt,
            p.mu + pb * p.nt, p.var + pb * p.nt, st, sums);
  if (!p.yt) return;
  va_scores(s.sh, sums, p.sc + pb * GPS_N_SC, p.nt);
}

// whether this launch scores anything: a checkpoint among its steps, or the final pass
__device__ __forceinline__ bool va_launch_scores(const BatchFitcParams& p, int va_every) {
  const int64_t ve = va_every, first = (p.step0 + ve - 1) / ve * ve;
  return p.do_final || first < (int64_t)p.step0 + p.nsteps;
}

}  // namespace

}  // namespace gps
