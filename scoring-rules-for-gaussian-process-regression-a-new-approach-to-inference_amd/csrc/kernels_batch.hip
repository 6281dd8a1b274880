// Batches of small full GPs, one workgroup of 256 threads per problem: objective value and
// analytic gradient, the SGD fit loop (KF:236-260, SD:192-231 / 277-301 / 372-396) and the final
// test predictive with its scores (KF:267-299), all without leaving the CU.  The whole n×(n+1)
// matrix (n <= GPS_SURFACE_MAX_N) lives in dynamic LDS, as in the surface kernel; workgroups
// never communicate, the hardware queues those beyond the resident set.  DESIGN §19.
//
// One evaluation at θ restates oracle/gp_oracle.py fast_full_fit / grad_weight_matrix /
// grad_contract (the algebra of gps_full_grad):
//   forward   A = K + σ²I (lower); the Cholesky factor and its inverse X = L⁻¹ in ONE sweep over
//             the pivots (step k scales row k of X, forms column k of L and applies the rank-one
//             update to the rows below: the trailing Cholesky update right of column k, the
//             forward substitution of the identity left of it, whose columns of L are dead);
//             β = Xy, α = Xᵀβ, d = colsum(X∘X), log|A| → the five GPS_OBJ_* entries
//   gradient  P = A⁻¹ = XᵀX: the strict upper triangle is free and zeroed, so every row of the
//             array is a row of the triangular X; each thread sums its 8×8 (stride 16) register
//             tile of P and, once X is dead, writes it to both triangles;
//             NLML  M = ½(P − ααᵀ);
//             LOO   M = −½(vαᵀ + αvᵀ) − P diag(c̃) P,  u = −g_μ/d, c̃ = (g_μα − g_c)/d², v = Pu;
//             M is never stored: the thread that summed a tile of P diag(c̃) P (registers again,
//             parked over the P entries they stand at) contracts each M_ij with ∂A_ij/∂θ, K_ij
//             recomputed from the features, into [ΣMK, tr M, ΣMKΔ_k²/ℓ_k²]; one fixed-order block sum.
// The k loops are LDS-bandwidth bound (plain FP64 FMAs from LDS, not the MFMA: DESIGN §19).
// Every reduction order is a function of n, d and the 256 threads only: results are bitwise
// reproducible and independent of the batch size, the problem's position and the launch split.
#include "batch_driver.h"
#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

constexpr int BT = 256;               // threads per workgroup: a 16×16 grid of (ti, tj)
constexpr int BR = 8;                 // register-tile edge: rows ti + 16a, columns tj + 16b
constexpr int BG = 2 + GPS_BATCH_MAX_D;  // gradient sums: ΣMK, tr M, per-dimension
constexpr int kThDoubles = 40;        // θ (<= 18) then 1/ℓ_k (<= 16)
static_assert(BR * 16 == GPS_SURFACE_MAX_N, "the register tiles cover the largest matrix");

struct Lds {
  double* A;      // [n][n + 1]
  double *y, *beta, *alpha, *dinv;
  double *u, *ct, *v, *w;   // gradient vectors; the sweep's row / column; the test rows' k*
  double* xs;     // [n][d] raw features
  double* sh;     // block_sum scratch, BG·16
  double* th;     // θ, then 1/ℓ_k at th + 20
};

__device__ __forceinline__ Lds carve(double* sm, int n, int d) {
  Lds s;
  s.A = sm;
  s.y = sm + n * (n + 1);
  s.beta = s.y + n; s.alpha = s.beta + n; s.dinv = s.alpha + n;
  s.u = s.dinv + n; s.ct = s.u + n; s.v = s.ct + n; s.w = s.v + n;
  s.xs = s.w + n;
  s.sh = s.xs + n * d;
  s.th = s.sh + BG * 16;
  return s;
}

// A = K + σ²I, Cholesky and X = L⁻¹ (lower triangle of A, diagonal included), β, α, d and the
// objectives.  Returns 0, or the 1-based order of the leading minor whose pivot is not > 0 (a NaN
// pivot included) — the same value in every thread.  Ends synchronised.
__device__ __forceinline__ int forward(const Lds& s, int n, int d, double sf2, double sn2,
                                       double obj[GPS_N_OBJ]) {
  const int t = threadIdx.x, lda = n + 1;
  const double* il = s.th + 20;
  double* A = s.A;
  const int ti = t >> 4, tj = t & 15, nb = (n + 15) >> 4;
  for (int a = 0; a < nb; ++a) {  // this thread's tiles of the lower triangle
    const int i = ti + 16 * a;
    if (i >= n) continue;
    for (int b = 0; b <= a; ++b) {
      const int j = tj + 16 * b;
      if (j > i) continue;
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (s.xs[i * d + k] - s.xs[j * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      A[i * lda + j] = sf2 * exp(-0.5 * r2) + (i == j ? sn2 : 0.0);
    }
  }
  __syncthreads();
  double* w = s.w;    // step k: X_kj/L_kk (j < k), 1/L_kk (j = k), L_jk (j > k)
  double* lc = s.ct;  // step k: L_ik (i > k)
  double* piv = s.v;  // L_kk, for log|A| after the sweep (off the pivots' critical path)
  int ci[BR], cj[BR];  // clamped rows / columns of this thread's tiles
#pragma unroll
  for (int a = 0; a < BR; ++a) {
    ci[a] = min(ti + 16 * a, n - 1);
    cj[a] = min(tj + 16 * a, n - 1);
  }
  for (int k = 0; k < n; ++k) {
    const double dk = A[k * lda + k];
    if (!(dk > 0.0)) return k + 1;
    const double is = rsqrt(dk);
    if (t < n) {
      if (t < k) {
        const double x = A[k * lda + t] * is;
        w[t] = x;
        A[k * lda + t] = x;
      } else if (t == k) {
        w[t] = is;
        piv[k] = dk * is;
      } else {
        const double l = A[t * lda + k] * is;
        w[t] = l;
        lc[t] = l;
        A[t * lda + k] = 0.0;  // the update below then writes X_tk = 0 − L_tk/L_kk like any entry
      }
    }
    __syncthreads();
    if (t == 0) A[k * lda + k] = is;  // row k is not read below, the next pivot is A[k+1][k+1]
    // the rank-one update of this thread's tiles, rows below k: every load first, then the
    // stores (a store between them would order the loads behind it: all of it is one LDS array).
    // Off-diagonal tiles (b < a) lie below the diagonal whole; block row k/16 starts below row k.
    const int kb = k >> 4, k15 = k & 15;
    double wj[BR], nl[BR], old[BR][BR];
#pragma unroll
    for (int a = 0; a < BR; ++a) {
      wj[a] = w[cj[a]];
      nl[a] = -lc[ci[a]];
    }
    // loads are unconditional within the live block rows (clamped rows, never stored; a diagonal
    // tile's upper half is read and dropped): only the stores carry the per-thread conditions
#pragma unroll
    for (int a = 0; a < BR; ++a)
      if (a >= kb && a < nb) {
#pragma unroll
        for (int b = 0; b < BR; ++b)  // b <= a: a rectangular loop unrolls fully
          if (b <= a) old[a][b] = A[ci[a] * lda + tj + 16 * b];
      }
#pragma unroll
    for (int a = 0; a < BR; ++a)
      if (a >= kb && a < nb) {
        const int i = ti + 16 * a;
        if (i < n && (a > kb || ti > k15)) {
#pragma unroll
          for (int b = 0; b < BR; ++b)
            if (b < a || (b == a && tj <= ti))
              A[i * lda + tj + 16 * b] = fma(nl[a], wj[b], old[a][b]);
        }
      }
    __syncthreads();
  }
  if (t < n) {
    double b = 0.0;
    for (int j = 0; j <= t; ++j) b = fma(A[t * lda + j], s.y[j], b);
    s.beta[t] = b;
  }
  __syncthreads();
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // Σ crps, Σ logs, Σ β², Σ log L_kk
  if (t < n) {
    double a = 0.0, dj = 0.0;
    for (int i = t; i < n; ++i) {
      const double x = A[i * lda + t];
      a = fma(x, s.beta[i], a);
      dj = fma(x, x, dj);
    }
    s.alpha[t] = a;
    s.dinv[t] = dj;
    const double yy = s.y[t], m = yy - a / dj, c = 1.0 / dj;
    v[0] = crps_term(m, c, yy);
    v[1] = logs_term(m, c, yy);
    v[2] = s.beta[t] * s.beta[t];
    v[3] = log(piv[t]);
  }
  block_sum<4>(v, s.sh);
  const double hl = v[3];  // ½ log|A|
  obj[GPS_OBJ_NLML] = 0.5 * n * 1.83787706640934548356 + hl + 0.5 * v[2];
  obj[GPS_OBJ_LOO_CRPS] = v[0] / n;
  obj[GPS_OBJ_LOO_LOGS] = v[1] / n;
  obj[GPS_OBJ_LOGDET] = 2.0 * hl;
  obj[GPS_OBJ_QUAD] = v[2];
  return 0;
}

// After forward(): g = [ΣMK, tr M, ΣMKΔ_k²/ℓ_k² (k < d)] over the full symmetric M, valid in
// every thread.  Destroys X.  Ends synchronised.
__device__ __forceinline__ void gradient(const Lds& s, int n, int d, int objective, double sf2,
                                         double (&g)[BG]) {
  const int t = threadIdx.x, lda = n + 1, nb = (n + 15) >> 4;
  const int ti = t >> 4, tj = t & 15;
  const double* il = s.th + 20;
  double* A = s.A;
  const bool loo = objective != GPS_OBJ_NLML;
  if (loo && t < n) {  // score_derivs of the MEAN score, then u and c̃ (kernels_grad.hip)
    const double dd = s.dinv[t], a = s.alpha[t];
    const double c = 1.0 / dd, r = a / dd;  // y − μ_loo = α/d (kernels_grad.hip)
    double gm, gc;
    if (objective == GPS_OBJ_LOO_CRPS) {
      const double sd = sqrt(c), z = r / sd;
      const double cdf = 0.5 * (1.0 + erf(z * 0.70710678118654752440));
      const double pdf = 0.39894228040143267794 * exp(-0.5 * z * z);
      gm = 1.0 - 2.0 * cdf;
      gc = (2.0 * pdf - 0.56418958354775628695) / (2.0 * sd);
    } else {
      gm = -r / c;
      gc = 0.5 / c - r * r / (2.0 * c * c);
    }
    gm /= n;
    gc /= n;
    s.u[t] = -gm / dd;
    s.ct[t] = (gm * a - gc) / (dd * dd);
  }
  // P = XᵀX.  The strict upper triangle is free: zeroed, every row k of the array is row k of
  // the triangular X and both operands of P_ij = Σ_k X_ki X_kj come from it without masks.  Each
  // thread keeps its i >= j tiles in registers and, once every thread is done reading X, writes
  // them to both triangles (the diagonal sums as d did, term by term).
  for (int a = 0; a < nb; ++a) {
    const int i = ti + 16 * a;
    if (i >= n) continue;
    for (int b = 0; b <= a; ++b) {
      const int j = tj + 16 * b;
      if (j < i) A[j * lda + i] = 0.0;
    }
  }
  int ci[BR], cj[BR];  // clamped: a tile entry beyond n reads a valid address and is never stored
#pragma unroll
  for (int a = 0; a < BR; ++a) {
    ci[a] = min(ti + 16 * a, n - 1);
    cj[a] = min(tj + 16 * a, n - 1);
  }
  double acc[BR][BR];
#pragma unroll
  for (int a = 0; a < BR; ++a)
#pragma unroll
    for (int b = 0; b < BR; ++b) acc[a][b] = 0.0;
  __syncthreads();
#pragma unroll 2
  for (int k = 0; k < n; ++k) {
    const double* row = A + k * lda;
    double xr[BR], xc[BR];
#pragma unroll
    for (int a = 0; a < BR; ++a) {
      xr[a] = row[ci[a]];
      xc[a] = row[cj[a]];
    }
#pragma unroll
    for (int a = 0; a < BR; ++a)
      if (a < nb) {
#pragma unroll
        for (int b = 0; b < BR; ++b)
          if (b <= a) acc[a][b] = fma(xr[a], xc[b], acc[a][b]);
      }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < BR; ++a)
#pragma unroll
    for (int b = 0; b < BR; ++b) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (b <= a && j <= i && i < n) {
        A[i * lda + j] = acc[a][b];
        if (j < i) A[j * lda + i] = acc[a][b];
      }
    }
  __syncthreads();
  if (loo) {
    if (t < n) {
      double vv = 0.0;
      for (int j = 0; j < n; ++j) vv = fma(A[t * lda + j], s.u[j], vv);
      s.v[t] = vv;
    }
    __syncthreads();
  }
  // (P diag(c̃) P)_ij for this thread's i >= j tiles: P is symmetric, both operands are rows of k
#pragma unroll
  for (int a = 0; a < BR; ++a)
#pragma unroll
    for (int b = 0; b < BR; ++b) acc[a][b] = 0.0;
  if (loo) {
#pragma unroll 2
    for (int k = 0; k < n; ++k) {
      const double ck = s.ct[k];
      const double* row = A + k * lda;
      double pi[BR], pj[BR];
#pragma unroll
      for (int a = 0; a < BR; ++a) {
        pi[a] = row[ci[a]] * ck;
        pj[a] = row[cj[a]];
      }
#pragma unroll
      for (int a = 0; a < BR; ++a)
        if (a < nb) {
#pragma unroll
          for (int b = 0; b < BR; ++b)
            if (b <= a) acc[a][b] = fma(pi[a], pj[b], acc[a][b]);
        }
    }
    // every thread is done reading P: each product entry replaces the P_ij it stands at (i >= j),
    // to be read back below by the thread that wrote it — the contraction's code is too large to
    // unroll over the register tile, and M itself is still never stored
    __syncthreads();
#pragma unroll
    for (int a = 0; a < BR; ++a)
#pragma unroll
      for (int b = 0; b < BR; ++b) {
        const int i = ti + 16 * a, j = tj + 16 * b;
        if (b <= a && j <= i && i < n) A[i * lda + j] = acc[a][b];
      }
  }
#pragma unroll
  for (int q = 0; q < BG; ++q) g[q] = 0.0;
  for (int a = 0; a < nb; ++a) {
    const int i = ti + 16 * a;
    if (i >= n) continue;
    const double ai = s.alpha[i], vi = loo ? s.v[i] : 0.0;
    for (int b = 0; b <= a; ++b) {
      const int j = tj + 16 * b;
      if (j > i) continue;
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (s.xs[i * d + k] - s.xs[j * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      const double K = sf2 * exp(-0.5 * r2);
      const double aj = s.alpha[j], pij = A[i * lda + j];  // P_ij, or (P diag(c̃) P)_ij
      const double m = loo ? fma(-0.5, vi * aj + ai * s.v[j], -pij) : 0.5 * (pij - ai * aj);
      const double mk = (i == j ? 1.0 : 2.0) * m * K;  // the lower triangle stands for both
      g[0] += mk;
      if (i == j) g[1] += m;
#pragma unroll
      for (int q = 0; q < GPS_BATCH_MAX_D; ++q)
        if (q < d) {
          const double df = (s.xs[i * d + q] - s.xs[j * d + q]) * il[q];
          g[2 + q] = fma(mk, df * df, g[2 + q]);
        }
    }
  }
  block_sum<BG>(g, s.sh);
}

__global__ __launch_bounds__(BT) void batch_kernel(BatchParams p) {
  extern __shared__ double sm[];
  const int n = p.n, d = p.d, t = threadIdx.x, lda = n + 1;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, n, d);
  double* il = s.th + 20;
  int info = p.info[pb];
  int done = p.steps_done[pb];
  double stale = p.stale[pb];
  for (int e = t; e < n * d; e += BT) s.xs[e] = p.x[pb * n * d + e];
  if (t < n) s.y[t] = p.y[pb * n + t];
  if (t < nth) s.th[t] = p.theta[pb * nth + t];
  const double bscale = p.kind == GPS_RBF ? 0.5 : 1.0;
  double obj[GPS_N_OBJ];
  // the training steps of this launch, then (do_final) one more forward: the final pass at the
  // final kernel parameters, whose noise is the final σ² or, with stale_noise, the σ² the last
  // step's forward used (the scripts' module-global sigma_noise_sq)
  const int ntrain = p.mode == BATCH_MODE_GRAD ? 1 : p.nsteps;
  const int neval = ntrain + (p.mode == BATCH_MODE_TRAIN && p.do_final ? 1 : 0);
  double sf2 = 0.0, sn2 = 0.0;
  for (int st = 0; st < neval && info == 0; ++st) {
    const bool fin = st == ntrain;
    step_prologue(p, t, s.th, il, p.kind, fin, stale, sf2, sn2);
    info = forward(s, n, d, sf2, sn2, obj);
    if (info || fin) break;
    double g[BG];
    gradient(s, n, d, p.objective, sf2, g);
    if (t == 0) {
      double gr[BG];  // [∂/∂log sf², ∂/∂b (n_ell), ∂/∂log σ²]
      gr[0] = g[0];
      double tot = 0.0;
#pragma unroll
      for (int q = 0; q < GPS_BATCH_MAX_D; ++q)
        if (q < d) {
          const double gk = bscale * g[2 + q];
          if (p.n_ell != 1) gr[1 + q] = gk;
          tot += gk;
        }
      if (p.n_ell == 1) gr[1] = tot;
      const double gn = sn2 * g[1];
      if (p.mode == BATCH_MODE_GRAD) {
        for (int q = 0; q < GPS_N_OBJ; ++q) p.obj[pb * GPS_N_OBJ + q] = obj[q];
#pragma unroll
        for (int q = 0; q < BG - 1; ++q)
          if (q < nth - 1) p.grad[pb * nth + q] = gr[q];
        p.grad[pb * nth + nth - 1] = gn;
      } else {
        const int64_t si = pb * p.itr + p.step0 + st;
        p.values[si] = p.objective == GPS_OBJ_NLML ? obj[GPS_OBJ_NLML]
                       : p.objective == GPS_OBJ_LOO_CRPS ? obj[GPS_OBJ_LOO_CRPS]
                                                         : obj[GPS_OBJ_LOO_LOGS];
#pragma unroll
        for (int q = 0; q < BG - 1; ++q)
          if (q < nth - 1) {
            const double nv = s.th[q] - p.lr * gr[q];
            s.th[q] = nv;
            p.thetas[si * nth + q] = nv;
          }
        const double nv = s.th[nth - 1] - p.lr * gn;
        s.th[nth - 1] = nv;
        p.thetas[si * nth + nth - 1] = nv;
      }
    }
    ++done;
  }
  __syncthreads();

  if (p.mode == BATCH_MODE_GRAD) {
    full_grad_end(p, pb, t, info);
    return;
  }
  train_write_back<BT>(p, pb, t, s.th, nullptr, info, done, stale);
  if (!p.do_final) {
    if (t == 0) p.info[pb] = info;
    return;
  }
  if (t == 0) p.info[pb] = info;
  const bool pred = p.xt != nullptr && p.nt > 0;
  if (!final_outputs<BT>(p, pb, t, info, pred, obj)) return;
  // train-target mean and unbiased variance, in gps_full_set_data's order
  double ysum = 0.0, yss = 0.0;
  for (int i = 0; i < n; ++i) ysum += s.y[i];
  const double ymean = ysum / n;
  for (int i = 0; i < n; ++i) yss += (s.y[i] - ymean) * (s.y[i] - ymean);
  const double yvar = yss / (n - 1);
  // test rows streamed four at a time, one per wave: k* into the wave's n doubles of u..w,
  // μ* = k*·α, var* = σ² + sf² − ‖X k*‖² (lane i and i + 64 own rows of X)
  const int wave = t >> 6, lane = t & 63;
  double* kb = s.u + wave * n;
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // as score_rows_kernel, this wave's rows
  const double triv_c = 0.5 * log(6.28318530717958647692 * yvar);
  __syncthreads();
  for (int r0 = 0; r0 < p.nt; r0 += 4) {
    const int row = r0 + wave;
    const bool on = row < p.nt;
    double mu = 0.0, q = 0.0;
    if (on) {
      const double* xr = p.xt + (pb * p.nt + row) * d;
      for (int j = lane; j < n; j += 64) {
        double r2 = 0.0;
        for (int k = 0; k < d; ++k) {
          const double df = (xr[k] - s.xs[j * d + k]) * il[k];
          r2 = fma(df, df, r2);
        }
        const double kv = sf2 * exp(-0.5 * r2);
        kb[j] = kv;
        mu = fma(kv, s.alpha[j], mu);
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < n) {
          double r = 0.0;
          for (int j = 0; j <= i; ++j) r = fma(s.A[i * lda + j], kb[j], r);
          q = fma(r, r, q);
        }
      }
    }
    mu = wave_sum(mu);
    q = wave_sum(q);
    if (on) {
      const double c = (sn2 + sf2) - q;
      if (lane == 0) {
        p.mu[pb * p.nt + row] = mu;
        p.var[pb * p.nt + row] = c;
      }
      if (p.yt) {
        const double yv = p.yt[pb * p.nt + row];
        score_row_add(sums, mu, c, yv, ymean, yvar, triv_c);
      }
    }
    __syncthreads();
  }
  if (!p.yt) return;
  if (lane == 0)
    for (int q = 0; q < 6; ++q) s.sh[q * 16 + wave] = sums[q];
  __syncthreads();
  if (t == 0) {
    double tot[6];
    for (int q = 0; q < 6; ++q) {
      double a = 0.0;
      for (int w = 0; w < BT / 64; ++w) a += s.sh[q * 16 + w];
      tot[q] = a;
    }
    scores_store(p, pb, tot);
  }
}

}  // namespace

size_t batch_lds_bytes(int n, int d) {
  return (size_t)(n * (n + 1) + 8 * n + n * d + BG * 16 + kThDoubles) * sizeof(double);
}

hipError_t launch_batch(const BatchParams& p, hipStream_t s) {
  if (p.n < 1 || p.n > GPS_SURFACE_MAX_N || p.d < 1 || p.d > GPS_BATCH_MAX_D || p.nprob < 1 ||
      (p.n_ell != 1 && p.n_ell != p.d) || p.nsteps < 0 || p.nsteps > kBatchStepsPerLaunch)
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds(
      (const void*)batch_kernel, batch_lds_bytes(GPS_SURFACE_MAX_N, GPS_BATCH_MAX_D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_kernel, dim3((unsigned)p.nprob), dim3(BT), batch_lds_bytes(p.n, p.d), s,
                     p);
  return hipGetLastError();
}

}  // namespace gps
