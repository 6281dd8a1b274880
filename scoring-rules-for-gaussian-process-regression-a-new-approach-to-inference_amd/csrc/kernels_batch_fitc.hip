// Batches of small FITC GPs, one workgroup of 256 threads per problem: objective value and the
// analytic gradient with respect to θ and the inducing inputs Z, the SGD fit loop of
// "SIMPLE-FITC--comapre.py" (SF:189-237, 301-343, 420-463: θ -= lr·g, Z -= lr_z·g_Z) and the final
// test predictive with its scores, all without leaving the CU.  n <= GPS_SURFACE_MAX_N training
// points, m <= GPS_BATCH_FITC_MAX_M inducing inputs (m > n is legal), d <= GPS_BATCH_MAX_D; every
// array lives in dynamic LDS (carve below, the table is in DESIGN §20); workgroups never
// communicate.  The sibling of kernels_batch.hip.
//
// One evaluation at (θ, Z) restates oracle/gp_oracle.py fast_fitc / fast_fitc_grad / fitc_contract
// in their whitened form (no explicit Km⁻¹ or B⁻¹, the oracle's docstring says why):
//   forward   K̃mm = K(Z,Z) + 1e-3·I → Lm⁻¹ (chol_inv: the factor and its inverse in one sweep);
//             K = K(X,Z), V = K Lm⁻ᵀ, q_i = ‖V_i‖², λ = sf² − q + σ²;
//             B = K̃mm + KᵀΛ⁻¹K, b = KᵀΛ⁻¹y → Lb⁻¹, c = Lb⁻ᵀLb⁻¹b;
//             U = K Lb⁻ᵀ in K's place (row by row, columns descending), r_i = ‖U_i‖²,
//             d_i = 1/λ_i − r_i/λ_i², α = (y − Kc)/λ, LOO μ = y − α/d, σ² = 1/d → the GPS_OBJ_* entries
//   gradient  (a, v, h) of the objective (NLML: ½, ½α, 0; LOO: 0, C⁻¹u by Woodbury, c̃);
//             P = Uᵀdiag(h/λ²)U, (UP)_i·U_i, M_ii, ŵ = Lm⁻ᵀ(Vᵀv), S = Vᵀdiag(M_ii)V;
//             G_Km = Lb⁻ᵀ(P + aI)Lb⁻¹ + Lm⁻ᵀ(S − aI)Lm⁻¹ + ½(ŵcᵀ + cŵᵀ)   (m×m, stored);
//             G_K  = [diag(2(a/λ − h/λ²))U + diag(2/λ)UP]Lb⁻¹ − diag(2M_ii)V Lm⁻¹ − vcᵀ − αŵᵀ is
//             never stored: the thread that forms G_K[i][j] multiplies it with K_ij (recomputed
//             from the features) and contracts it with ∂K/∂θ and ∂K/∂z_j on the spot, then does
//             the same with row j of G_Km ∘ K(Z,Z).
// Reductions: a column (or m×m entry) is owned by a group of C adjacent lanes (C a power of two
// <= 64 fixed by m), lane c sums rows c, c + C, ... in order and the group adds its lanes by a
// butterfly of shuffles; block-wide sums are block_sum's fixed tree.  No atomics: every order is
// a function of n, m, d and the 256 threads only, so results are bitwise independent of the
// batch size, the problem's position and the launch split.  Every loop bound is a function of
// n, m, d, nt and nsteps; every exit is workgroup-uniform (the pivots are read from LDS by all).
// Plain FP64 FMAs: at SF's m = 5 a step is barrier- and latency-bound.
#include "batch_fitc_shared.h"  // FT, FG, odd_ld, group_lanes, group_sum, block_sum_n, chol_inv
#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

constexpr int kNVec = 9, kMVec = 9, kMMat = 6;

struct Lds {
  double *xs, *zs, *y;                     // [n][d], [m][d], [n]
  double *V, *U;                           // [n][ldv]; U's array holds K until the row pass
  double *Lmi, *Lbi;                       // [m][ldm] Lm⁻¹, Lb⁻¹ (strict upper triangle zero)
  double *P, *PL, *S, *SL;                 // [m][ldm] K̃mm → P → G_Km; P Lb⁻¹; S; S Lm⁻¹
  double *lam, *alpha, *dinv, *r, *w1, *w2, *v, *h, *md;   // [n]
  double *b, *beta, *c, *tv, *wh, *pivm, *pivb, *wv, *lc;   // [m]
  double* sh;                              // block_sum scratch, FG·16
  double* th;                              // θ, then 1/ℓ_k at th + 20
  int ldv, ldm;
};

__device__ __forceinline__ Lds carve(double* sm, int n, int m, int d) {
  Lds s;
  s.ldv = odd_ld(m);
  s.ldm = odd_ld(m);
  double* p = sm;
  auto take = [&p](int k) { double* q = p; p += k; return q; };
  s.xs = take(n * d); s.zs = take(m * d); s.y = take(n);
  s.V = take(n * s.ldv); s.U = take(n * s.ldv);
  s.Lmi = take(m * s.ldm); s.Lbi = take(m * s.ldm);
  s.P = take(m * s.ldm); s.PL = take(m * s.ldm); s.S = take(m * s.ldm); s.SL = take(m * s.ldm);
  s.lam = take(n); s.alpha = take(n); s.dinv = take(n); s.r = take(n); s.w1 = take(n);
  s.w2 = take(n); s.v = take(n); s.h = take(n); s.md = take(n);
  s.b = take(m); s.beta = take(m); s.c = take(m); s.tv = take(m); s.wh = take(m);
  s.pivm = take(m); s.pivb = take(m); s.wv = take(m); s.lc = take(m);
  s.sh = take(FG * 16);
  s.th = take(kThDoubles);
  return s;
}

// out[j] = Σ_i A[i][j]·w[i] (j < m): group j of C lanes, lane c takes rows c, c + C, ...
__device__ __forceinline__ void tmatvec(const double* A, int lda, const double* w, int n, int m,
                                        double* out) {
  const int C = group_lanes(m), j = threadIdx.x / C, c = threadIdx.x - j * C;
  double a = 0.0;
  if (j < m)
    for (int i = c; i < n; i += C) a = fma(A[i * lda + j], w[i], a);
  a = group_sum(a, C);
  if (j < m && c == 0) out[j] = a;
}

// out[j][l] = (base ? base[j][l] : 0) + Σ_i A[i][j]·A[i][l]·w[i] for all m×m entries (the product
// A_ij·A_il is formed first, so the result is bitwise symmetric).  Up to 128 entries share the
// workgroup as tmatvec's columns do; more take one thread each, 256 at a time.
__device__ __forceinline__ void wgram(const double* A, int lda, const double* w, int n, int m,
                                      const double* base, double* out, int ldm) {
  const int ne = m * m;
  const int C = ne <= FT / 2 ? group_lanes(ne) : 1, G = FT / C;
  const int g = threadIdx.x / C, c = threadIdx.x - g * C;
  for (int e0 = 0; e0 < ne; e0 += G) {
    const int e = e0 + g;
    const bool on = e < ne;
    const int j = on ? e / m : 0, l = on ? e - j * m : 0;
    double a = 0.0;
    if (on)
      for (int i = c; i < n; i += C) a = fma(A[i * lda + j] * A[i * lda + l], w[i], a);
    a = group_sum(a, C);
    if (on && c == 0) out[j * ldm + l] = base ? base[j * ldm + l] + a : a;
  }
}

// K̃mm, Lm⁻¹, K, V, λ, B, b, Lb⁻¹, c, U, r, d, α and the objectives.  Returns 0, k (K̃mm's
// leading minor of order k is not > 0) or m + k (B's) — the same value in every thread.  Call with
// θ's sf2 / sn2 / 1/ℓ and Z visible; ends synchronised.
__device__ __forceinline__ int forward(const Lds& s, int n, int m, int d, double sf2, double sn2,
                                       double obj[GPS_N_OBJ]) {
  const int t = threadIdx.x, ldv = s.ldv, ldm = s.ldm;
  const double* il = s.th + 20;
  for (int e = t; e < m * m; e += FT) {
    const int j = e / m, l = e - j * m;
    double r2 = 0.0;
    for (int k = 0; k < d; ++k) {
      const double df = (s.zs[j * d + k] - s.zs[l * d + k]) * il[k];
      r2 = fma(df, df, r2);
    }
    const double kv = sf2 * exp(-0.5 * r2) + (j == l ? kJitter : 0.0);
    s.Lmi[j * ldm + l] = kv;
    s.P[j * ldm + l] = kv;
  }
  for (int e = t; e < n * m; e += FT) {
    const int i = e / m, l = e - i * m;
    double r2 = 0.0;
    for (int k = 0; k < d; ++k) {
      const double df = (s.xs[i * d + k] - s.zs[l * d + k]) * il[k];
      r2 = fma(df, df, r2);
    }
    s.U[i * ldv + l] = sf2 * exp(-0.5 * r2);
  }
  __syncthreads();
  int info = chol_inv(s.Lmi, m, ldm, s.pivm, s.wv, s.lc);
  if (info) return info;
  for (int e = t; e < n * m; e += FT) {  // V = K Lm⁻ᵀ
    const int i = e / m, a = e - i * m;
    double acc = 0.0;
    for (int l = 0; l <= a; ++l) acc = fma(s.U[i * ldv + l], s.Lmi[a * ldm + l], acc);
    s.V[i * ldv + a] = acc;
  }
  __syncthreads();
  if (t < n) {
    double q = 0.0;
    for (int a = 0; a < m; ++a) q = fma(s.V[t * ldv + a], s.V[t * ldv + a], q);
    const double lam = sf2 - q + sn2;
    s.lam[t] = lam;
    s.w1[t] = 1.0 / lam;
    s.w2[t] = s.y[t] / lam;
  }
  __syncthreads();
  wgram(s.U, ldv, s.w1, n, m, s.P, s.Lbi, ldm);  // B = K̃mm + KᵀΛ⁻¹K
  tmatvec(s.U, ldv, s.w2, n, m, s.b);            // b = KᵀΛ⁻¹y
  __syncthreads();
  info = chol_inv(s.Lbi, m, ldm, s.pivb, s.wv, s.lc);
  if (info) return m + info;
  if (t < m) {
    double a = 0.0;
    for (int l = 0; l <= t; ++l) a = fma(s.Lbi[t * ldm + l], s.b[l], a);
    s.beta[t] = a;
  }
  __syncthreads();
  if (t < m) {
    double a = 0.0;
    for (int q = t; q < m; ++q) a = fma(s.Lbi[q * ldm + t], s.beta[q], a);
    s.c[t] = a;
  }
  __syncthreads();
  // Σ crps, Σ logs, Σ log λ, Σ y²/λ, b·c, Σ log (Lb_kk / Lm_kk)
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < n) {
    double* row = s.U + t * ldv;  // K_t·, turned into U_t· from the last column down
    double g = 0.0, r = 0.0;
    for (int l = 0; l < m; ++l) g = fma(row[l], s.c[l], g);
    for (int a = m - 1; a >= 0; --a) {
      double acc = 0.0;
      for (int l = 0; l <= a; ++l) acc = fma(row[l], s.Lbi[a * ldm + l], acc);
      row[a] = acc;
      r = fma(acc, acc, r);
    }
    const double lam = s.lam[t], yy = s.y[t];
    const double dinv = 1.0 / lam - r / (lam * lam);
    const double al = (yy - g) / lam;
    s.r[t] = r;
    s.dinv[t] = dinv;
    s.alpha[t] = al;
    const double mu = yy - al / dinv, cv = 1.0 / dinv;
    v[0] = crps_term(mu, cv, yy);
    v[1] = logs_term(mu, cv, yy);
    v[2] = log(lam);
    v[3] = yy * yy / lam;
  }
  if (t < m) {
    v[4] = s.b[t] * s.c[t];
    v[5] = log(s.pivb[t]) - log(s.pivm[t]);
  }
  block_sum<6>(v, s.sh);
  const double logdet = v[2] + 2.0 * v[5], quad = v[3] - v[4];
  obj[GPS_OBJ_NLML] = 0.5 * n * 1.83787706640934548356 + 0.5 * logdet + 0.5 * quad;
  obj[GPS_OBJ_LOO_CRPS] = v[0] / n;
  obj[GPS_OBJ_LOO_LOGS] = v[1] / n;
  obj[GPS_OBJ_LOGDET] = logdet;
  obj[GPS_OBJ_QUAD] = quad;
  return 0;
}

// After forward(): g = [ΣG_K∘K + ΣG_Km∘K(Z,Z), ΣM_ii, the per-dimension ∂/∂log ℓ_k sums], valid in
// every thread; gz[k] = ∂/∂z_jk, valid in the first lane (c == 0) of column group j < m, whose
// column and lane the caller gets in (*col, *lane0).  Ends synchronised.
__device__ __forceinline__ void gradient(const Lds& s, int n, int m, int d, int objective,
                                         double sf2, double (&g)[FG],
                                         double (&gz)[GPS_BATCH_MAX_D], int* col, bool* lane0) {
  const int t = threadIdx.x, ldv = s.ldv, ldm = s.ldm;
  const double* il = s.th + 20;
  const bool loo = objective != GPS_OBJ_NLML;
  const double ac = loo ? 0.0 : 0.5;
  if (t < n) {  // score_derivs of the MEAN score, then u and h = c̃ (kernels_grad.hip)
    const double dd = s.dinv[t], a = s.alpha[t], yy = s.y[t], lam = s.lam[t];
    double h = 0.0;
    if (loo) {
      const double mu = yy - a / dd, c = 1.0 / dd, r = yy - mu;
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
      h = (gm * a - gc) / (dd * dd);
      s.w1[t] = (-gm / dd) / lam;  // u/λ
    } else {
      s.v[t] = 0.5 * a;
    }
    s.h[t] = h;
    s.w2[t] = h / (lam * lam);
  }
  __syncthreads();
  if (loo) {  // v = C⁻¹u = u/λ − U(Uᵀ(u/λ))/λ
    tmatvec(s.U, ldv, s.w1, n, m, s.tv);
    __syncthreads();
    if (t < n) {
      double a = 0.0;
      for (int q = 0; q < m; ++q) a = fma(s.U[t * ldv + q], s.tv[q], a);
      s.v[t] = s.w1[t] - a / s.lam[t];
    }
  }
  wgram(s.U, ldv, s.w2, n, m, nullptr, s.P, ldm);  // P = Uᵀdiag(h/λ²)U
  __syncthreads();
  for (int e = t; e < m * m; e += FT) {  // PL = P Lb⁻¹
    const int a = e / m, l = e - a * m;
    double acc = 0.0;
    for (int q = l; q < m; ++q) acc = fma(s.P[a * ldm + q], s.Lbi[q * ldm + l], acc);
    s.PL[a * ldm + l] = acc;
  }
  if (t < n) {  // M_ii
    const double* u = s.U + t * ldv;
    double q = 0.0;
    for (int a = 0; a < m; ++a) {
      double up = 0.0;
      for (int b = 0; b < m; ++b) up = fma(u[b], s.P[b * ldm + a], up);
      q = fma(up, u[a], q);
    }
    const double lam = s.lam[t], h = s.h[t], l2 = lam * lam;
    s.md[t] = ac * s.dinv[t] - s.v[t] * s.alpha[t] -
              (h / l2 - 2.0 * h * s.r[t] / (l2 * lam) + q / l2);
  }
  __syncthreads();
  tmatvec(s.V, ldv, s.v, n, m, s.tv);                // Vᵀv
  wgram(s.V, ldv, s.md, n, m, nullptr, s.S, ldm);    // S = Vᵀdiag(M_ii)V
  __syncthreads();
  if (t < m) {  // ŵ = Lm⁻ᵀ(Vᵀv)
    double a = 0.0;
    for (int q = t; q < m; ++q) a = fma(s.Lmi[q * ldm + t], s.tv[q], a);
    s.wh[t] = a;
  }
  for (int e = t; e < m * m; e += FT) {  // SL = S Lm⁻¹
    const int a = e / m, l = e - a * m;
    double acc = 0.0;
    for (int q = l; q < m; ++q) acc = fma(s.S[a * ldm + q], s.Lmi[q * ldm + l], acc);
    s.SL[a * ldm + l] = acc;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += FT) {  // G_Km, over P (dead)
    const int j = e / m, l = e - j * m;
    double a1 = 0.0, a2 = 0.0;
    for (int q = j; q < m; ++q) {
      a1 = fma(s.Lbi[q * ldm + j], fma(ac, s.Lbi[q * ldm + l], s.PL[q * ldm + l]), a1);
      a2 = fma(s.Lmi[q * ldm + j], fma(-ac, s.Lmi[q * ldm + l], s.SL[q * ldm + l]), a2);
    }
    s.P[j * ldm + l] = a1 + a2 + 0.5 * (s.wh[j] * s.c[l] + s.c[j] * s.wh[l]);
  }
  __syncthreads();
  // the contraction: column group j, lane c takes rows c, c + C, ... of G_K∘K and entries
  // c, c + C, ... of row j of G_Km∘K(Z,Z)
  const int C = group_lanes(m), j = t / C, c = t - j * C;
  double g0 = 0.0, gl[GPS_BATCH_MAX_D];
#pragma unroll
  for (int k = 0; k < GPS_BATCH_MAX_D; ++k) {
    gl[k] = 0.0;
    gz[k] = 0.0;
  }
  if (j < m) {
    const double cj = s.c[j], wj = s.wh[j];
    for (int i = c; i < n; i += C) {
      const double lam = s.lam[i], hi = s.h[i];
      const double s1 = 2.0 * (ac / lam - hi / (lam * lam)), s2 = 2.0 / lam;
      double t1 = 0.0, t2 = 0.0, t3 = 0.0;
      for (int a = 0; a < m; ++a) {
        const double u = s.U[i * ldv + a];
        t1 = fma(u, s.Lbi[a * ldm + j], t1);
        t2 = fma(u, s.PL[a * ldm + j], t2);
        t3 = fma(s.V[i * ldv + a], s.Lmi[a * ldm + j], t3);
      }
      const double gk = s1 * t1 + s2 * t2 - 2.0 * s.md[i] * t3 - s.v[i] * cj - s.alpha[i] * wj;
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (s.xs[i * d + k] - s.zs[j * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      const double gkk = gk * (sf2 * exp(-0.5 * r2));
      g0 += gkk;
#pragma unroll
      for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
        if (k < d) {
          const double df = (s.xs[i * d + k] - s.zs[j * d + k]) * il[k];
          gl[k] = fma(gkk, df * df, gl[k]);
          gz[k] = fma(gkk, df, gz[k]);
        }
    }
    for (int l = c; l < m; l += C) {
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (s.zs[j * d + k] - s.zs[l * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      const double gmk = s.P[j * ldm + l] * (sf2 * exp(-0.5 * r2));  // K(Z,Z) without the jitter
      g0 += gmk;
#pragma unroll
      for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
        if (k < d) {
          const double df = (s.zs[j * d + k] - s.zs[l * d + k]) * il[k];
          gl[k] = fma(gmk, df * df, gl[k]);
          gz[k] = fma(-2.0 * gmk, df, gz[k]);
        }
    }
  }
#pragma unroll
  for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
    if (k < d) gz[k] = group_sum(gz[k], C) * il[k];
  g[0] = g0;
  g[1] = t < n ? s.md[t] : 0.0;
#pragma unroll
  for (int k = 0; k < GPS_BATCH_MAX_D; ++k) g[2 + k] = gl[k];
  block_sum_n<FG>(g, 2 + d, s.sh);
  *col = j;
  *lane0 = j < m && c == 0;
}

__global__ __launch_bounds__(FT) void batch_fitc_kernel(BatchFitcParams p) {
  extern __shared__ double sm[];
  const int n = p.n, m = p.m, d = p.d, t = threadIdx.x;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, n, m, d);
  double* il = s.th + 20;
  int info = p.info[pb];
  int done = p.steps_done[pb];
  double stale = p.stale[pb];
  for (int e = t; e < n * d; e += FT) s.xs[e] = p.x[pb * n * d + e];
  for (int e = t; e < m * d; e += FT) s.zs[e] = p.z[pb * m * d + e];
  if (t < n) s.y[t] = p.y[pb * n + t];
  if (t < nth) s.th[t] = p.theta[pb * nth + t];
  double obj[GPS_N_OBJ];
  // the training steps of this launch, then (do_final) one more forward: the final pass at the
  // final θ and Z, whose noise is the final σ² or, with stale_noise, the σ² the last step's
  // forward used (kernels_batch.hip)
  const int ntrain = p.mode == BATCH_MODE_GRAD ? 1 : p.nsteps;
  const int neval = ntrain + (p.mode == BATCH_MODE_TRAIN && p.do_final ? 1 : 0);
  double sf2 = 0.0, sn2 = 0.0;
  for (int st = 0; st < neval && info == 0; ++st) {
    const bool fin = st == ntrain;
    step_prologue(p, t, s.th, il, GPS_ARD, fin, stale, sf2, sn2);
    info = forward(s, n, m, d, sf2, sn2, obj);
    if (info || fin) break;
    double g[FG], gz[GPS_BATCH_MAX_D];
    int col;
    bool lane0;
    gradient(s, n, m, d, p.objective, sf2, g, gz, &col, &lane0);
    const double gn = sn2 * g[1];
    if (p.mode == BATCH_MODE_GRAD) {
      if (t == 0) {
        for (int q = 0; q < GPS_N_OBJ; ++q) p.obj[pb * GPS_N_OBJ + q] = obj[q];
        p.grad[pb * nth] = g[0] + sf2 * g[1];
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < GPS_BATCH_MAX_D; ++q)
          if (q < d) {
            if (p.n_ell != 1) p.grad[pb * nth + 1 + q] = g[2 + q];
            tot += g[2 + q];
          }
        if (p.n_ell == 1) p.grad[pb * nth + 1] = tot;
        p.grad[pb * nth + nth - 1] = gn;
      }
      if (lane0)
#pragma unroll
        for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
          if (k < d) p.grad_z[(pb * m + col) * d + k] = gz[k];
    } else {
      // every read of θ and Z of this step lies before gradient()'s closing barriers
      if (t == 0) {
        const int64_t si = pb * p.itr + p.step0 + st;
        p.values[si] = p.objective == GPS_OBJ_NLML ? obj[GPS_OBJ_NLML]
                       : p.objective == GPS_OBJ_LOO_CRPS ? obj[GPS_OBJ_LOO_CRPS]
                                                         : obj[GPS_OBJ_LOO_LOGS];
        double nv = s.th[0] - p.lr * (g[0] + sf2 * g[1]);
        s.th[0] = nv;
        p.thetas[si * nth] = nv;
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < GPS_BATCH_MAX_D; ++q)
          if (q < d) {
            if (p.n_ell != 1) {
              nv = s.th[1 + q] - p.lr * g[2 + q];
              s.th[1 + q] = nv;
              p.thetas[si * nth + 1 + q] = nv;
            }
            tot += g[2 + q];
          }
        if (p.n_ell == 1) {
          nv = s.th[1] - p.lr * tot;
          s.th[1] = nv;
          p.thetas[si * nth + 1] = nv;
        }
        nv = s.th[nth - 1] - p.lr * gn;
        s.th[nth - 1] = nv;
        p.thetas[si * nth + nth - 1] = nv;
      }
      if (lane0)
#pragma unroll
        for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
          if (k < d) s.zs[col * d + k] -= p.lr_z * gz[k];
    }
    ++done;
  }
  __syncthreads();

  if (p.mode == BATCH_MODE_GRAD) {
    fitc_grad_end(p, pb, t, info);
    return;
  }
  train_write_back<FT>(p, pb, t, s.th, s.zs, info, done, stale);
  if (t == 0) p.info[pb] = info;
  if (!p.do_final) return;
  const bool pred = p.xt != nullptr && p.nt > 0;
  if (!final_outputs<FT>(p, pb, t, info, pred, obj)) return;
  // train-target mean and unbiased variance, in gps_fitc_set_data's order
  double ysum = 0.0, yss = 0.0;
  for (int i = 0; i < n; ++i) ysum += s.y[i];
  const double ymean = ysum / n;
  for (int i = 0; i < n; ++i) yss += (s.y[i] - ymean) * (s.y[i] - ymean);
  const double yvar = yss / (n - 1);
  // test rows streamed four at a time, one per wave: lane l < m holds k*_l and hands it round by
  // shuffles; lanes a < 32 form (Lm⁻¹k*)_a, lanes 32 + a (Lb⁻¹k*)_a (rows a >= m count as zero);
  // μ* = k*·c, var* = σ² + sf² − ‖Lm⁻¹k*‖² + ‖Lb⁻¹k*‖²
  const int wave = t >> 6, lane = t & 63;
  const int a = lane & 31;
  const bool hi = lane >= 32;
  const double* Lr = (hi ? s.Lbi : s.Lmi) + (a < m ? a : m - 1) * s.ldm;
  const double cl = lane < m ? s.c[lane] : 0.0;
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // as score_rows_kernel, this wave's rows
  const double triv_c = 0.5 * log(6.28318530717958647692 * yvar);
  for (int r0 = 0; r0 < p.nt; r0 += 4) {
    const int row = r0 + wave;
    const bool on = row < p.nt;
    double kv = 0.0;
    if (on && lane < m) {
      const double* xr = p.xt + (pb * p.nt + row) * d;
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (xr[k] - s.zs[lane * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      kv = sf2 * exp(-0.5 * r2);
    }
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc = fma(Lr[l], __shfl(kv, l), acc);
    const double sq = a < m ? acc * acc : 0.0;
    const double mu = wave_sum(kv * cl);
    const double q1 = wave_sum(hi ? 0.0 : sq);
    const double q2 = wave_sum(hi ? sq : 0.0);
    if (on) {
      const double c = (sn2 + sf2) - q1 + q2;
      if (lane == 0) {
        p.mu[pb * p.nt + row] = mu;
        p.var[pb * p.nt + row] = c;
      }
      if (p.yt) {
        const double yv = p.yt[pb * p.nt + row];
        score_row_add(sums, mu, c, yv, ymean, yvar, triv_c);
      }
    }
  }
  if (!p.yt) return;
  if (lane == 0)
    for (int q = 0; q < 6; ++q) s.sh[q * 16 + wave] = sums[q];
  __syncthreads();
  if (t == 0) {
    double tot[6];
    for (int q = 0; q < 6; ++q) {
      double acc = 0.0;
      for (int w = 0; w < FT / 64; ++w) acc += s.sh[q * 16 + w];
      tot[q] = acc;
    }
    scores_store(p, pb, tot);
  }
}

}  // namespace

size_t batch_fitc_lds_bytes(int n, int m, int d) {
  const int ld = odd_ld(m);
  return (size_t)(n * d + m * d + n + 2 * n * ld + kMMat * m * ld + kNVec * n + kMVec * m +
                  FG * 16 + kThDoubles) * sizeof(double);
}

hipError_t launch_batch_fitc(const BatchFitcParams& p, hipStream_t s) {
  if (p.n < 1 || p.n > GPS_SURFACE_MAX_N || p.m < 1 || p.m > GPS_BATCH_FITC_MAX_M || p.d < 1 ||
      p.d > GPS_BATCH_MAX_D || p.nprob < 1 || (p.n_ell != 1 && p.n_ell != p.d) || p.nsteps < 0 ||
      p.nsteps > kBatchStepsPerLaunch)
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds(
      (const void*)batch_fitc_kernel,
      batch_fitc_lds_bytes(GPS_SURFACE_MAX_N, GPS_BATCH_FITC_MAX_M, GPS_BATCH_MAX_D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_fitc_kernel, dim3((unsigned)p.nprob), dim3(FT),
                     batch_fitc_lds_bytes(p.n, p.m, p.d), s, p);
  return hipGetLastError();
}

}  // namespace gps
