// Batches of tall FITC GPs, one workgroup of 256 threads per problem: kernels_batch_fitc.hip's
// sibling for n up to GPS_BATCH_FITC_TALL_MAX_N training points ("KIN40K-COMPARE-ALL-FITC-20":
// n = 500, d = 8, m = 20).  Same model, same algebra (the whitened fast_fitc / fast_fitc_grad /
// fitc_contract of oracle/gp_oracle.py, no explicit Km⁻¹ or B⁻¹), same training loop and final
// pass; what differs is where the n-sized arrays live.  V, U (n×ld each) and the nine n-vectors
// sit in a per-problem device workspace that only this workgroup writes and reads, so
// __syncthreads() is all the ordering it needs (no device-scope fence, no atomic); X and y are
// read from the input buffer.  LDS holds the six m×m arrays, the m-vectors, Z, θ, 1/ℓ, the
// reduction scratch and ONE chunk of kTallChunk rows of whatever the current pass needs (two
// chunk×ld arrays A and Bf, the chunk's rows of X and five chunk-vectors).  A chunk moves between
// the workspace and LDS as one contiguous block with twelve loads in flight per thread
// (copy_flat): with one wave per SIMD nothing else hides a memory round trip.  The passes over
// the chunks:
//   1  K → V → q, λ; B = K̃mm + KᵀΛ⁻¹K and b = KᵀΛ⁻¹y accumulated chunk after chunk.  K is stored in
//      U's array (an L2 round trip is cheaper than n·m more exps)
//   2  after Lb⁻¹ and c: g, U = K Lb⁻ᵀ over K, r, d, α, the LOO moments, the objective sums, the
//      score derivatives (h, u/λ, h/λ²) and Uᵀ(u/λ)
//   3  v = u/λ − U(Uᵀ(u/λ))/λ; P = Uᵀdiag(h/λ²)U and Vᵀv
//   4  (UP)_i·U_i, M_ii; S = Vᵀdiag(M_ii)V and ΣM_ii
//   5  G_K formed entry by entry and contracted with ∂K/∂θ, ∂K/∂z_j on the spot, then G_Km∘K(Z,Z)
// Reductions: as the small kernel, a column (or m×m entry) is owned by a group of C lanes, lane c
// sums rows c, c + C, ... of the chunk in order, the group adds its lanes by a butterfly, and the
// group's first lane adds the chunk's sum to the running total in LDS: chunks in ascending order.
// kTallChunk is a multiple of every C, so the order is a function of n, m, d and the 256 threads
// only: results are bitwise independent of the batch size, the problem's position and the
// launch split.  Every loop bound is a function of n, m, d, nt and nsteps; every exit is
// workgroup-uniform (pivots are read from one LDS word by all); every shuffle is executed by all
// lanes of its wave.  Plain FP64 FMAs.
#include "batch_fitc_tall_shared.h"
#include "batch_fitc_tall_va.h"
#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

constexpr int kTallNVec = 9, kTallCVec = 5, kTallMVec = 10, kTallMMat = 6;

struct Lds {
  double* zs;                              // [m][d]
  double* xs;                              // [ch][d] the chunk's rows of X (passes 1 and 5)
  double *A, *Bf;                          // [ch][ld] the chunk's rows of K / U / V / UP
  double *Lmi, *Lbi;                       // [m][ld] Lm⁻¹, Lb⁻¹ (strict upper triangle zero)
  double *P, *PL, *S, *SL;                 // [m][ld] K̃mm → P → G_Km; P Lb⁻¹; S; S Lm⁻¹
  double* cv[kTallCVec];                   // [ch] the chunk's weights / n-vector entries
  double *b, *beta, *c, *tv, *tw, *wh, *pivm, *pivb, *wv, *lc;   // [m]
  double* sh;                              // block_sum scratch, FG·16
  double* th;                              // θ, then 1/ℓ_k at th + 20
  int ld;
};

struct Ws {                                // this problem's slice of the device workspace
  double *V, *U;                           // [n][ld]; U's array holds K until pass 2
  double *lam, *alpha, *dinv, *r, *w1, *w2, *v, *h, *md;   // [n]
};

__device__ __forceinline__ Lds carve(double* sm, int n, int m, int d) {
  Lds s;
  s.ld = odd_ld(m);
  const int ch = chunk_rows(n);
  double* p = sm;
  auto take = [&p](int k) { double* q = p; p += k; return q; };
  s.zs = take(m * d);
  s.xs = take(ch * d);
  s.A = take(ch * s.ld); s.Bf = take(ch * s.ld);
  s.Lmi = take(m * s.ld); s.Lbi = take(m * s.ld);
  s.P = take(m * s.ld); s.PL = take(m * s.ld); s.S = take(m * s.ld); s.SL = take(m * s.ld);
  for (int q = 0; q < kTallCVec; ++q) s.cv[q] = take(ch);
  s.b = take(m); s.beta = take(m); s.c = take(m); s.tv = take(m); s.tw = take(m);
  s.wh = take(m); s.pivm = take(m); s.pivb = take(m); s.wv = take(m); s.lc = take(m);
  s.sh = take(FG * 16);
  s.th = take(kThDoubles);
  return s;
}

__device__ __forceinline__ Ws carve_ws(double* w, int n, int ld) {
  Ws s;
  double* p = w;
  auto take = [&p](int64_t k) { double* q = p; p += k; return q; };
  s.V = take((int64_t)n * ld); s.U = take((int64_t)n * ld);
  s.lam = take(n); s.alpha = take(n); s.dinv = take(n); s.r = take(n); s.w1 = take(n);
  s.w2 = take(n); s.v = take(n); s.h = take(n); s.md = take(n);
  return s;
}

// Passes 1 and 2: K̃mm, Lm⁻¹, K, V, λ, B, b, Lb⁻¹, c, U, r, d, α, the objectives and, with
// `objective` >= 0, the score derivatives (h, u/λ, h/λ², NLML's v) and Uᵀ(u/λ) in s.tv.  Returns
// 0, k (K̃mm's leading minor of order k is not > 0) or m + k (B's) — the same value in every
// thread.  Call with θ's sf2 / sn2 / 1/ℓ and Z visible; ends synchronised.
__device__ __forceinline__ int forward(const Lds& s, const Ws& w, const double* __restrict__ x,
                                       const double* __restrict__ y, int n, int m, int d,
                                       double sf2, double sn2, int objective,
                                       double obj[GPS_N_OBJ]) {
  const int t = threadIdx.x, ld = s.ld;
  const double* il = s.th + 20;
  for (int e = t; e < m * m; e += FT) {
    const int j = e / m, l = e - j * m;
    double r2 = 0.0;
    for (int k = 0; k < d; ++k) {
      const double df = (s.zs[j * d + k] - s.zs[l * d + k]) * il[k];
      r2 = fma(df, df, r2);
    }
    const double kv = sf2 * exp(-0.5 * r2) + (j == l ? kJitter : 0.0);
    s.Lmi[j * ld + l] = kv;
    s.P[j * ld + l] = kv;
  }
  __syncthreads();
  int info = chol_inv(s.Lmi, m, ld, s.pivm, s.wv, s.lc);
  if (info) return info;
  // pass 1
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    copy_flat(s.xs, x + (int64_t)c0 * d, rows * d);
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {
      const int i = e / m, l = e - i * m;
      const double* xr = s.xs + i * d;
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (xr[k] - s.zs[l * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      s.A[i * ld + l] = sf2 * exp(-0.5 * r2);
    }
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {  // V = K Lm⁻ᵀ
      const int i = e / m, a = e - i * m;
      double acc = 0.0;
#pragma unroll 4
      for (int l = 0; l <= a; ++l) acc = fma(s.A[i * ld + l], s.Lmi[a * ld + l], acc);
      s.Bf[i * ld + a] = acc;
    }
    store_rows(w.U, s.A, c0, rows, ld);
    __syncthreads();
    store_rows(w.V, s.Bf, c0, rows, ld);
    if (t < rows) {
      double q = 0.0;
      for (int a = 0; a < m; ++a) q = fma(s.Bf[t * ld + a], s.Bf[t * ld + a], q);
      const double lam = sf2 - q + sn2;
      w.lam[c0 + t] = lam;
      s.cv[0][t] = 1.0 / lam;
      s.cv[1][t] = y[c0 + t] / lam;
    }
    __syncthreads();
    wgram_acc(s.A, ld, s.cv[0], rows, m, s.P, s.Lbi, ld, c0 == 0);  // B = K̃mm + KᵀΛ⁻¹K
    tmatvec_acc(s.A, ld, s.cv[1], rows, m, s.b, c0 == 0);           // b = KᵀΛ⁻¹y
    __syncthreads();
  }
  info = chol_inv(s.Lbi, m, ld, s.pivb, s.wv, s.lc);
  if (info) return m + info;
  if (t < m) {
    double a = 0.0;
    for (int l = 0; l <= t; ++l) a = fma(s.Lbi[t * ld + l], s.b[l], a);
    s.beta[t] = a;
  }
  __syncthreads();
  if (t < m) {
    double a = 0.0;
    for (int q = t; q < m; ++q) a = fma(s.Lbi[q * ld + t], s.beta[q], a);
    s.c[t] = a;
  }
  __syncthreads();
  // pass 2.  Σ crps, Σ logs, Σ log λ, Σ y²/λ, b·c, Σ log (Lb_kk / Lm_kk): thread t < CH sums rows
  // t, t + CH, ... in order, then block_sum's tree
  const bool grad = objective >= 0, loo = objective != GPS_OBJ_NLML;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    load_rows(s.A, w.U, c0, rows, ld);  // K
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {  // U = K Lb⁻ᵀ
      const int i = e / m, a = e - i * m;
      double acc = 0.0;
#pragma unroll 4
      for (int l = 0; l <= a; ++l) acc = fma(s.A[i * ld + l], s.Lbi[a * ld + l], acc);
      s.Bf[i * ld + a] = acc;
    }
    __syncthreads();
    store_rows(w.U, s.Bf, c0, rows, ld);
    if (t < rows) {
      const int row = c0 + t;
      double g = 0.0, r = 0.0;
      for (int l = 0; l < m; ++l) g = fma(s.A[t * ld + l], s.c[l], g);
      for (int a = 0; a < m; ++a) r = fma(s.Bf[t * ld + a], s.Bf[t * ld + a], r);
      const double lam = w.lam[row], yy = y[row];
      const double dinv = 1.0 / lam - r / (lam * lam);
      const double al = (yy - g) / lam;
      w.r[row] = r;
      w.dinv[row] = dinv;
      w.alpha[row] = al;
      const double mu = yy - al / dinv, cv = 1.0 / dinv;
      v[0] += crps_term(mu, cv, yy);
      v[1] += logs_term(mu, cv, yy);
      v[2] += log(lam);
      v[3] += yy * yy / lam;
      if (grad) {  // score_derivs of the MEAN score, then u and h = c̃ (kernels_grad.hip)
        double h = 0.0;
        if (loo) {
          const double rr = yy - mu;
          double gm, gc;
          if (objective == GPS_OBJ_LOO_CRPS) {
            const double sd = sqrt(cv), z = rr / sd;
            const double cdf = 0.5 * (1.0 + erf(z * 0.70710678118654752440));
            const double pdf = 0.39894228040143267794 * exp(-0.5 * z * z);
            gm = 1.0 - 2.0 * cdf;
            gc = (2.0 * pdf - 0.56418958354775628695) / (2.0 * sd);
          } else {
            gm = -rr / cv;
            gc = 0.5 / cv - rr * rr / (2.0 * cv * cv);
          }
          gm /= n;
          gc /= n;
          h = (gm * al - gc) / (dinv * dinv);
          const double ul = (-gm / dinv) / lam;  // u/λ
          w.w1[row] = ul;
          s.cv[0][t] = ul;
        } else {
          w.v[row] = 0.5 * al;
        }
        w.h[row] = h;
        w.w2[row] = h / (lam * lam);
      }
    }
    __syncthreads();
    if (grad && loo) tmatvec_acc(s.Bf, ld, s.cv[0], rows, m, s.tv, c0 == 0);  // Uᵀ(u/λ)
    __syncthreads();
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

// Passes 3 to 5, after forward(..., objective >= 0): g = [ΣG_K∘K + ΣG_Km∘K(Z,Z), ΣM_ii, the
// per-dimension ∂/∂log ℓ_k sums], valid in every thread; gz[k] = ∂/∂z_jk, valid in the first lane
// (c == 0) of column group j < m, whose column and lane the caller gets in (*col, *lane0).  Ends
// synchronised.
__device__ __forceinline__ void gradient(const Lds& s, const Ws& w, const double* __restrict__ x,
                                         int n, int m, int d, int objective, double sf2,
                                         double (&g)[FG], double (&gz)[GPS_BATCH_MAX_D], int* col,
                                         bool* lane0) {
  const int t = threadIdx.x, ld = s.ld;
  const double* il = s.th + 20;
  const bool loo = objective != GPS_OBJ_NLML;
  const double ac = loo ? 0.0 : 0.5;
  // pass 3: v = C⁻¹u = u/λ − U(Uᵀ(u/λ))/λ (LOO), P = Uᵀdiag(h/λ²)U, Vᵀv
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    copy_flat2(s.A, w.U + (int64_t)c0 * ld, s.Bf, w.V + (int64_t)c0 * ld, rows * ld);
    __syncthreads();
    if (t < rows) {
      const int row = c0 + t;
      double vv;
      if (loo) {
        double a = 0.0;
        for (int q = 0; q < m; ++q) a = fma(s.A[t * ld + q], s.tv[q], a);
        vv = w.w1[row] - a / w.lam[row];
        w.v[row] = vv;
      } else {
        vv = w.v[row];
      }
      s.cv[0][t] = w.w2[row];
      s.cv[1][t] = vv;
    }
    __syncthreads();
    wgram_acc(s.A, ld, s.cv[0], rows, m, nullptr, s.P, ld, c0 == 0);
    tmatvec_acc(s.Bf, ld, s.cv[1], rows, m, s.tw, c0 == 0);
    __syncthreads();
  }
  for (int e = t; e < m * m; e += FT) {  // PL = P Lb⁻¹
    const int a = e / m, l = e - a * m;
    double acc = 0.0;
    for (int q = l; q < m; ++q) acc = fma(s.P[a * ld + q], s.Lbi[q * ld + l], acc);
    s.PL[a * ld + l] = acc;
  }
  // pass 4: (UP)_i·U_i, M_ii, S = Vᵀdiag(M_ii)V, ΣM_ii (thread t < CH: rows t, t + CH, ...)
  double msum = 0.0;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    load_rows(s.A, w.U, c0, rows, ld);
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {  // UP
      const int i = e / m, a = e - i * m;
      double up = 0.0;
#pragma unroll 4
      for (int b = 0; b < m; ++b) up = fma(s.A[i * ld + b], s.P[b * ld + a], up);
      s.Bf[i * ld + a] = up;
    }
    __syncthreads();
    if (t < rows) {
      const int row = c0 + t;
      double q = 0.0;
      for (int a = 0; a < m; ++a) q = fma(s.Bf[t * ld + a], s.A[t * ld + a], q);
      const double lam = w.lam[row], h = w.h[row], l2 = lam * lam;
      const double md = ac * w.dinv[row] - w.v[row] * w.alpha[row] -
                        (h / l2 - 2.0 * h * w.r[row] / (l2 * lam) + q / l2);
      w.md[row] = md;
      s.cv[0][t] = md;
      msum += md;
    }
    __syncthreads();
    load_rows(s.Bf, w.V, c0, rows, ld);
    __syncthreads();
    wgram_acc(s.Bf, ld, s.cv[0], rows, m, nullptr, s.S, ld, c0 == 0);
    __syncthreads();
  }
  if (t < m) {  // ŵ = Lm⁻ᵀ(Vᵀv)
    double a = 0.0;
    for (int q = t; q < m; ++q) a = fma(s.Lmi[q * ld + t], s.tw[q], a);
    s.wh[t] = a;
  }
  for (int e = t; e < m * m; e += FT) {  // SL = S Lm⁻¹
    const int a = e / m, l = e - a * m;
    double acc = 0.0;
    for (int q = l; q < m; ++q) acc = fma(s.S[a * ld + q], s.Lmi[q * ld + l], acc);
    s.SL[a * ld + l] = acc;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += FT) {  // G_Km, over P (dead)
    const int j = e / m, l = e - j * m;
    double a1 = 0.0, a2 = 0.0;
    for (int q = j; q < m; ++q) {
      a1 = fma(s.Lbi[q * ld + j], fma(ac, s.Lbi[q * ld + l], s.PL[q * ld + l]), a1);
      a2 = fma(s.Lmi[q * ld + j], fma(-ac, s.Lmi[q * ld + l], s.SL[q * ld + l]), a2);
    }
    s.P[j * ld + l] = a1 + a2 + 0.5 * (s.wh[j] * s.c[l] + s.c[j] * s.wh[l]);
  }
  __syncthreads();
  // pass 5, the contraction: column group j, lane c takes rows c, c + C, ... of G_K∘K (CH is a
  // multiple of C, so the chunks do not change that order) and entries c, c + C, ... of row j of
  // G_Km∘K(Z,Z)
  const int C = group_lanes(m), j = t / C, c = t - j * C;
  double g0 = 0.0, gl[GPS_BATCH_MAX_D];
#pragma unroll
  for (int k = 0; k < GPS_BATCH_MAX_D; ++k) {
    gl[k] = 0.0;
    gz[k] = 0.0;
  }
  const double cj = j < m ? s.c[j] : 0.0, wj = j < m ? s.wh[j] : 0.0;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    copy_flat2(s.A, w.U + (int64_t)c0 * ld, s.Bf, w.V + (int64_t)c0 * ld, rows * ld);
    copy_flat(s.xs, x + (int64_t)c0 * d, rows * d);
    if (t < rows) {
      s.cv[0][t] = w.lam[c0 + t];
      s.cv[1][t] = w.h[c0 + t];
      s.cv[2][t] = w.md[c0 + t];
      s.cv[3][t] = w.v[c0 + t];
      s.cv[4][t] = w.alpha[c0 + t];
    }
    __syncthreads();
    if (j < m)
      for (int i = c; i < rows; i += C) {
        const double lam = s.cv[0][i], hi = s.cv[1][i];
        const double s1 = 2.0 * (ac / lam - hi / (lam * lam)), s2 = 2.0 / lam;
        double t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll 4
        for (int a = 0; a < m; ++a) {
          const double u = s.A[i * ld + a];
          t1 = fma(u, s.Lbi[a * ld + j], t1);
          t2 = fma(u, s.PL[a * ld + j], t2);
          t3 = fma(s.Bf[i * ld + a], s.Lmi[a * ld + j], t3);
        }
        const double gk =
            s1 * t1 + s2 * t2 - 2.0 * s.cv[2][i] * t3 - s.cv[3][i] * cj - s.cv[4][i] * wj;
        const double* xr = s.xs + i * d;
        double df[GPS_BATCH_MAX_D];
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
          if (k < d) {
            df[k] = (xr[k] - s.zs[j * d + k]) * il[k];
            r2 = fma(df[k], df[k], r2);
          }
        const double gkk = gk * (sf2 * exp(-0.5 * r2));
        g0 += gkk;
#pragma unroll
        for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
          if (k < d) {
            gl[k] = fma(gkk, df[k] * df[k], gl[k]);
            gz[k] = fma(gkk, df[k], gz[k]);
          }
      }
    __syncthreads();
  }
  if (j < m)
    for (int l = c; l < m; l += C) {
      double r2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = (s.zs[j * d + k] - s.zs[l * d + k]) * il[k];
        r2 = fma(df, df, r2);
      }
      const double gmk = s.P[j * ld + l] * (sf2 * exp(-0.5 * r2));  // K(Z,Z) without the jitter
      g0 += gmk;
#pragma unroll
      for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
        if (k < d) {
          const double df = (s.zs[j * d + k] - s.zs[l * d + k]) * il[k];
          gl[k] = fma(gmk, df * df, gl[k]);
          gz[k] = fma(-2.0 * gmk, df, gz[k]);
        }
    }
#pragma unroll
  for (int k = 0; k < GPS_BATCH_MAX_D; ++k)
    if (k < d) gz[k] = group_sum(gz[k], C) * il[k];
  g[0] = g0;
  g[1] = msum;
#pragma unroll
  for (int k = 0; k < GPS_BATCH_MAX_D; ++k) g[2 + k] = gl[k];
  block_sum_n<FG>(g, 2 + d, s.sh);
  *col = j;
  *lane0 = j < m && c == 0;
}

__global__ __launch_bounds__(FT) void batch_fitc_tall_kernel(BatchFitcTallParams tp) {
  extern __shared__ double sm[];
  const BatchFitcParams& p = tp.b;
  const int n = p.n, m = p.m, d = p.d, t = threadIdx.x;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, n, m, d);
  const Ws w = carve_ws(tp.ws + pb * tp.ws_stride, n, s.ld);
  const double* x = p.x + pb * n * d;
  const double* y = p.y + pb * n;
  double* il = s.th + 20;
  int info = p.info[pb];
  int done = p.steps_done[pb];
  double stale = p.stale[pb];
  for (int e = t; e < m * d; e += FT) s.zs[e] = p.z[pb * m * d + e];
  if (t < nth) s.th[t] = p.theta[pb * nth + t];
  double obj[GPS_N_OBJ];
  // the training steps of this launch, then (do_final) one more forward: the final pass at the
  // final θ and Z, whose noise is the final σ² or, with stale_noise, the σ² the last step's
  // forward used (kernels_batch_fitc.hip)
  const int ntrain = p.mode == BATCH_MODE_GRAD ? 1 : p.nsteps;
  const int neval = ntrain + (p.mode == BATCH_MODE_TRAIN && p.do_final ? 1 : 0);
  double sf2 = 0.0, sn2 = 0.0;
  for (int st = 0; st < neval && info == 0; ++st) {
    const bool fin = st == ntrain;
    __syncthreads();  // θ and Z (loaded, or the previous step's update) are visible
    const double lsn = s.th[nth - 1];
    sf2 = exp(s.th[0]);
    sn2 = exp(fin && p.stale_noise ? stale : lsn);
    const double bq = t < d ? s.th[1 + (p.n_ell == 1 ? 0 : t)] : 0.0;
    if (t < d) il[t] = exp(-bq);  // th + 20: beside θ, never over it
    __syncthreads();
    if (!fin) stale = lsn;
    info = forward(s, w, x, y, n, m, d, sf2, sn2, fin ? -1 : p.objective, obj);
    if (info || fin) break;
    double g[FG], gz[GPS_BATCH_MAX_D];
    int col;
    bool lane0;
    gradient(s, w, x, n, m, d, p.objective, sf2, g, gz, &col, &lane0);
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
  for (int i = 0; i < n; ++i) ysum += y[i];
  const double ymean = ysum / n;
  for (int i = 0; i < n; ++i) yss += (y[i] - ymean) * (y[i] - ymean);
  const double yvar = yss / (n - 1);
  // test rows streamed four at a time, one per wave: lane l < m holds k*_l and hands it round by
  // shuffles; lanes a < 32 form (Lm⁻¹k*)_a, lanes 32 + a (Lb⁻¹k*)_a (rows a >= m count as zero);
  // μ* = k*·c, var* = σ² + sf² − ‖Lm⁻¹k*‖² + ‖Lb⁻¹k*‖²
  const int wave = t >> 6, lane = t & 63;
  const int a = lane & 31;
  const bool hi = lane >= 32;
  const double* Lr = (hi ? s.Lbi : s.Lmi) + (a < m ? a : m - 1) * s.ld;
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
      for (int w4 = 0; w4 < FT / 64; ++w4) acc += s.sh[q * 16 + w4];
      tot[q] = acc;
    }
    scores_store(p, pb, tot);
  }
}

// batch_fitc_tall_kernel plus the validation rows: the same step driver without
// BATCH_MODE_GRAD (the launcher refuses it), a checkpoint between forward() and gradient() at every
// step whose global index is a multiple of va_every, and the final pass's row in front of the test
// rows.  Nothing the fit reads is written by a checkpoint, so θ, Z, the series and every final
// output carry the plain kernel's bits.
__global__ __launch_bounds__(FT) void batch_fitc_tall_va_kernel(BatchFitcTallVaParams vp) {
  extern __shared__ double sm[];
  const BatchFitcParams& p = vp.t.b;
  const BatchVaParams& va = vp.va;
  const int n = p.n, m = p.m, d = p.d, t = threadIdx.x;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, n, m, d);
  const Ws w = carve_ws(vp.t.ws + pb * vp.t.ws_stride, n, s.ld);
  const double* x = p.x + pb * n * d;
  const double* y = p.y + pb * n;
  double* il = s.th + 20;
  int info = p.info[pb];
  int done = p.steps_done[pb];
  double stale = p.stale[pb];
  for (int e = t; e < m * d; e += FT) s.zs[e] = p.z[pb * m * d + e];
  if (t < nth) s.th[t] = p.theta[pb * nth + t];
  double obj[GPS_N_OBJ];
  VaStats ys = {0.0, 0.0, 0.0};
  if (info == 0 && va_launch_scores(p, va.va_every)) ys = va_target_stats(y, n);
  const int64_t nva = va_rows(p.itr, va.va_every);
  int vfrom = p.step0;  // the first step of this launch whose row is not written yet
  const int ntrain = p.nsteps;
  const int neval = ntrain + (p.do_final ? 1 : 0);
  double sf2 = 0.0, sn2 = 0.0;
  for (int st = 0; st < neval && info == 0; ++st) {
    const bool fin = st == ntrain;
    __syncthreads();  // θ and Z (loaded, or the previous step's update) are visible
    const double lsn = s.th[nth - 1];
    sf2 = exp(s.th[0]);
    sn2 = exp(fin && p.stale_noise ? stale : lsn);
    const double bq = t < d ? s.th[1 + (p.n_ell == 1 ? 0 : t)] : 0.0;
    if (t < d) il[t] = exp(-bq);  // th + 20: beside θ, never over it
    __syncthreads();
    if (!fin) stale = lsn;
    info = forward(s, w, x, y, n, m, d, sf2, sn2, fin ? -1 : p.objective, obj);
    if (info || fin) break;
    const int gi = p.step0 + st;
    if (gi % va.va_every == 0) {  // workgroup-uniform
      va_checkpoint(s, va, pb, gi / va.va_every, nva, m, d, sf2, sn2, ys);
      vfrom = gi + 1;
    }
    double g[FG], gz[GPS_BATCH_MAX_D];
    int col;
    bool lane0;
    gradient(s, w, x, n, m, d, p.objective, sf2, g, gz, &col, &lane0);
    const double gn = sn2 * g[1];
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
    ++done;
  }
  __syncthreads();
  train_write_back<FT>(p, pb, t, s.th, s.zs, info, done, stale);
  if (t == 0) p.info[pb] = info;
  va_finish(s, p, va, pb, info, vfrom, sf2, sn2, obj, ys);
}

}  // namespace

size_t batch_fitc_tall_lds_bytes(int n, int m, int d) {
  const int ld = odd_ld(m), ch = chunk_rows(n);
  return (size_t)(m * d + ch * d + 2 * ch * ld + kTallMMat * m * ld + kTallCVec * ch + kTallMVec * m +
                  FG * 16 + kThDoubles) * sizeof(double);
}

int64_t batch_fitc_tall_ws_doubles(int64_t n, int m) {
  return 2 * n * odd_ld(m) + kTallNVec * n;
}

int batch_fitc_tall_steps(int64_t n) {
  const int64_t chunks = (n + kBatchFitcTallChunk - 1) / kBatchFitcTallChunk;
  const int64_t k = kBatchStepsPerLaunch / (chunks < 1 ? 1 : chunks);
  return (int)(k < 1 ? 1 : k);
}

hipError_t launch_batch_fitc_tall(const BatchFitcTallParams& tp, hipStream_t s) {
  const BatchFitcParams& p = tp.b;
  if (p.n < 1 || p.n > GPS_BATCH_FITC_TALL_MAX_N || p.m < 1 || p.m > GPS_BATCH_FITC_MAX_M ||
      p.d < 1 || p.d > GPS_BATCH_MAX_D || p.nprob < 1 || (p.n_ell != 1 && p.n_ell != p.d) ||
      p.nsteps < 0 || p.nsteps > batch_fitc_tall_steps(p.n) || !tp.ws ||
      tp.ws_stride < batch_fitc_tall_ws_doubles(p.n, p.m))
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds(
      (const void*)batch_fitc_tall_kernel,
      batch_fitc_tall_lds_bytes(GPS_BATCH_FITC_TALL_MAX_N, GPS_BATCH_FITC_MAX_M, GPS_BATCH_MAX_D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_fitc_tall_kernel, dim3((unsigned)p.nprob), dim3(FT),
                     batch_fitc_tall_lds_bytes(p.n, p.m, p.d), s, tp);
  return hipGetLastError();
}

int batch_fitc_tall_va_steps(int64_t n, int64_t nv, int64_t va_every) {
  const int64_t plain = batch_fitc_tall_steps(n);
  const int64_t k = kBatchFitcVaRowBudget / (nv < 1 ? 1 : nv) * (va_every < 1 ? 1 : va_every);
  return (int)(k < 1 ? 1 : (k < plain ? k : plain));
}

hipError_t launch_batch_fitc_tall_va(const BatchFitcTallVaParams& vp, hipStream_t s) {
  const BatchFitcParams& p = vp.t.b;
  const BatchVaParams& va = vp.va;
  if (p.mode != BATCH_MODE_TRAIN || !va.xv || !va.yv || !va.va_sc || va.nv < 1 ||
      va.va_every < 1 || p.n < 1 || p.n > GPS_BATCH_FITC_TALL_MAX_N || p.m < 1 ||
      p.m > GPS_BATCH_FITC_MAX_M || p.d < 1 || p.d > GPS_BATCH_MAX_D || p.nprob < 1 ||
      (p.n_ell != 1 && p.n_ell != p.d) || p.nsteps < 0 ||
      p.nsteps > batch_fitc_tall_va_steps(p.n, va.nv, va.va_every) || p.step0 < 0 ||
      (int64_t)p.step0 + p.nsteps > p.itr || !vp.t.ws ||
      vp.t.ws_stride < batch_fitc_tall_ws_doubles(p.n, p.m))
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds(
      (const void*)batch_fitc_tall_va_kernel,
      batch_fitc_tall_lds_bytes(GPS_BATCH_FITC_TALL_MAX_N, GPS_BATCH_FITC_MAX_M, GPS_BATCH_MAX_D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_fitc_tall_va_kernel, dim3((unsigned)p.nprob), dim3(FT),
                     batch_fitc_tall_lds_bytes(p.n, p.m, p.d), s, vp);
  return hipGetLastError();
}

}  // namespace gps
