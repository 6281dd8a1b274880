// Batches of tall FITC GPs on the block-LOO objectives GPS_BLOCK_DSS and GPS_BLOCK_KC (K20:523-593,
// K20:655-726), one workgroup of 256 threads per problem: kernels_batch_fitc_tall.hip's sibling
// (DESIGN §27).  Same model, limits, chunking and step driver; the objective is fast_fitc_blockloo
// of oracle/gp_oracle.py with the fold covariance C_f = Λ_f + W_f W_fᵀ never formed.
//
// Folds are [⌊f·n/k⌋, ⌊(f+1)·n/k⌋), of b_f rows each.  With K = K(X,Z), V = K Lm⁻ᵀ, λ, B = K̃mm +
// Σ_f part_f (part_f = K_fᵀΛ_f⁻¹K_f), Ũ = Λ⁻¹K Lb⁻ᵀ (the workspace's U holds Ũ, the oracle's
// scaling) and α as §22 forms them, each fold has
//   B₋f = K̃mm + Σ_{g≠f} part_g (summed, never subtracted), L₋f⁻¹ by chol_inv, W = K_f L₋f⁻ᵀ,
//   r = λ∘α_f + W(Wᵀα_f),  c = λ + rowsum(W∘W),  log|C_f| = Σ_f log λ + log|B| − log|B₋f|
//   DSS  ½b_f log2π + ½log|C_f| + ½α_fᵀr;   F̃ = −½(CŨ + r(rᵀŨ)), diag G = −½(c + r²), g = r
//   KC   mean crps(y_f − r, c, y_f), (gm, gc) its derivatives, w = C gm, D = diag(gc):
//        F̃ = ½(w(rᵀŨ) + r(wᵀŨ)) − C(D·CŨ),  g = −w,
//        diag G = w∘r − [λ²gc + 2λgc(c − λ) + rowdot(W(WᵀDW), W)]
// where CX = λ∘X + W(WᵀX) and WᵀD(CŨ) = Wᵀdiag(gc∘λ)Ũ + (WᵀDW)(WᵀŨ) keep a fold at O(b·m²).
// The passes over chunks of kBatchFitcTallChunk rows (a fold's chunks count from its first row):
//   1   per fold: K → V → λ, part_f, b; K, V to the workspace; B summed in fold order
//   2   U = K Lb⁻ᵀ, r, d, α, the five pointwise objectives; Ũ to the workspace
//   per fold, after L₋f⁻¹:
//   f1  W (kept in F's rows of the fold), Wᵀα
//   f2  r, c, the value terms, WᵀŨ, rᵀŨ; KC: gm, gc, Wᵀgm, WᵀDW, Wᵀdiag(gcλ)Ũ
//   f3  KC: w, wᵀŨ
//   f4  F̃ over W's rows, diag G, g; S̃ += ŨᵀF̃, Ũᵀg
//   3   v = g/λ − Ũ(Ũᵀg), Vᵀv
//   4   H = −2Λ⁻¹F̃ + 2ŨS̃ over F̃, M_ii, S = Vᵀdiag(M_ii)V
//   5   G_K = H Lb⁻¹ − 2diag(M_ii)V Lm⁻¹ − v cᵀ − α ŵᵀ contracted with ∂K/∂θ, ∂K/∂z on the spot
// Reductions, ordering and exits are §22's: a column or an m×m entry is owned by the same lanes in
// every chunk, chunks add in ascending order, folds in ascending order, so every sum's order is a
// function of (n, m, d, nfold) and the 256 threads only; no atomics; __syncthreads() is the only
// ordering; every exit is workgroup-uniform; every shuffle is executed by all lanes of its wave.
// The chunk helpers are batch_fitc_tall_shared.h's; the step driver in the __global__ function is
// kernels_batch_fitc_tall.hip's text, copied (§27 says what was shared and what was not).
#include "batch_fitc_tall_shared.h"
#include "batch_fitc_tall_va.h"

namespace gps {

namespace {

static_assert(FT == 2 * CH, "row_quad gives a chunk row two threads");

constexpr int kBlkNVec = 11, kBlkCVec = 5, kBlkMVec = 15, kBlkMMat = 7, kBlkNMat = 4;

struct Lds {
  double* zs;                              // [m][d]
  double* xs;                              // [ch][d] the chunk's rows of X (passes 1 and 5)
  double *A, *Bf;                          // [ch][ld] the chunk's rows of two workspace matrices
  double *Lmi, *Lbi;                       // [m][ld] Lm⁻¹, Lb⁻¹ (strict upper triangle zero)
  double *P, *PL, *S, *SL, *Q;             // [m][ld] folds: L₋f⁻¹, WᵀŨ, WᵀDW, S̃, Wᵀdiag(gcλ)Ũ
  double* cv[kBlkCVec];                    // [ch] the chunk's weights / n-vector entries
  double *b, *beta, *c, *ug, *tw, *wh, *pivm, *pivb, *wv, *lc, *wa, *ru, *wgm, *wu, *pivf;  // [m]
  double* sh;                              // block_sum scratch, FG·16
  double* th;                              // θ, then 1/ℓ_k at th + 20
  int ld;
};

struct Ws {                                // this problem's slice of the device workspace
  double *K, *V, *U, *F;                   // [n][ld]: K, V, Ũ, and W_f → F̃ → H
  double* part;                            // [nfold + 1][m][ld] part_f, then K̃mm
  double *lam, *alpha, *r, *cc, *gm, *gc, *w, *gd, *g, *v, *md;   // [n]
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
  s.Q = take(m * s.ld);
  for (int q = 0; q < kBlkCVec; ++q) s.cv[q] = take(ch);
  s.b = take(m); s.beta = take(m); s.c = take(m); s.ug = take(m); s.tw = take(m);
  s.wh = take(m); s.pivm = take(m); s.pivb = take(m); s.wv = take(m); s.lc = take(m);
  s.wa = take(m); s.ru = take(m); s.wgm = take(m); s.wu = take(m); s.pivf = take(m);
  s.sh = take(FG * 16);
  s.th = take(kThDoubles);
  return s;
}

__device__ __forceinline__ Ws carve_ws(double* w, int n, int m, int ld, int nfold) {
  Ws s;
  double* p = w;
  auto take = [&p](int64_t k) { double* q = p; p += k; return q; };
  s.K = take((int64_t)n * ld); s.V = take((int64_t)n * ld);
  s.U = take((int64_t)n * ld); s.F = take((int64_t)n * ld);
  s.part = take((int64_t)(nfold + 1) * m * ld);
  s.lam = take(n); s.alpha = take(n); s.r = take(n); s.cc = take(n); s.gm = take(n);
  s.gc = take(n); s.w = take(n); s.gd = take(n); s.g = take(n); s.v = take(n); s.md = take(n);
  return s;
}

// wgram_acc's two-array sibling: out[j][l] (+)= Σ_i A[i][j]·B[i][l]·w[i] (WEIGHT) or Σ_i A[i][j]·
// B[i][l] over the chunk's rows, the same lanes and the same order
template <bool WEIGHT>
__device__ __forceinline__ void wgram2_acc(const double* A, const double* B, int lda,
                                           const double* w, int rows, int m, double* out, int ldm,
                                           bool first) {
  const int ne = m * m;
  const int C = ne <= FT / 2 ? group_lanes(ne) : 1, G = FT / C;
  const int g = threadIdx.x / C, c = threadIdx.x - g * C;
  for (int e0 = 0; e0 < ne; e0 += G) {
    const int e = e0 + g;
    const bool on = e < ne;
    const int j = on ? e / m : 0, l = on ? e - j * m : 0;
    double a = 0.0;
    if (on) {
      if (WEIGHT) {
#pragma unroll 8
        for (int i = c; i < rows; i += C) a = fma(A[i * lda + j] * B[i * lda + l], w[i], a);
      } else {
#pragma unroll 8
        for (int i = c; i < rows; i += C) a = fma(A[i * lda + j], B[i * lda + l], a);
      }
    }
    a = group_sum(a, C);
    if (on && c == 0) out[j * ldm + l] = first ? a : out[j * ldm + l] + a;
  }
}

// the two halves of A_i T A_iᵀ for the chunk's rows: thread t takes row t mod CH and the rows b =
// t / CH, t / CH + 2, ... of T; o0[i] + o1[i] is the form
__device__ __forceinline__ void row_quad(const double* A, int lda, const double* T, int ldm,
                                         int rows, int m, double* o0, double* o1) {
  const int i = threadIdx.x & (CH - 1), h = threadIdx.x / CH;
  if (i < rows) {
    double acc = 0.0;
    for (int b = h; b < m; b += 2) {
      double in = 0.0;
#pragma unroll 4
      for (int a = 0; a < m; ++a) in = fma(T[b * ldm + a], A[i * lda + a], in);
      acc = fma(A[i * lda + b], in, acc);
    }
    (h ? o1 : o0)[i] = acc;
  }
}

// Passes 1 and 2: K̃mm, Lm⁻¹, K, V, λ, the folds' partials, B, b, Lb⁻¹, c, Ũ, α and the five
// pointwise objectives.  Returns 0, k (K̃mm's leading minor of order k is not > 0) or m + k (B's) —
// the same value in every thread.  Call with θ's sf2 / sn2 / 1/ℓ and Z visible; ends synchronised.
__device__ __forceinline__ int forward(const Lds& s, const Ws& w, const double* __restrict__ x,
                                       const double* __restrict__ y, int n, int m, int d,
                                       int nfold, double sf2, double sn2, double obj[GPS_N_OBJ]) {
  const int t = threadIdx.x, ld = s.ld, mld = m * ld;
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
    w.part[(int64_t)nfold * mld + j * ld + l] = kv;
  }
  __syncthreads();
  int info = chol_inv(s.Lmi, m, ld, s.pivm, s.wv, s.lc);
  if (info) return info;
  // pass 1, fold by fold
  for (int f = 0; f < nfold; ++f) {
    const int fa = fold_begin(f, n, nfold), fb = fold_begin(f + 1, n, nfold);
    for (int c0 = fa; c0 < fb; c0 += CH) {
      const int rows = fb - c0 < CH ? fb - c0 : CH;
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
      store_rows(w.K, s.A, c0, rows, ld);
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
      wgram_acc(s.A, ld, s.cv[0], rows, m, nullptr, s.Q, ld, c0 == fa);  // part_f = K_fᵀΛ_f⁻¹K_f
      tmatvec_acc(s.A, ld, s.cv[1], rows, m, s.b, c0 == 0);              // b = KᵀΛ⁻¹y
      __syncthreads();
    }
    for (int e = t; e < m * m; e += FT) {  // B = K̃mm + Σ_f part_f, in fold order
      const int j = e / m, l = e - j * m;
      const double pv = s.Q[j * ld + l];
      w.part[(int64_t)f * mld + j * ld + l] = pv;
      s.Lbi[j * ld + l] = (f == 0 ? s.P[j * ld + l] : s.Lbi[j * ld + l]) + pv;
    }
  }
  __syncthreads();
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
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    load_rows(s.A, w.K, c0, rows, ld);
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {  // U = K Lb⁻ᵀ
      const int i = e / m, a = e - i * m;
      double acc = 0.0;
#pragma unroll 4
      for (int l = 0; l <= a; ++l) acc = fma(s.A[i * ld + l], s.Lbi[a * ld + l], acc);
      s.Bf[i * ld + a] = acc;
    }
    __syncthreads();
    if (t < rows) {
      const int row = c0 + t;
      double g = 0.0, r = 0.0;
      for (int l = 0; l < m; ++l) g = fma(s.A[t * ld + l], s.c[l], g);
      for (int a = 0; a < m; ++a) r = fma(s.Bf[t * ld + a], s.Bf[t * ld + a], r);
      const double lam = w.lam[row], yy = y[row];
      const double dinv = 1.0 / lam - r / (lam * lam);
      const double al = (yy - g) / lam;
      w.alpha[row] = al;
      s.cv[0][t] = lam;
      const double mu = yy - al / dinv, cv = 1.0 / dinv;
      v[0] += crps_term(mu, cv, yy);
      v[1] += logs_term(mu, cv, yy);
      v[2] += log(lam);
      v[3] += yy * yy / lam;
    }
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {  // Ũ = Λ⁻¹U
      const int i = e / m, a = e - i * m;
      s.Bf[i * ld + a] /= s.cv[0][i];
    }
    __syncthreads();
    store_rows(w.U, s.Bf, c0, rows, ld);
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

// The fold passes and passes 3 to 5, after forward(): the block objective in `value` (each fold's
// term to fold_values where given), g = [ΣG_K∘K + ΣG_Km∘K(Z,Z), ΣM_ii, the per-dimension ∂/∂log ℓ_k
// sums], valid in every thread; gz[k] = ∂/∂z_jk, valid in the first lane (c == 0) of column group
// j < m, whose column and lane the caller gets in (*col, *lane0).  Returns 0 or (2 + f)·m + k: the
// leading minor of order k of fold f's B₋f is not > 0 — the same value in every thread.  Ends
// synchronised.
__device__ __forceinline__ int block_gradient(const Lds& s, const Ws& w,
                                              const double* __restrict__ x,
                                              const double* __restrict__ y, int n, int m, int d,
                                              int objective, int nfold, double sf2, double& value,
                                              double* fold_values, double (&g)[FG],
                                              double (&gz)[GPS_BATCH_MAX_D], int* col,
                                              bool* lane0) {
  const int t = threadIdx.x, ld = s.ld, mld = m * ld;
  const double* il = s.th + 20;
  const bool kc = objective == GPS_BLOCK_KC;
  value = 0.0;
  for (int f = 0; f < nfold; ++f) {
    const int fa = fold_begin(f, n, nfold), fb = fold_begin(f + 1, n, nfold), bs = fb - fa;
    for (int e = t; e < m * m; e += FT) {  // B₋f = K̃mm + Σ_{g≠f} part_g, in fold order
      const int j = e / m, l = e - j * m;
      double acc = w.part[(int64_t)nfold * mld + j * ld + l];
      for (int q = 0; q < nfold; ++q)
        if (q != f) acc += w.part[(int64_t)q * mld + j * ld + l];
      s.P[j * ld + l] = acc;
    }
    __syncthreads();
    const int bad = chol_inv(s.P, m, ld, s.pivf, s.wv, s.lc);
    if (bad) return (2 + f) * m + bad;
    // f1: W = K_f L₋f⁻ᵀ into F's rows of the fold, Wᵀα_f
    for (int c0 = fa; c0 < fb; c0 += CH) {
      const int rows = fb - c0 < CH ? fb - c0 : CH;
      load_rows(s.A, w.K, c0, rows, ld);
      if (t < rows) s.cv[0][t] = w.alpha[c0 + t];
      __syncthreads();
      for (int e = t; e < rows * m; e += FT) {
        const int i = e / m, a = e - i * m;
        double acc = 0.0;
#pragma unroll 4
        for (int l = 0; l <= a; ++l) acc = fma(s.A[i * ld + l], s.P[a * ld + l], acc);
        s.Bf[i * ld + a] = acc;
      }
      __syncthreads();
      store_rows(w.F, s.Bf, c0, rows, ld);
      tmatvec_acc(s.Bf, ld, s.cv[0], rows, m, s.wa, c0 == fa);
      __syncthreads();
    }
    // f2: r, c, the fold's value terms; WᵀŨ, rᵀŨ; KC: gm, gc, Wᵀgm, WᵀDW, Wᵀdiag(gcλ)Ũ
    double vs0 = 0.0, vs1 = 0.0;  // this thread's rows: Σ crps, or Σ log λ and Σ α·r
    for (int c0 = fa; c0 < fb; c0 += CH) {
      const int rows = fb - c0 < CH ? fb - c0 : CH;
      const bool first = c0 == fa;
      copy_flat2(s.A, w.F + (int64_t)c0 * ld, s.Bf, w.U + (int64_t)c0 * ld, rows * ld);
      __syncthreads();
      if (t < rows) {
        const int row = c0 + t;
        const double lam = w.lam[row], al = w.alpha[row];
        double wr = 0.0, ww = 0.0;
        for (int a = 0; a < m; ++a) {
          const double wi = s.A[t * ld + a];
          wr = fma(wi, s.wa[a], wr);
          ww = fma(wi, wi, ww);
        }
        const double r = lam * al + wr, c = lam + ww;
        w.r[row] = r;
        w.cc[row] = c;
        s.cv[0][t] = r;
        if (kc) {
          const double yy = y[row];
          const double sd = sqrt(c), z = r / sd;
          const double cdf = 0.5 * (1.0 + erf(z * 0.70710678118654752440));
          const double pdf = 0.39894228040143267794 * exp(-0.5 * z * z);
          const double gm = (1.0 - 2.0 * cdf) / bs;
          const double gc = (2.0 * pdf - 0.56418958354775628695) / (2.0 * sd) / bs;
          vs0 += crps_term(yy - r, c, yy);
          w.gm[row] = gm;
          w.gc[row] = gc;
          s.cv[1][t] = gm;
          s.cv[2][t] = gc;
          s.cv[3][t] = gc * lam;
        } else {
          vs0 += log(lam);
          vs1 = fma(al, r, vs1);
        }
      }
      __syncthreads();
      wgram2_acc<false>(s.A, s.Bf, ld, nullptr, rows, m, s.PL, ld, first);  // WᵀŨ
      tmatvec_acc(s.Bf, ld, s.cv[0], rows, m, s.ru, first);                 // rᵀŨ
      if (kc) {
        tmatvec_acc(s.A, ld, s.cv[1], rows, m, s.wgm, first);                       // Wᵀgm
        wgram_acc(s.A, ld, s.cv[2], rows, m, nullptr, s.S, ld, first);              // WᵀDW
        wgram2_acc<true>(s.A, s.Bf, ld, s.cv[3], rows, m, s.Q, ld, first);          // Wᵀdiag(gcλ)Ũ
      }
      __syncthreads();
    }
    // the third sum is ½(log|B| − log|B₋f|)
    double vs[3] = {vs0, vs1, t < m ? log(s.pivb[t]) - log(s.pivf[t]) : 0.0};
    block_sum_n<3>(vs, 3, s.sh);
    const double fv = kc ? vs[0] / bs
                         : 0.5 * bs * 1.83787706640934548356 + 0.5 * (vs[0] + 2.0 * vs[2]) +
                               0.5 * vs[1];
    if (kc) {
      // f3: w = C gm, wᵀŨ
      for (int c0 = fa; c0 < fb; c0 += CH) {
        const int rows = fb - c0 < CH ? fb - c0 : CH;
        copy_flat2(s.A, w.F + (int64_t)c0 * ld, s.Bf, w.U + (int64_t)c0 * ld, rows * ld);
        __syncthreads();
        if (t < rows) {
          const int row = c0 + t;
          double a = 0.0;
          for (int q = 0; q < m; ++q) a = fma(s.A[t * ld + q], s.wgm[q], a);
          const double wi = fma(w.lam[row], w.gm[row], a);
          w.w[row] = wi;
          s.cv[0][t] = wi;
        }
        __syncthreads();
        tmatvec_acc(s.Bf, ld, s.cv[0], rows, m, s.wu, c0 == fa);
        __syncthreads();
      }
      for (int e = t; e < m * m; e += FT) {  // WᵀD(CŨ) = Wᵀdiag(gcλ)Ũ + (WᵀDW)(WᵀŨ), over Q
        const int j = e / m, l = e - j * m;
        double acc = s.Q[j * ld + l];
        for (int q = 0; q < m; ++q) acc = fma(s.S[j * ld + q], s.PL[q * ld + l], acc);
        s.Q[j * ld + l] = acc;
      }
      __syncthreads();
    }
    // f4: F̃'s rows over W's, diag G_f, g_f; S̃ += ŨᵀF̃, Ũᵀg
    for (int c0 = fa; c0 < fb; c0 += CH) {
      const int rows = fb - c0 < CH ? fb - c0 : CH;
      const bool first = f == 0 && c0 == fa;
      copy_flat2(s.A, w.F + (int64_t)c0 * ld, s.Bf, w.U + (int64_t)c0 * ld, rows * ld);
      if (t < rows) {
        s.cv[0][t] = w.lam[c0 + t];
        s.cv[1][t] = w.r[c0 + t];
        if (kc) {
          s.cv[2][t] = w.gc[c0 + t];
          s.cv[3][t] = w.w[c0 + t];
        }
      }
      __syncthreads();
      if (kc) row_quad(s.A, ld, s.S, ld, rows, m, s.cv[4], s.xs);
      for (int e = t; e < rows * m; e += FT) {
        const int i = e / m, a = e - i * m;
        const double lam = s.cv[0][i], r = s.cv[1][i];
        double wt1 = 0.0;
#pragma unroll 4
        for (int b = 0; b < m; ++b) wt1 = fma(s.A[i * ld + b], s.PL[b * ld + a], wt1);
        const double cu = fma(lam, s.Bf[i * ld + a], wt1);  // (CŨ)_ia
        double fv2;
        if (kc) {
          double wt3 = 0.0;
#pragma unroll 4
          for (int b = 0; b < m; ++b) wt3 = fma(s.A[i * ld + b], s.Q[b * ld + a], wt3);
          fv2 = 0.5 * (s.cv[3][i] * s.ru[a] + r * s.wu[a]) - fma(lam * s.cv[2][i], cu, wt3);
        } else {
          fv2 = -0.5 * fma(r, s.ru[a], cu);
        }
        s.Bf[i * ld + a] = fv2;
      }
      __syncthreads();
      store_rows(w.F, s.Bf, c0, rows, ld);
      double gi = 0.0;
      if (t < rows) {
        const int row = c0 + t;
        const double lam = s.cv[0][t], r = s.cv[1][t], c = w.cc[row];
        double gd;
        if (kc) {
          const double gc = s.cv[2][t], wi = s.cv[3][t];
          gd = wi * r - (lam * lam * gc + 2.0 * lam * gc * (c - lam) + (s.cv[4][t] + s.xs[t]));
          gi = -wi;
        } else {
          gd = -0.5 * fma(r, r, c);
          gi = r;
        }
        w.gd[row] = gd;
        w.g[row] = gi;
      }
      __syncthreads();
      load_rows(s.A, w.U, c0, rows, ld);
      if (t < rows) s.cv[0][t] = gi;
      __syncthreads();
      wgram2_acc<false>(s.A, s.Bf, ld, nullptr, rows, m, s.SL, ld, first);  // S̃ += ŨᵀF̃
      tmatvec_acc(s.A, ld, s.cv[0], rows, m, s.ug, first);                  // Ũᵀg
      __syncthreads();
    }
    value += fv;
    if (fold_values && t == 0) fold_values[f] = fv;
  }
  // pass 3: v = g/λ − Ũ(Ũᵀg), Vᵀv
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    copy_flat2(s.A, w.U + (int64_t)c0 * ld, s.Bf, w.V + (int64_t)c0 * ld, rows * ld);
    __syncthreads();
    if (t < rows) {
      const int row = c0 + t;
      double a = 0.0;
      for (int q = 0; q < m; ++q) a = fma(s.A[t * ld + q], s.ug[q], a);
      const double vv = w.g[row] / w.lam[row] - a;
      w.v[row] = vv;
      s.cv[0][t] = vv;
    }
    __syncthreads();
    tmatvec_acc(s.Bf, ld, s.cv[0], rows, m, s.tw, c0 == 0);
    __syncthreads();
  }
  if (t < m) {  // ŵ = Lm⁻ᵀ(Vᵀv)
    double a = 0.0;
    for (int q = t; q < m; ++q) a = fma(s.Lmi[q * ld + t], s.tw[q], a);
    s.wh[t] = a;
  }
  // pass 4: H = −2Λ⁻¹F̃ + 2ŨS̃ over F̃, M_ii, S = Vᵀdiag(M_ii)V, ΣM_ii (thread t < CH: rows t,
  // t + CH, ...).  (ŨS̃)_i·Ũ_i = ½H_i·Ũ_i + F̃_i·Ũ_i/λ_i, so M_ii = −G_ii/λ² + F̃_i·Ũ_i/λ − ½H_i·Ũ_i
  // − v_iα_i
  double msum = 0.0;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int rows = n - c0 < CH ? n - c0 : CH;
    copy_flat2(s.A, w.U + (int64_t)c0 * ld, s.Bf, w.F + (int64_t)c0 * ld, rows * ld);
    if (t < rows) s.cv[0][t] = w.lam[c0 + t];
    __syncthreads();
    double fu = 0.0;
    if (t < rows)
      for (int a = 0; a < m; ++a) fu = fma(s.Bf[t * ld + a], s.A[t * ld + a], fu);
    __syncthreads();
    for (int e = t; e < rows * m; e += FT) {
      const int i = e / m, a = e - i * m;
      double us = 0.0;
#pragma unroll 4
      for (int b = 0; b < m; ++b) us = fma(s.A[i * ld + b], s.SL[b * ld + a], us);
      s.Bf[i * ld + a] = -2.0 * s.Bf[i * ld + a] / s.cv[0][i] + 2.0 * us;
    }
    __syncthreads();
    store_rows(w.F, s.Bf, c0, rows, ld);
    if (t < rows) {
      const int row = c0 + t;
      double hu = 0.0;
      for (int a = 0; a < m; ++a) hu = fma(s.Bf[t * ld + a], s.A[t * ld + a], hu);
      const double lam = s.cv[0][t];
      const double md = -w.gd[row] / (lam * lam) + fu / lam - 0.5 * hu - w.v[row] * w.alpha[row];
      w.md[row] = md;
      s.cv[1][t] = md;
      msum += md;
    }
    __syncthreads();
    load_rows(s.A, w.V, c0, rows, ld);
    __syncthreads();
    wgram_acc(s.A, ld, s.cv[1], rows, m, nullptr, s.S, ld, c0 == 0);
    __syncthreads();
  }
  for (int e = t; e < m * m; e += FT) {  // PL = S̃ Lb⁻¹, Q = S Lm⁻¹
    const int a = e / m, l = e - a * m;
    double a1 = 0.0, a2 = 0.0;
    for (int q = l; q < m; ++q) {
      a1 = fma(s.SL[a * ld + q], s.Lbi[q * ld + l], a1);
      a2 = fma(s.S[a * ld + q], s.Lmi[q * ld + l], a2);
    }
    s.PL[a * ld + l] = a1;
    s.Q[a * ld + l] = a2;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += FT) {  // G_Km, over P (dead)
    const int j = e / m, l = e - j * m;
    double a1 = 0.0, a2 = 0.0;
    for (int q = j; q < m; ++q) {
      a1 = fma(s.Lbi[q * ld + j], s.PL[q * ld + l], a1);
      a2 = fma(s.Lmi[q * ld + j], s.Q[q * ld + l], a2);
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
    copy_flat2(s.A, w.F + (int64_t)c0 * ld, s.Bf, w.V + (int64_t)c0 * ld, rows * ld);
    copy_flat(s.xs, x + (int64_t)c0 * d, rows * d);
    if (t < rows) {
      s.cv[0][t] = w.md[c0 + t];
      s.cv[1][t] = w.v[c0 + t];
      s.cv[2][t] = w.alpha[c0 + t];
    }
    __syncthreads();
    if (j < m)
      for (int i = c; i < rows; i += C) {
        double t1 = 0.0, t3 = 0.0;
#pragma unroll 4
        for (int a = 0; a < m; ++a) {
          t1 = fma(s.A[i * ld + a], s.Lbi[a * ld + j], t1);
          t3 = fma(s.Bf[i * ld + a], s.Lmi[a * ld + j], t3);
        }
        const double gk = t1 - 2.0 * s.cv[0][i] * t3 - s.cv[1][i] * cj - s.cv[2][i] * wj;
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
  return 0;
}

__global__ __launch_bounds__(FT) void batch_fitc_tall_block_kernel(BatchFitcTallBlockParams tp) {
  extern __shared__ double sm[];
  const BatchFitcParams& p = tp.b;
  const int n = p.n, m = p.m, d = p.d, t = threadIdx.x;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, n, m, d);
  const Ws w = carve_ws(tp.ws + pb * tp.ws_stride, n, m, s.ld, tp.nfold);
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
    info = forward(s, w, x, y, n, m, d, tp.nfold, sf2, sn2, obj);
    if (info || fin) break;
    double g[FG], gz[GPS_BATCH_MAX_D], value;
    int col;
    bool lane0;
    info = block_gradient(s, w, x, y, n, m, d, p.objective, tp.nfold, sf2, value,
                          p.mode == BATCH_MODE_GRAD && tp.fold_values
                              ? tp.fold_values + pb * tp.nfold
                              : nullptr,
                          g, gz, &col, &lane0);
    if (info) break;
    const double gn = sn2 * g[1];
    if (p.mode == BATCH_MODE_GRAD) {
      if (t == 0) {
        tp.value[pb] = value;
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
      // every read of θ and Z of this step lies before block_gradient()'s closing barriers
      if (t == 0) {
        const int64_t si = pb * p.itr + p.step0 + st;
        p.values[si] = value;
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
    if (info) {
      if (t == 0) tp.value[pb] = batch_nan();
      if (tp.fold_values && t < tp.nfold) tp.fold_values[pb * tp.nfold + t] = batch_nan();
    }
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

// batch_fitc_tall_block_kernel plus the validation rows, as batch_fitc_tall_va_kernel:
// the checkpoint stands between forward() and block_gradient(), so a fit that fails in its fold
// work after a good forward keeps that step's row (§34's rule).
__global__ __launch_bounds__(FT) void batch_fitc_tall_block_va_kernel(
    BatchFitcTallBlockVaParams vp) {
  extern __shared__ double sm[];
  const BatchFitcTallBlockParams& tp = vp.t;
  const BatchFitcParams& p = tp.b;
  const BatchVaParams& va = vp.va;
  const int n = p.n, m = p.m, d = p.d, t = threadIdx.x;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, n, m, d);
  const Ws w = carve_ws(tp.ws + pb * tp.ws_stride, n, m, s.ld, tp.nfold);
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
    info = forward(s, w, x, y, n, m, d, tp.nfold, sf2, sn2, obj);
    if (info || fin) break;
    const int gi = p.step0 + st;
    if (gi % va.va_every == 0) {  // workgroup-uniform
      va_checkpoint(s, va, pb, gi / va.va_every, nva, m, d, sf2, sn2, ys);
      vfrom = gi + 1;
    }
    double g[FG], gz[GPS_BATCH_MAX_D], value;
    int col;
    bool lane0;
    info = block_gradient(s, w, x, y, n, m, d, p.objective, tp.nfold, sf2, value, nullptr, g, gz,
                          &col, &lane0);
    if (info) break;
    const double gn = sn2 * g[1];
    // every read of θ and Z of this step lies before block_gradient()'s closing barriers
    if (t == 0) {
      const int64_t si = pb * p.itr + p.step0 + st;
      p.values[si] = value;
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

size_t batch_fitc_tall_block_lds_bytes(int n, int m, int d) {
  const int ld = odd_ld(m), ch = chunk_rows(n);
  return (size_t)(m * d + ch * d + 2 * ch * ld + kBlkMMat * m * ld + kBlkCVec * ch + kBlkMVec * m +
                  FG * 16 + kThDoubles) * sizeof(double);
}

int64_t batch_fitc_tall_block_ws_doubles(int64_t n, int m, int nfold) {
  const int64_t ld = odd_ld(m);
  return kBlkNMat * n * ld + (int64_t)(nfold + 1) * m * ld + kBlkNVec * n;
}

int batch_fitc_tall_block_steps(int64_t n) {
  const int64_t chunks = (n + kBatchFitcTallChunk - 1) / kBatchFitcTallChunk;
  const int64_t k = kBatchStepsPerLaunch / kBatchFitcTallBlockDiv / (chunks < 1 ? 1 : chunks);
  return (int)(k < 1 ? 1 : k);
}

hipError_t launch_batch_fitc_tall_block(const BatchFitcTallBlockParams& tp, hipStream_t s) {
  const BatchFitcParams& p = tp.b;
  if (p.n < 1 || p.n > GPS_BATCH_FITC_TALL_MAX_N || p.m < 1 || p.m > GPS_BATCH_FITC_MAX_M ||
      p.d < 1 || p.d > GPS_BATCH_MAX_D || p.nprob < 1 || (p.n_ell != 1 && p.n_ell != p.d) ||
      p.nsteps < 0 || p.nsteps > batch_fitc_tall_block_steps(p.n) || tp.nfold < 2 ||
      tp.nfold > GPS_BATCH_BLOCK_MAX_FOLDS || tp.nfold > p.n ||
      (p.objective != GPS_BLOCK_DSS && p.objective != GPS_BLOCK_KC) || !tp.ws ||
      tp.ws_stride < batch_fitc_tall_block_ws_doubles(p.n, p.m, tp.nfold) ||
      (p.mode == BATCH_MODE_GRAD && !tp.value))
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds(
      (const void*)batch_fitc_tall_block_kernel,
      batch_fitc_tall_block_lds_bytes(GPS_BATCH_FITC_TALL_MAX_N, GPS_BATCH_FITC_MAX_M,
                                      GPS_BATCH_MAX_D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_fitc_tall_block_kernel, dim3((unsigned)p.nprob), dim3(FT),
                     batch_fitc_tall_block_lds_bytes(p.n, p.m, p.d), s, tp);
  return hipGetLastError();
}

int batch_fitc_tall_block_va_steps(int64_t n, int64_t nv, int64_t va_every) {
  const int64_t plain = batch_fitc_tall_block_steps(n);
  const int64_t k = kBatchFitcVaRowBudget / (nv < 1 ? 1 : nv) * (va_every < 1 ? 1 : va_every);
  return (int)(k < 1 ? 1 : (k < plain ? k : plain));
}

hipError_t launch_batch_fitc_tall_block_va(const BatchFitcTallBlockVaParams& vp, hipStream_t s) {
  const BatchFitcTallBlockParams& tp = vp.t;
  const BatchFitcParams& p = tp.b;
  const BatchVaParams& va = vp.va;
  if (p.mode != BATCH_MODE_TRAIN || !va.xv || !va.yv || !va.va_sc || va.nv < 1 ||
      va.va_every < 1 || p.n < 1 || p.n > GPS_BATCH_FITC_TALL_MAX_N || p.m < 1 ||
      p.m > GPS_BATCH_FITC_MAX_M || p.d < 1 || p.d > GPS_BATCH_MAX_D || p.nprob < 1 ||
      (p.n_ell != 1 && p.n_ell != p.d) || p.nsteps < 0 ||
      p.nsteps > batch_fitc_tall_block_va_steps(p.n, va.nv, va.va_every) || p.step0 < 0 ||
      (int64_t)p.step0 + p.nsteps > p.itr || tp.nfold < 2 ||
      tp.nfold > GPS_BATCH_BLOCK_MAX_FOLDS || tp.nfold > p.n ||
      (p.objective != GPS_BLOCK_DSS && p.objective != GPS_BLOCK_KC) || !tp.ws ||
      tp.ws_stride < batch_fitc_tall_block_ws_doubles(p.n, p.m, tp.nfold))
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds(
      (const void*)batch_fitc_tall_block_va_kernel,
      batch_fitc_tall_block_lds_bytes(GPS_BATCH_FITC_TALL_MAX_N, GPS_BATCH_FITC_MAX_M,
                                      GPS_BATCH_MAX_D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_fitc_tall_block_va_kernel, dim3((unsigned)p.nprob), dim3(FT),
                     batch_fitc_tall_block_lds_bytes(p.n, p.m, p.d), s, vp);
  return hipGetLastError();
}

}  // namespace gps
