// Batches of full GPs of up to 512 training rows on the block-LOO objectives GPS_BLOCK_DSS and
// GPS_BLOCK_KC (KF:487-601, K20:655-720), one workgroup of 256 threads per problem.  DESIGN §26.
// The kernel is batch_full_tall_shared.h's body — forward(), the SGD loop, the final pass and the
// outputs of kernels_batch_full_tall.hip (§24) — with this file's block_gradient() in gradient()'s
// place.
//
// Folds are [⌊f·n/k⌋, ⌊(f+1)·n/k⌋) (KF:496-499), of b_f rows each; with P = A⁻¹ and α = Py:
//   P_f = P_ff,  Π_f = P_f⁻¹ (Cholesky with the fused inverse, Π_f = X_fᵀX_f),  r_f = Π_f α_f
//   DSS  value Σ_f ½b_f·log2π − ½log|P_f| + ½α_fᵀr_f;   G_f = −½(Π_f + r_f r_fᵀ),  g_f = r_f
//   KC   m_f = y_f − r_f, c_f = diag Π_f, value Σ_f mean crps(m_f, c_f, y_f); (gm, gc) the fold
//        mean's derivatives, w_f = Π_f gm:  G_f = ½(w_f r_fᵀ + r_f w_fᵀ) − Π_f diag(gc) Π_f,
//        g_f = −w_f
//   M = −P·Gblk·P − ½(vαᵀ + αvᵀ), v = Pg, contracted with ∂A/∂θ tile by tile as §24's LOO M is.
//
// Workspace per problem, np = 64·⌈n/64⌉, bp = 64·⌈⌈n/k⌉/64⌉ (the largest fold, padded):
//   W0  np²               A, L, then P (both triangles) for the rest of the step
//   W1  max(np², 2·bp²)   X = L⁻¹; X dead after P: the fold scratch S0 | S1 (bq² each, bq the
//                         fold's own padded size: P_f with identity padding, L_f, then Π_f | X_f);
//                         the folds done: Y = Gblk·P (np²)
//   W2  np²               Gblk: the G_f on the diagonal, zeros in the rest of the tile columns a
//                         row tile's folds touch (all that Y's k ranges read)
// 2·bp² exceeds np² only at np = 64 (one tile, where bp = np).  LDS is §24's layout unchanged: the
// fold vectors live in n-vectors that are dead after forward() — r in beta, w in dinv, g in u, the
// fold-local diag scale gc in ct, gm in v until v = Pg replaces it, L_f's diagonal in piv.
// Ordering, exits and the order of every sum are as §24 promises: a function of (n, d, nfold) and
// the 256 threads alone.
#include "batch_full_tall_shared.h"

namespace gps {

namespace {

__device__ __forceinline__ int block_gradient(const Lds& s, const double* x, double* W0,
                                              double* W1, double* W2, int n, int np, int d,
                                              int objective, int nfold, double sf2,
                                              double (&g)[BG], double& value,
                                              double* fold_values) {
  const int t = threadIdx.x, nb = np / T;
  const int64_t ld = np;
  double* r = s.beta;   // r_f at the fold's global rows
  double* w = s.dinv;   // w_f likewise
  double* gv = s.u;     // g
  double* gc = s.ct;    // fold-local: the CRPS variance derivative, zero in the fold's padding
  double* gm = s.v;     // the CRPS mean derivative at the fold's global rows
  gram_lower(s, W1, W0, ld, nb);  // P = XᵀX; X is dead from here on
  gblk_zero(W2, n, nfold, ld, nb, t);
  __syncthreads();
  value = 0.0;
  for (int f = 0; f < nfold; ++f) {
    const int a = fold_begin(f, n, nfold), bs = fold_begin(f + 1, n, nfold) - a;
    const int bq = T * ((bs + T - 1) / T), nbf = bq / T;
    double* S0 = W1;
    double* S1 = W1 + (int64_t)bq * bq;
    for (int e = t; e < bq * bq; e += BT) {  // P_f, the identity in the padding
      const int i = e / bq, j = e - i * bq;
      S0[e] = i < bs && j < bs ? W0[(a + i) * ld + a + j] : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    const int bad = factor_invert(s, S0, S1, bq, nbf, bs, s.piv + a);
    if (bad) return n + a + bad;
    gram_lower(s, S1, S0, bq, nbf);  // Π_f = X_fᵀX_f over L_f
    for (int i = t; i < bs; i += BT) {  // r_f = Π_f α_f: a thread per column of the symmetric Π_f
      double rr = 0.0;
#pragma unroll 4
      for (int j = 0; j < bs; ++j) rr = fma(S0[j * bq + i], s.alpha[a + j], rr);
      r[a + i] = rr;
    }
    __syncthreads();
    double fv;
    if (objective == GPS_BLOCK_DSS) {
      double v2[2] = {0.0, 0.0};  // Σ log L_f,kk = ½log|P_f|, α_fᵀr_f
      for (int i = t; i < bs; i += BT) {
        v2[0] += log(s.piv[a + i]);
        v2[1] = fma(s.alpha[a + i], r[a + i], v2[1]);
        gv[a + i] = r[a + i];
      }
      block_sum<2>(v2, s.sh);
      fv = 0.5 * bs * 1.83787706640934548356 - v2[0] + 0.5 * v2[1];
      for (int e = t; e < bs * bs; e += BT) {
        const int i = e / bs, j = e - i * bs;
        W2[(a + i) * ld + a + j] = -0.5 * fma(r[a + i], r[a + j], S0[i * bq + j]);
      }
    } else {
      double v1[1] = {0.0};
      for (int i = t; i < bq; i += BT) {
        double cc = 0.0;
        if (i < bs) {
          const double c = S0[i * bq + i], yy = s.y[a + i], m = yy - r[a + i];
          const double sd = sqrt(c), z = (yy - m) / sd;
          const double cdf = 0.5 * (1.0 + erf(z * 0.70710678118654752440));
          const double pdf = 0.39894228040143267794 * exp(-0.5 * z * z);
          v1[0] += crps_term(m, c, yy);
          gm[a + i] = (1.0 - 2.0 * cdf) / bs;
          cc = (2.0 * pdf - 0.56418958354775628695) / (2.0 * sd) / bs;
        }
        gc[i] = cc;
      }
      block_sum<1>(v1, s.sh);  // (its barriers publish gm and gc)
      fv = v1[0] / bs;
      for (int i = t; i < bs; i += BT) {  // w_f = Π_f gm
        double ww = 0.0;
#pragma unroll 4
        for (int j = 0; j < bs; ++j) ww = fma(S0[j * bq + i], gm[a + j], ww);
        w[a + i] = ww;
        gv[a + i] = -ww;
      }
      __syncthreads();
      for (int bi = 0; bi < nbf; ++bi)
        for (int bj = 0; bj < nbf; ++bj) {
          d4 acc[2][2];  // (Π_f diag(gc) Π_f)_ij
          acc_zero(acc);
          tile_mma<KMAJ, KMAJ, true>(acc, S0 + bi * T, bq, S0 + bj * T, bq, 0, bq, gc, s.pan);
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int i = bi * T + acc_row(mi, q);
#pragma unroll
              for (int ni = 0; ni < 2; ++ni) {
                const int j = bj * T + acc_col(ni);
                if (i < bs && j < bs)
                  W2[(a + i) * ld + a + j] =
                      0.5 * (w[a + i] * r[a + j] + r[a + i] * w[a + j]) - acc[mi][ni][q];
              }
            }
        }
    }
    value += fv;
    if (fold_values && t == 0) fold_values[f] = fv;
    __syncthreads();  // the next fold overwrites S0, gc
  }
  for (int i = t; i < n; i += BT) {  // v = Pg: a thread per column of the symmetric P
    double vv = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) vv = fma(W0[j * ld + i], gv[j], vv);
    s.v[i] = vv;
  }
  // Y = Gblk·P over the fold scratch, k clipped to the tile columns the row tile's folds touch
  for (int bi = 0; bi < nb; ++bi) {
    int klo, khi;
    fold_span(bi, n, nfold, klo, khi);
    for (int bj = 0; bj < nb; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, W2 + bi * T * ld, ld, W0 + bj * T, ld, klo, khi, nullptr,
                                  s.pan);
      acc_store<false>(acc, W1 + bi * T * ld + bj * T, ld, 1.0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < BG; ++q) g[q] = 0.0;
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      d4 acc[2][2];  // (P·Gblk·P)_ij
      acc_zero(acc);
      tile_mma<KMAJ, KMAJ, false>(acc, W0 + bi * T, ld, W1 + bj * T, ld, 0, np, nullptr, s.pan);
      contract_tile(s, x, acc, bi, bj, n, d, sf2, true, g);
    }
  block_sum<BG>(g, s.sh);
  return 0;
}

__global__ __launch_bounds__(BT) void batch_full_tall_block_kernel(BatchFullTallBlockParams tp) {
  tall_body<true>(tp.b, tp.ws, tp.ws_stride, tp.nfold, tp.w1, tp.value, tp.fold_values);
}

// the same fit with the validation rows scored at the checkpoints
__global__ __launch_bounds__(BT) void batch_full_tall_block_va_kernel(BatchFullTallBlockParams tp) {
  tall_body<true, true>(tp.b, tp.ws, tp.ws_stride, tp.nfold, tp.w1, tp.value, tp.fold_values);
}

// W1's doubles: X, then the fold scratch, then Y
int64_t w1_doubles(int64_t n, int nfold) {
  const int64_t np = padded(n), bp = padded((n + nfold - 1) / nfold);
  return std::max(np * np, 2 * bp * bp);
}

}  // namespace

int64_t batch_full_tall_block_ws_doubles(int64_t n, int nfold) {
  const int64_t np = padded(n);
  return 2 * np * np + w1_doubles(n, nfold);
}

namespace {

// what both launchers refuse (the fold count first: the workspace size divides by it)
bool block_args_ok(const BatchFullTallBlockParams& tp) {
  const BatchParams& p = tp.b;
  return !(tp.nfold < 2 || tp.nfold > GPS_BATCH_BLOCK_MAX_FOLDS || tp.nfold > p.n ||
           (p.objective != GPS_BLOCK_DSS && p.objective != GPS_BLOCK_KC) ||
           (p.mode == BATCH_MODE_GRAD && !tp.value) ||
           !full_tall_args_ok(p, batch_full_tall_steps, tp.ws, tp.ws_stride,
                              batch_full_tall_block_ws_doubles(p.n, tp.nfold)));
}

}  // namespace

hipError_t launch_batch_full_tall_block(const BatchFullTallBlockParams& tq, hipStream_t s) {
  BatchFullTallBlockParams tp = tq;
  const BatchParams& p = tp.b;
  if (!block_args_ok(tp)) return hipErrorInvalidValue;
  tp.w1 = w1_doubles(p.n, tp.nfold);
  const hipError_t e = raise_dynamic_lds((const void*)batch_full_tall_block_kernel,
                                         batch_full_tall_lds_bytes(GPS_BATCH_FULL_TALL_MAX_N));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_full_tall_block_kernel, dim3((unsigned)p.nprob), dim3(BT),
                     batch_full_tall_lds_bytes(p.n), s, tp);  // §24's LDS layout unchanged
  return hipGetLastError();
}

hipError_t launch_batch_full_tall_block_va(const BatchFullTallBlockParams& tq, hipStream_t s) {
  BatchFullTallBlockParams tp = tq;
  const BatchParams& p = tp.b;
  if (!block_args_ok(tp) || !full_tall_va_args_ok(p)) return hipErrorInvalidValue;
  tp.w1 = w1_doubles(p.n, tp.nfold);
  const hipError_t e = raise_dynamic_lds((const void*)batch_full_tall_block_va_kernel,
                                         batch_full_tall_lds_bytes(GPS_BATCH_FULL_TALL_MAX_N));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_full_tall_block_va_kernel, dim3((unsigned)p.nprob), dim3(BT),
                     batch_full_tall_lds_bytes(p.n), s, tp);  // LDS and workspace as without
  return hipGetLastError();
}

}  // namespace gps
