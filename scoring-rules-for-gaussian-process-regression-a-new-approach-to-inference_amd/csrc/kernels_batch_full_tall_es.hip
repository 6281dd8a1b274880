// Batches of full GPs of up to 512 training rows on the block-LOO energy score (KF:607-732).
// DESIGN §32.  The tile product, forward(), the factorisation of a padded block and the contraction
// are batch_full_tall_shared.h's (§24, §26); the algebra per fold is api_block.hip's es_fold.
//
// A step is three kinds of launch on one stream, 256 threads a workgroup ((E) in launches of at most
// 256 workgroups, whole problems each: one round of the chip, so that no launch outlasts ~20 ms):
//   (A) es_forward_kernel   per problem: forward(), P = XᵀX into W0, Gblk's zeros, α and the five
//                           objectives into the problem's vector area
//   (E) es_fold_kernel      per (problem, fold): P_f → Π_f = P_f⁻¹, r_f = Π_f α_f, s = ‖Π_f‖∞,
//                           R = Π_f^½ by the scaled coupled Newton–Schulz iteration on Π_f/s
//                           (schedule from σ²/s, ns_schedule_fill), z = ξR, ẑ = [ξ'R; −r],
//                           D_ij = ‖z_i − ẑ_j‖ by direct differences, the fold's value in
//                           es_reduce's order, W, G_z, G_ẑ, Ḡ = sym(ξᵀG_z + ξ'ᵀG_ẑ), X from the
//                           off-diagonal block of the same iteration on [[C, Ḡ], [0, C]] (the
//                           forward iterates recomputed: 9 products a step, no stored iterates),
//                           G_f = −ΠXΠ − ½(w rᵀ + r wᵀ) into Gblk, g_f = w = Π·∂ES/∂r
//   (C) es_tail_kernel      per problem: the fold values summed in fold order, v = Pg, Y = Gblk·P
//                           with clipped k, P·Y contracted tile by tile, the θ update, the series
// and the final pass is launch_batch_full_tall's kernel with no steps (§24's text).
//
// Workspace per problem (np, bp the padded n and largest fold, Sp = 64·⌈(S + 1)/64⌉):
//   W0 np² | W1 np² | W2 np² (Gblk) | α np | g np | obj 8 | fold values 32 | fold info 32 (ints in
//   doubles' slots, 8 spare) | nfold × [Π bp² | 10 matrices bp² | ξ ξ' z ẑ G_z G_ẑ Sp·bp each |
//   D Sp²]
// A fold's slice is touched by its own workgroup only; (A), (E) and (C) meet at kernel boundaries.
// Every symmetric product is formed on its lower tiles and mirrored, so every iterate is exactly
// symmetric in storage and both operands of a product are read k-major.  Every sum's order is a
// function of (n, d, nfold, num_sim) and the 256 threads.
#include "batch_full_tall_shared.h"

namespace gps {

namespace {

constexpr int kVec = 72;  // obj 8 | fold values 32 | fold info 32
constexpr int kEsFoldWgs = 256;  // fold workgroups a launch holds: the MI355X's compute units

struct EsShape {
  int np, bp, Sp;
  int64_t vec, fws, stride;
};

__host__ __device__ inline EsShape es_shape(int n, int nfold, int S) {
  EsShape e;
  e.np = (int)padded(n);
  e.bp = (int)padded((n + nfold - 1) / nfold);
  e.Sp = (int)padded(S + 1);
  e.vec = 3 * (int64_t)e.np * e.np;
  e.fws = 11 * (int64_t)e.bp * e.bp + 6 * (int64_t)e.Sp * e.bp + (int64_t)e.Sp * e.Sp;
  e.stride = e.vec + 2 * e.np + kVec + nfold * e.fws;
  return e;
}

// θ of problem pb into LDS, then sf², σ² and 1/ℓ_k: step_prologue's arithmetic
__device__ __forceinline__ void load_theta(const BatchParams& p, const Lds& s, int64_t pb,
                                           double& sf2, double& sn2) {
  const int t = threadIdx.x, d = p.d, nth = 2 + p.n_ell;
  double* il = s.th + 20;
  if (t < nth) s.th[t] = p.theta[pb * nth + t];
  __syncthreads();
  sf2 = exp(s.th[0]);
  sn2 = exp(s.th[nth - 1]);
  const double bq = t < d ? s.th[1 + (p.n_ell == 1 ? 0 : t)] : 0.0;
  if (t < d) il[t] = p.kind == GPS_ARD ? exp(-bq) : exp(-0.5 * bq);
  __syncthreads();
}

// ------------------------------------------------------------------ (A)
__global__ __launch_bounds__(BT) void es_forward_kernel(BatchFullTallEsParams tp) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const BatchParams& p = tp.b;
  const int n = p.n, d = p.d, t = threadIdx.x;
  const EsShape sh = es_shape(n, tp.nfold, tp.num_sim);
  const int np = sh.np, nb = np / T;
  const int64_t ld = np, pb = blockIdx.x;
  if (p.info[pb]) return;  // failed in an earlier step: (C) writes the NaNs
  const Lds s = carve(sm, np);
  const double* x = p.x + pb * n * d;
  double* W0 = tp.ws + pb * tp.ws_stride;
  double* W1 = W0 + ld * ld;
  double* W2 = W1 + ld * ld;
  double* vec = W0 + sh.vec;
  for (int e = t; e < n; e += BT) s.y[e] = p.y[pb * n + e];
  double sf2, sn2, obj[GPS_N_OBJ];
  load_theta(p, s, pb, sf2, sn2);
  const int info = forward(s, x, W0, W1, n, np, d, sf2, sn2, obj);
  if (info) {
    if (t == 0) p.info[pb] = info;
    return;
  }
  gram_lower(s, W1, W0, ld, nb);  // P = XᵀX; X is dead from here on
  gblk_zero(W2, n, tp.nfold, ld, nb, t);
  for (int e = t; e < np; e += BT) vec[e] = e < n ? s.alpha[e] : 0.0;
  if (t == 0)
    for (int q = 0; q < GPS_N_OBJ; ++q) vec[2 * np + q] = obj[q];
}

// ------------------------------------------------------------------ (E)
// C = al·(A1·B1 + A2·B2) + dg·I on the lower tiles, mirrored; every operand symmetric in storage
// (nb×nb tiles, row stride ld), A2 may be NULL, C none of the operands.  Ends synchronised.
__device__ __forceinline__ void sym_prod(const Lds& s, const double* A1, const double* B1,
                                         const double* A2, const double* B2, double* C, int ld,
                                         int nb, double al, double dg) {
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<KMAJ, KMAJ, false>(acc, A1 + bi * T, ld, B1 + bj * T, ld, 0, nb * T, nullptr, s.pan);
      if (A2)
        tile_mma<KMAJ, KMAJ, false>(acc, A2 + bi * T, ld, B2 + bj * T, ld, 0, nb * T, nullptr,
                                    s.pan);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(mi, r), i = bi * T + row;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int col = acc_col(ni), j = bj * T + col;
            if (bi == bj && col > row) continue;
            const double v = al * acc[mi][ni][r] + (i == j ? dg : 0.0);
            C[(int64_t)i * ld + j] = v;
            C[(int64_t)j * ld + i] = v;
          }
        }
    }
  __syncthreads();
}

// mt×nt tiles of opA·opB (+ opA2·opB2, same layouts) over k in [0, kd): epi(i, j, value) per
// entry.  A is XMAJ (rows i, row stride lda) or KMAJ (rows k); B is KMAJ.  Ends synchronised.
template <int AL, class Epi>
__device__ __forceinline__ void gen_prod(const Lds& s, const double* A, const double* A2, int lda,
                                         const double* B, const double* B2, int ldb, int mt, int nt,
                                         int kd, Epi epi) {
  for (int bi = 0; bi < mt; ++bi)
    for (int bj = 0; bj < nt; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      const int64_t ao = AL == XMAJ ? (int64_t)bi * T * lda : (int64_t)bi * T;
      tile_mma<AL, KMAJ, false>(acc, A + ao, lda, B + bj * T, ldb, 0, kd, nullptr, s.pan);
      if (A2) tile_mma<AL, KMAJ, false>(acc, A2 + ao, lda, B2 + bj * T, ldb, 0, kd, nullptr, s.pan);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            epi(bi * T + acc_row(mi, r), bj * T + acc_col(ni), acc[mi][ni][r]);
    }
  __syncthreads();
}

__global__ __launch_bounds__(BT) void es_fold_kernel(BatchFullTallEsParams tp, int64_t set_off,
                                                     int64_t pb0) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const BatchParams& p = tp.b;
  const int n = p.n, t = threadIdx.x, nfold = tp.nfold, S = tp.num_sim;
  const int64_t pb = pb0 + blockIdx.x / nfold;
  const int f = (int)(blockIdx.x % nfold);
  if (p.info[pb]) return;
  const EsShape sh = es_shape(n, nfold, S);
  const int np = sh.np, Sp = sh.Sp, nS = Sp / T;
  const Lds s = carve(sm, max(sh.bp, Sp));
  const int a = fold_begin(f, n, nfold), bs = fold_begin(f + 1, n, nfold) - a;
  const int bq = (int)padded(bs), nbf = bq / T;
  const int64_t ld = np, b2 = (int64_t)bq * bq, sb = (int64_t)Sp * bq;
  double* W0 = tp.ws + pb * tp.ws_stride;
  double* W2 = W0 + 2 * ld * ld;
  double* vec = W0 + sh.vec;
  double* gvec = vec + np;
  double* fval = vec + 2 * np + 8;
  int* finfo = reinterpret_cast<int*>(vec + 2 * np + 40);
  double* F = vec + 2 * np + kVec + f * sh.fws;
  double* PI = F;
  double* M[10];
  for (int q = 0; q < 10; ++q) M[q] = F + (1 + q) * b2;
  double* xi = F + 11 * b2;
  double *xip = xi + sb, *Zs = xip + sb, *Zh = Zs + sb, *Gz = Zh + sb, *Gh = Gz + sb;
  double* D = Gh + sb;
  double* al = s.alpha;  // α_f, zero in the padding
  double* r = s.beta;    // r_f, zero in the padding
  double* w = s.dinv;
  double* dr = s.u;      // first the row sums of |Π_f|, then ∂ES/∂r
  double* rs = s.ct;     // W's row sums (Sp)
  double* cs = s.v;      // W's column sums (Sp)
  double* sched = s.y;   // β per step, kBatchEsNsCap <= 64 of them
  const int nth = 2 + p.n_ell;
  const double sn2 = exp(p.theta[pb * nth + nth - 1]);

  for (int e = t; e < bq * bq; e += BT) {  // P_f, the identity in the padding
    const int i = e / bq, j = e - i * bq;
    PI[e] = i < bs && j < bs ? W0[(a + i) * ld + a + j] : (i == j ? 1.0 : 0.0);
  }
  for (int i = t; i < bq; i += BT) al[i] = i < bs ? vec[a + i] : 0.0;
  __syncthreads();
  const int bad = factor_invert(s, PI, M[0], bq, nbf, bs, s.piv);
  if (bad) {
    if (t == 0) finfo[f] = n + a + bad;
    return;
  }
  gram_lower(s, M[0], PI, bq, nbf);  // Π_f = X_fᵀX_f over L_f, the identity in the padding
  for (int i = t; i < bq; i += BT) {  // r_f = Π_f α_f and Π_f's absolute row sums
    double rr = 0.0, nr = 0.0;
    if (i < bs) {
#pragma unroll 4
      for (int j = 0; j < bs; ++j) {
        const double v = PI[j * bq + i];
        rr = fma(v, al[j], rr);
        nr += fabs(v);
      }
    }
    r[i] = rr;
    dr[i] = nr;
  }
  __syncthreads();
  if (t == 0) {  // s = ‖Π_f‖∞ (padded a touch, as the resident path); the schedule from σ²/s
    double nm = 0.0;
    for (int i = 0; i < bs; ++i) nm = dr[i] > nm ? dr[i] : nm;
    const double sc0 = nm * (1.0 + 1e-12);
    s.sw[0] = sc0;
    s.sw[1] = (double)ns_schedule_fill(sn2 / sc0, sched, kBatchEsNsCap);
  }
  __syncthreads();
  const double sc = s.sw[0];
  const int iters = (int)s.sw[1];
  if (!(iters > 0) || !(sc > 0.0) || !(sn2 > 0.0)) {
    if (t == 0) finfo[f] = 2 * n + 1 + f;
    return;
  }
  const double rt = sqrt(sc);

  // the draws, padded with zeros: ξ then ξ', S × b_f each
  const double* src = tp.draws + pb * tp.draw_sets * 2 * (int64_t)S * n + set_off +
                      2 * (int64_t)S * a;
  for (int64_t e = t; e < sb; e += BT) {
    const int i = (int)(e / bq), j = (int)(e - (int64_t)i * bq);
    const bool live = i < S && j < bs;
    xi[e] = live ? src[(int64_t)i * bs + j] : 0.0;
    xip[e] = live ? src[(int64_t)(S + i) * bs + j] : 0.0;
  }
  // forward iteration: Y → (Π/s)^½, Z → its inverse
  double *Y = M[1], *Z = M[2], *Tm = M[3], *Yn = M[4], *Zn = M[5];
  for (int e = t; e < bq * bq; e += BT) {
    const int i = e / bq, j = e - i * bq;
    const bool live = i < bs && j < bs;
    Y[e] = live ? PI[e] / sc : (i == j ? 1.0 : 0.0);
    Z[e] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const double bt = sched[it], mu = sqrt(bt);
    sym_prod(s, Z, Y, nullptr, nullptr, Tm, bq, nbf, -0.5 * bt, 1.5);
    sym_prod(s, Y, Tm, nullptr, nullptr, Yn, bq, nbf, mu, 0.0);
    sym_prod(s, Tm, Z, nullptr, nullptr, Zn, bq, nbf, mu, 0.0);
    double* q = Y; Y = Yn; Yn = q;
    q = Z; Z = Zn; Zn = q;
  }
  // z = ξR, ẑ = [ξ'R; −r]
  gen_prod<XMAJ>(s, xi, nullptr, bq, Y, nullptr, bq, nS, nbf, bq,
                 [&](int i, int j, double v) { Zs[(int64_t)i * bq + j] = rt * v; });
  gen_prod<XMAJ>(s, xip, nullptr, bq, Y, nullptr, bq, nS, nbf, bq,
                 [&](int i, int j, double v) { Zh[(int64_t)i * bq + j] = i == S ? -r[j] : rt * v; });
  // D_ij = ‖z_i − ẑ_j‖ (i < S, j <= S) by direct differences: 16×16 pairs a pass, the rows staged
  // in LDS at an odd stride
  {
    const int ti = t >> 4, tj = t & 15, zl = bq + 1;
    double* za = s.tile;
    double* zb = s.tile + 16 * zl;
    for (int i0 = 0; i0 < S; i0 += 16) {
      for (int e = t; e < 16 * bq; e += BT) {
        const int rr = e / bq, k = e - rr * bq;
        za[rr * zl + k] = i0 + rr < S ? Zs[(int64_t)(i0 + rr) * bq + k] : 0.0;
      }
      for (int j0 = 0; j0 <= S; j0 += 16) {
        for (int e = t; e < 16 * bq; e += BT) {
          const int rr = e / bq, k = e - rr * bq;
          zb[rr * zl + k] = j0 + rr <= S ? Zh[(int64_t)(j0 + rr) * bq + k] : 0.0;
        }
        __syncthreads();
        double acc = 0.0;
#pragma unroll 8
        for (int k = 0; k < bq; ++k) {
          const double df = za[ti * zl + k] - zb[tj * zl + k];
          acc = fma(df, df, acc);
        }
        const int i = i0 + ti, j = j0 + tj;
        if (i < S && j <= S) D[(int64_t)i * Sp + j] = sqrt(acc);
        __syncthreads();
      }
    }
  }
  // the value in es_reduce's order; D becomes W = ∂ES/∂D ∘ D⁻¹, zero-padded, with its sums
  {
    const double cz = 1.0 / ((double)S * (S - 1)), cy = 1.0 / S, beta = tp.beta;
    const bool b1 = beta == 1.0;
    double v[2] = {0.0, 0.0};
    for (int i = t; i < Sp; i += BT) {
      double* row = D + (int64_t)i * Sp;
      double rsum = 0.0;
      if (i < S) {
        for (int j = 0; j <= S; ++j) {
          const double dd = row[j];
          const double pw = b1 ? dd : pow(dd, beta);
          if (j < S) v[0] += pw;
          else v[1] += pw;
          const double wv = (j < S ? -0.5 * cz : cy) * (b1 ? 1.0 / dd : beta * pw / (dd * dd));
          row[j] = wv;
          rsum += wv;
        }
      }
      for (int j = i < S ? S + 1 : 0; j < Sp; ++j) row[j] = 0.0;
      rs[i] = rsum;
    }
    block_sum<2>(v, s.sh);  // ends with a barrier: W is complete for the column sums
    if (t == 0) fval[f] = cy * v[1] - 0.5 * cz * v[0];
    for (int j = t; j < Sp; j += BT) {
      double c = 0.0;
      for (int i = 0; i < S; ++i) c += D[(int64_t)i * Sp + j];
      cs[j] = c;
    }
    __syncthreads();
  }
  // G_z = diag(ΣW) z − W ẑ,  G_ẑ = diag(ΣWᵀ) ẑ − Wᵀ z
  gen_prod<XMAJ>(s, D, nullptr, Sp, Zh, nullptr, bq, nS, nbf, Sp, [&](int i, int j, double v) {
    Gz[(int64_t)i * bq + j] = fma(rs[i], Zs[(int64_t)i * bq + j], -v);
  });
  gen_prod<KMAJ>(s, D, nullptr, Sp, Zs, nullptr, bq, nS, nbf, Sp, [&](int i, int j, double v) {
    Gh[(int64_t)i * bq + j] = fma(cs[i], Zh[(int64_t)i * bq + j], -v);
  });
  // ∂ES/∂r = −G_ẑ[S] (ẑ_S = −r);  w = Π ∂ES/∂r
  for (int j = t; j < bq; j += BT) dr[j] = j < bs ? -Gh[(int64_t)S * bq + j] : 0.0;
  __syncthreads();
  for (int i = t; i < bq; i += BT) {
    double ww = 0.0;
    if (i < bs) {
#pragma unroll 4
      for (int j = 0; j < bs; ++j) ww = fma(PI[j * bq + i], dr[j], ww);
    }
    w[i] = ww;
  }
  // Ḡ = ξᵀG_z + ξ'ᵀG_ẑ, then symmetrised and scaled into the derivative block
  double* Gb = M[5];
  gen_prod<KMAJ>(s, xi, xip, bq, Gz, Gh, bq, nbf, nbf, Sp,
                 [&](int i, int j, double v) { Gb[(int64_t)i * bq + j] = v; });
  double *Y1 = M[1], *Z1 = M[2], *T1 = M[3], *Y1n = M[4], *Z1n = M[5];
  double *Y2 = M[6], *Z2 = M[7], *T2 = M[8], *Y2n = M[9], *Z2n = M[0];
  for (int e = t; e < bq * bq; e += BT) {
    const int i = e / bq, j = e - i * bq;
    const bool live = i < bs && j < bs;
    Y1[e] = live ? PI[e] / sc : (i == j ? 1.0 : 0.0);
    Z1[e] = i == j ? 1.0 : 0.0;
    Y2[e] = live ? 0.5 * (Gb[e] + Gb[j * bq + i]) / sc : 0.0;
    Z2[e] = 0.0;
  }
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const double bt = sched[it], mu = sqrt(bt);
    sym_prod(s, Z1, Y1, nullptr, nullptr, T1, bq, nbf, -0.5 * bt, 1.5);
    sym_prod(s, Z1, Y2, Z2, Y1, T2, bq, nbf, -0.5 * bt, 0.0);  // T2 = −½β(Z1Y2 + Z2Y1)
    sym_prod(s, Y1, T2, Y2, T1, Y2n, bq, nbf, mu, 0.0);        // Y2 ← √β(Y1T2 + Y2T1)
    sym_prod(s, T1, Z2, T2, Z1, Z2n, bq, nbf, mu, 0.0);        // Z2 ← √β(T1Z2 + T2Z1)
    sym_prod(s, Y1, T1, nullptr, nullptr, Y1n, bq, nbf, mu, 0.0);
    sym_prod(s, T1, Z1, nullptr, nullptr, Z1n, bq, nbf, mu, 0.0);
    double* q = Y1; Y1 = Y1n; Y1n = q;
    q = Z1; Z1 = Z1n; Z1n = q;
    q = Y2; Y2 = Y2n; Y2n = q;
    q = Z2; Z2 = Z2n; Z2n = q;
  }
  // X = √s·Y2;  G_f = −Π X Π − ½(w rᵀ + r wᵀ) into Gblk's diagonal block, g_f = w
  gen_prod<KMAJ>(s, Y2, nullptr, bq, PI, nullptr, bq, nbf, nbf, bq,
                 [&](int i, int j, double v) { T2[(int64_t)i * bq + j] = v; });
  for (int bi = 0; bi < nbf; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<KMAJ, KMAJ, false>(acc, PI + bi * T, bq, T2 + bj * T, bq, 0, bq, nullptr, s.pan);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = acc_row(mi, q), i = bi * T + row;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int col = acc_col(ni), j = bj * T + col;
            if (i >= bs || j >= bs || (bi == bj && col > row)) continue;
            const double gval = fma(-rt, acc[mi][ni][q], -0.5 * (w[i] * r[j] + r[i] * w[j]));
            W2[(a + i) * ld + a + j] = gval;
            W2[(a + j) * ld + a + i] = gval;
          }
        }
    }
  for (int i = t; i < bs; i += BT) gvec[a + i] = w[i];
  if (t == 0) finfo[f] = 0;
}

// ------------------------------------------------------------------ (C)
__global__ __launch_bounds__(BT) void es_tail_kernel(BatchFullTallEsParams tp) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const BatchParams& p = tp.b;
  const int n = p.n, d = p.d, t = threadIdx.x, nfold = tp.nfold;
  const EsShape sh = es_shape(n, nfold, tp.num_sim);
  const int np = sh.np, nb = np / T, nth = 2 + p.n_ell;
  const int64_t ld = np, pb = blockIdx.x;
  const Lds s = carve(sm, np);
  const double* x = p.x + pb * n * d;
  double* W0 = tp.ws + pb * tp.ws_stride;
  double* W1 = W0 + ld * ld;
  double* W2 = W1 + ld * ld;
  double* vec = W0 + sh.vec;
  const double* fval = vec + 2 * np + 8;
  const int* finfo = reinterpret_cast<const int*>(vec + 2 * np + 40);
  const bool grad_mode = p.mode == BATCH_MODE_GRAD;
  const int64_t si = pb * p.itr + p.step0;
  int info = p.info[pb];
  for (int f = 0; f < nfold && info == 0; ++f) info = finfo[f];  // the first fold that failed
  if (info) {
    if (grad_mode) {
      full_grad_end(p, pb, t, info);
      if (t == 0) tp.value[pb] = batch_nan();
      if (tp.fold_values && t < nfold) tp.fold_values[pb * nfold + t] = batch_nan();
    } else {
      if (t == 0) {
        p.info[pb] = info;
        p.values[si] = batch_nan();
      }
      if (t < nth) p.thetas[si * nth + t] = batch_nan();
    }
    return;
  }
  double sf2, sn2;
  load_theta(p, s, pb, sf2, sn2);
  for (int e = t; e < n; e += BT) {
    s.alpha[e] = vec[e];
    s.u[e] = vec[np + e];
  }
  __syncthreads();
  double value = 0.0;
  for (int f = 0; f < nfold; ++f) value += fval[f];
  for (int i = t; i < n; i += BT) {  // v = Pg: a thread per column of the symmetric P
    double vv = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) vv = fma(W0[j * ld + i], s.u[j], vv);
    s.v[i] = vv;
  }
  // Y = Gblk·P into W1, k clipped to the tile columns the row tile's folds touch
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
  double g[BG];
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
  if (t == 0) {
    const double bscale = p.kind == GPS_RBF ? 0.5 : 1.0;
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
    if (grad_mode) {
      for (int q = 0; q < GPS_N_OBJ; ++q) p.obj[pb * GPS_N_OBJ + q] = vec[2 * np + q];
#pragma unroll
      for (int q = 0; q < BG - 1; ++q)
        if (q < nth - 1) p.grad[pb * nth + q] = gr[q];
      p.grad[pb * nth + nth - 1] = gn;
      tp.value[pb] = value;
      if (tp.fold_values)
        for (int f = 0; f < nfold; ++f) tp.fold_values[pb * nfold + f] = fval[f];
      p.info[pb] = 0;
    } else {
      p.values[si] = value;
#pragma unroll
      for (int q = 0; q < BG - 1; ++q)
        if (q < nth - 1) {
          const double nv = s.th[q] - p.lr * gr[q];
          p.theta[pb * nth + q] = nv;
          p.thetas[si * nth + q] = nv;
        }
      const double nv = s.th[nth - 1] - p.lr * gn;
      p.stale[pb] = s.th[nth - 1];  // the σ² this step's forward used
      p.theta[pb * nth + nth - 1] = nv;
      p.thetas[si * nth + nth - 1] = nv;
      p.steps_done[pb] = p.steps_done[pb] + 1;
    }
  }
}

size_t es_fold_lds_bytes(int nv) {
  return (size_t)(T * TL + kPan + 8 * nv + 2 * T + BG * 16 + kThDoubles) * sizeof(double);
}

}  // namespace

int64_t batch_full_tall_es_ws_doubles(int64_t n, int nfold, int num_sim) {
  return es_shape((int)n, nfold, num_sim).stride;
}

hipError_t launch_batch_full_tall_es(const BatchFullTallEsParams& tp, int phase, hipStream_t s) {
  const BatchParams& p = tp.b;
  // (the fold count first: the workspace size divides by it; a step is a launch sequence, so a
  // launch runs at most one)
  if (tp.nfold < 2 || tp.nfold > GPS_BATCH_BLOCK_MAX_FOLDS || tp.nfold > p.n ||
      (p.n + tp.nfold - 1) / tp.nfold > GPS_BATCH_ES_MAX_FOLD || tp.num_sim < 2 ||
      tp.num_sim > GPS_BATCH_ES_MAX_SIM || !(tp.beta > 0.0 && tp.beta <= 2.0) || !tp.draws ||
      tp.draw_sets < 1 || (int64_t)p.nprob * tp.nfold > (int64_t)1 << 30 ||
      (p.mode == BATCH_MODE_GRAD && !tp.value) || phase < 0 || phase >= ES_PHASES ||
      !full_tall_args_ok(p, [](int64_t) { return 1; }, tp.ws, tp.ws_stride,
                         batch_full_tall_es_ws_doubles(p.n, tp.nfold, tp.num_sim)))
    return hipErrorInvalidValue;
  const EsShape sh = es_shape(p.n, tp.nfold, tp.num_sim);
  const size_t lds_n = batch_full_tall_lds_bytes(p.n);
  const size_t lds_f = es_fold_lds_bytes(std::max(sh.bp, sh.Sp));
  hipError_t e;
  if ((e = raise_dynamic_lds((const void*)es_forward_kernel,
                             batch_full_tall_lds_bytes(GPS_BATCH_FULL_TALL_MAX_N))) != hipSuccess ||
      (e = raise_dynamic_lds((const void*)es_tail_kernel,
                             batch_full_tall_lds_bytes(GPS_BATCH_FULL_TALL_MAX_N))) != hipSuccess ||
      (e = raise_dynamic_lds((const void*)es_fold_kernel,
                             es_fold_lds_bytes((int)padded(GPS_BATCH_ES_MAX_SIM + 1)))) != hipSuccess)
    return e;
  if (phase == ES_FINAL) {  // §24's final pass: its kernel with no steps
    if (p.mode != BATCH_MODE_TRAIN || !p.do_final) return hipSuccess;
    BatchFullTallParams fp = {p, tp.ws, tp.ws_stride};
    fp.b.objective = GPS_OBJ_NLML;
    fp.b.step0 = p.step0 + p.nsteps;
    fp.b.nsteps = 0;
    return launch_batch_full_tall(fp, s);
  }
  if (p.mode != BATCH_MODE_GRAD && p.nsteps != 1) return hipSuccess;
  const int64_t set = p.mode == BATCH_MODE_GRAD ? 0 : p.step0 % tp.draw_sets;
  const int64_t set_off = set * 2 * (int64_t)tp.num_sim * p.n;
  if (phase == ES_FORWARD)
    hipLaunchKernelGGL(es_forward_kernel, dim3((unsigned)p.nprob), dim3(BT), lds_n, s, tp);
  else if (phase == ES_FOLDS) {
    // a fold's workgroup has a compute unit to itself (its LDS), so kEsFoldWgs workgroups are one
    // round of the chip: whole problems up to that many a launch keep a launch one round long
    const int64_t per = std::max<int64_t>(1, kEsFoldWgs / tp.nfold);
    for (int64_t pb0 = 0; pb0 < p.nprob; pb0 += per) {
      const int64_t nq = std::min<int64_t>(per, p.nprob - pb0);
      hipLaunchKernelGGL(es_fold_kernel, dim3((unsigned)(nq * tp.nfold)), dim3(BT), lds_f, s, tp,
                         set_off, pb0);
    }
  } else
    hipLaunchKernelGGL(es_tail_kernel, dim3((unsigned)p.nprob), dim3(BT), lds_n, s, tp);
  return hipGetLastError();
}

}  // namespace gps
