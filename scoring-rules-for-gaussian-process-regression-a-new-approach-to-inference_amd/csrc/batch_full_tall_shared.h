// What the tall full-GP batch kernels share: kernels_batch_full_tall.hip (the pointwise
// objectives), kernels_batch_full_tall_block.hip (the block-LOO DSS / KC objectives,
// §26) and kernels_batch_full_tall_es.hip (the block-LOO energy score, §32).
// Included once by each of the three files; everything sits in that file's anonymous namespace.
//
// Batches of full GPs of up to GPS_BATCH_FULL_TALL_MAX_N = 512 training rows, one workgroup of 256
// threads per problem: kernels_batch.hip's evaluation, SGD loop and final pass step
// for step, with the n×n arrays in a per-problem device workspace instead of LDS and the O(n³)
// work done tile by tile (T = kBatchFullTallTile = 64) on v_mfma_f64_16x16x4.  DESIGN §24.
//
// Workspace per problem: two np×np row-major arrays, np = T·ceil(n/T).  W0 holds A = K + σ²I, then
// the off-diagonal blocks of L, then (L dead) P = A⁻¹ in both triangles, and in the final pass the
// np×T block K*ᵀ of the test rows at hand.  W1 holds X = L⁻¹ (lower block triangle; a diagonal
// tile carries explicit zeros above its diagonal).  The padding rows and columns n..np-1 of A are
// those of the identity, so L, X and P are block-diagonal with an identity there: every tile
// product runs over whole tiles without a mask, a padded entry only ever meets an exact zero, and
// every vector pass, sum and contraction is clipped to n.
//
// One evaluation at θ:
//   build      lower tiles of A from the raw features (staged per tile in LDS, 1/ℓ applied on use)
//   factorise  block column kb, left-looking: A_i,kb −= L_i,0:kb L_kb,0:kbᵀ (i >= kb); the diagonal
//              tile through kernels_batch.hip's fused sweep in LDS (Cholesky and X_kk = L_kk⁻¹ at
//              once, two barriers a pivot, the pivot test → info, log L_kk after the sweep);
//              the panel L_i,kb = A_i,kb X_kkᵀ
//   invert     X_ij = −X_ii (Σ_{j<=k<i} L_ik X_kj), row block by row block, the inner sum parked in
//              X_ij's own tile between the two products
//   vectors    β = Xy, α = Xᵀβ, d = colsum(X∘X), the five GPS_OBJ_* entries
//   P = XᵀX    lower tiles (k clipped to >= the row block), stored to both triangles of W0
//   LOO        u, c̃, v = Pu; P diag(c̃) P tile by tile, never stored: the threads that hold a tile
//              of M in their accumulators contract it with ∂A/∂θ on the spot (K_ij and Δ_k² from
//              the features) into the 2 + d sums.  NLML contracts ½(P − ααᵀ) read back from W0.
// The tile product is one device function (tile_mma): operand layouts, the diag(c̃) scaling of the
// k index and the k range are its parameters; each wave owns a 32×32 quadrant (four accumulators),
// operands go through double-buffered k-major LDS images 16 deep, the next slice's global loads
// are issued before the current slice's MFMAs.
// A workspace slice is touched by its own workgroup only, __syncthreads() is all the ordering there
// is; every sum's order is a function of n, d and the 256 threads, so results are bitwise
// independent of the batch size, the problem's position and the launch split.
#pragma once
#include "batch_driver.h"
#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double dv2 __attribute__((ext_vector_type(2)));

constexpr int BT = 256;                  // threads per workgroup: four waves, a 2×2 grid of quadrants
constexpr int T = kBatchFullTallTile;    // tile edge
constexpr int KS = 16;                   // k depth of one staged slice, what slice_load covers
                                         // (32, two loads of it a stage, measured the same)
constexpr int LS = T + 16;               // row stride of a k-major LDS image (≡ 32 dwords mod 64)
constexpr int TL = T + 1;                // row stride of the sweep tile
constexpr int BG = 2 + GPS_BATCH_MAX_D;  // gradient sums: ΣMK, tr M, per-dimension
constexpr int kThDoubles = 40;           // θ (<= 18) then 1/ℓ_k (<= 16) at th + 20
constexpr int kPan = 4 * KS * LS;        // two buffers × (A image, B image)
static_assert((T * TL) % 2 == 0, "the images behind the sweep tile stay 16-byte aligned");
static_assert(T == 64 && BT == 256, "the sweep's 4×4 register tiles and the quadrants assume these");
static_assert(2 * T * (GPS_BATCH_MAX_D + 1) <= kPan, "a tile's two feature panels fit the images");

struct Lds {
  double* tile;   // [T][TL]: the sweep's diagonal tile; the final pass's V tile and its sums
  double* pan;    // the tile product's images; between products a tile's row / column features
  double *y, *beta, *alpha, *dinv, *u, *ct, *v, *piv;  // np doubles each
  double* sw;     // the sweep's row and column, T each
  double* sh;     // block_sum scratch, BG·16
  double* th;     // θ, then 1/ℓ_k at th + 20
};

__device__ __forceinline__ Lds carve(double* sm, int np) {
  Lds s;
  s.tile = sm;
  s.pan = s.tile + T * TL;  // (T·TL is even: the images stay 16-byte aligned)
  s.y = s.pan + kPan;
  s.beta = s.y + np; s.alpha = s.beta + np; s.dinv = s.alpha + np;
  s.u = s.dinv + np; s.ct = s.u + np; s.v = s.ct + np; s.piv = s.v + np;
  s.sw = s.piv + np;
  s.sh = s.sw + 2 * T;
  s.th = s.sh + BG * 16;
  return s;
}

// n rounded up to whole tiles
__host__ __device__ inline int64_t padded(int64_t n) { return T * ((n + T - 1) / T); }

// what the three launchers check alike: the problem's shape, the steps of one launch (`steps`: the
// path's rule, asked only once n is known to be in range) and the workspace
inline bool full_tall_args_ok(const BatchParams& p, int (*steps)(int64_t n), const double* ws,
                              int64_t ws_stride, int64_t ws_need) {
  return p.n >= 1 && p.n <= GPS_BATCH_FULL_TALL_MAX_N && p.d >= 1 && p.d <= GPS_BATCH_MAX_D &&
         p.nprob >= 1 && (p.n_ell == 1 || p.n_ell == p.d) && p.nsteps >= 0 &&
         p.nsteps <= steps(p.n) && ws && ws_stride >= ws_need && !(ws_stride & 3) &&
         !(reinterpret_cast<uintptr_t>(ws) & 31);
}

// what the two VA launchers check on top of it: a training launch with validation rows (§34)
inline bool full_tall_va_args_ok(const BatchParams& p) {
  return p.mode == BATCH_MODE_TRAIN && p.xv && p.yv && p.va_sc && p.nv >= 1 && p.va_every >= 1;
}

// ------------------------------------------------------------------ the fold geometry (§26, §32)
// the tile-aligned column range [klo, khi) that the folds of row tile bi's live rows cover
__device__ __forceinline__ void fold_span(int bi, int n, int nfold, int& klo, int& khi) {
  const int r0 = bi * T, r1 = min(n, r0 + T) - 1;
  int lo = 0, hi = n;
  for (int f = 0; f < nfold; ++f) {
    const int a = fold_begin(f, n, nfold), b = fold_begin(f + 1, n, nfold);
    if (a <= r0 && r0 < b) lo = a;
    if (a <= r1 && r1 < b) hi = b;
  }
  klo = lo / T * T;
  khi = (hi + T - 1) / T * T;
}

// Gblk's zeros: every tile column a row tile's folds touch (ld, nb and t from the caller: §25)
__device__ __forceinline__ void gblk_zero(double* W2, int n, int nfold, int64_t ld, int nb, int t) {
  for (int bi = 0; bi < nb; ++bi) {
    int klo, khi;
    fold_span(bi, n, nfold, klo, khi);
    const int wd = khi - klo;
    for (int e = t; e < T * wd; e += BT) {
      const int i = e / wd, j = e - i * wd;
      W2[(bi * T + i) * ld + klo + j] = 0.0;
    }
  }
}

// ------------------------------------------------------------------ the tile product
// Operand layouts: element (k, x) of an operand — x the row of op(A) or the column of op(B) — is
// at p[k·ld + x] (KMAJ) or at p[x·ld + k] (XMAJ).
enum { KMAJ = 0, XMAJ = 1 };

template <int LAY>
__device__ __forceinline__ void slice_load(const double* p, int64_t ld, int k, dv2 (&r)[2]) {
  const int t = threadIdx.x;
  const double* q = LAY == KMAJ ? p + (int64_t)(k + (t >> 4)) * ld + (t & 15) * 4
                                : p + (int64_t)(t >> 2) * ld + k + (t & 3) * 4;
  r[0] = *reinterpret_cast<const dv2*>(q);
  r[1] = *reinterpret_cast<const dv2*>(q + 2);
}

template <int LAY>
__device__ __forceinline__ void slice_scale(dv2 (&r)[2], const double* scale, int k) {
  const int t = threadIdx.x;
  if (LAY == KMAJ) {
    const double c = scale[k + (t >> 4)];
    r[0] *= c;
    r[1] *= c;
  } else {
    const double* c = scale + k + (t & 3) * 4;
    r[0].x *= c[0]; r[0].y *= c[1]; r[1].x *= c[2]; r[1].y *= c[3];
  }
}

template <int LAY>
__device__ __forceinline__ void slice_store(double* img, const dv2 (&r)[2]) {
  const int t = threadIdx.x;
  if (LAY == KMAJ) {
    double* q = img + (t >> 4) * LS + (t & 15) * 4;
    *reinterpret_cast<dv2*>(q) = r[0];
    *reinterpret_cast<dv2*>(q + 2) = r[1];
  } else {
    double* q = img + (t & 3) * 4 * LS + (t >> 2);
    q[0] = r[0].x; q[LS] = r[0].y; q[2 * LS] = r[1].x; q[3 * LS] = r[1].y;
  }
}

// acc[mi][ni] += Σ_{k0 <= k < k1} opA(i, k) · (SCALE ? scale[k] : 1) · opB(k, j) over one T×T tile:
// this wave's quadrant is rows 32·(wave >> 1) + 16·mi + .., columns 32·(wave & 1) + 16·ni + ..;
// register r of lane l is row (l >> 4) + 4r, column l & 15 of its 16×16 block (the f64 MFMA's own
// map, kernels_gemm.hip).  k1 − k0 is a positive multiple of KS.  Both images must be free on
// entry (every caller arrives synchronised); ends synchronised.
template <int AL, int BL, bool SCALE>
__device__ __forceinline__ void tile_mma(d4 (&acc)[2][2], const double* A, int64_t lda,
                                         const double* B, int64_t ldb, int k0, int k1,
                                         const double* scale, double* pan) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int ro = 32 * (w >> 1) + (lane & 15), co = 32 * (w & 1) + (lane & 15), kq = lane >> 4;
  dv2 ra[2], rb[2];
  slice_load<AL>(A, lda, k0, ra);
  slice_load<BL>(B, ldb, k0, rb);
  if (SCALE) slice_scale<AL>(ra, scale, k0);
  slice_store<AL>(pan, ra);
  slice_store<BL>(pan + KS * LS, rb);
  __syncthreads();
  int buf = 0;
  for (int k = k0; k < k1; k += KS) {
    const bool more = k + KS < k1;
    if (more) {  // the next slice's loads fly over this slice's MFMAs
      slice_load<AL>(A, lda, k + KS, ra);
      slice_load<BL>(B, ldb, k + KS, rb);
    }
    const double* as = pan + buf * 2 * KS * LS;
    const double* bs = as + KS * LS;
#pragma unroll
    for (int s = 0; s < KS / 4; ++s) {
      const double a0 = as[(4 * s + kq) * LS + ro], a1 = as[(4 * s + kq) * LS + ro + 16];
      const double b0 = bs[(4 * s + kq) * LS + co], b1 = bs[(4 * s + kq) * LS + co + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) {  // the other buffer was last read before the previous barrier
      double* an = pan + (buf ^ 1) * 2 * KS * LS;
      if (SCALE) slice_scale<AL>(ra, scale, k + KS);
      slice_store<AL>(an, ra);
      slice_store<BL>(an + KS * LS, rb);
    }
    __syncthreads();
    buf ^= 1;
  }
}

__device__ __forceinline__ void acc_zero(d4 (&acc)[2][2]) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};
}

// this thread's accumulator coordinates inside a tile
__device__ __forceinline__ int acc_row(int mi, int r) {
  const int t = threadIdx.x;
  return 32 * (t >> 7) + 16 * mi + ((t & 63) >> 4) + 4 * r;
}
__device__ __forceinline__ int acc_col(int ni) {
  const int t = threadIdx.x;
  return 32 * ((t >> 6) & 1) + 16 * ni + (t & 15);
}

// C (a tile at c, row stride ld) = sgn·acc, or C −= acc with SUB
template <bool SUB>
__device__ __forceinline__ void acc_store(const d4 (&acc)[2][2], double* c, int64_t ld, double sgn) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* q = c + (int64_t)acc_row(mi, r) * ld + acc_col(ni);
        if (SUB) *q -= acc[mi][ni][r];
        else *q = sgn * acc[mi][ni][r];
      }
}

// ------------------------------------------------------------------ features of a tile
// Raw feature rows r0.. (at most `live` of them, the rest zeros) of src ([..][d]) into dst[T][dp];
// dp is odd so the 16 rows a wave instruction reads fall in different banks.
__device__ __forceinline__ void stage_feat(double* dst, const double* src, int r0, int live, int d,
                                           int dp) {
  for (int e = threadIdx.x; e < T * d; e += BT) {
    const int r = e / d, k = e - r * d;
    dst[r * dp + k] = r < live ? src[(int64_t)(r0 + r) * d + k] : 0.0;
  }
}

__device__ __forceinline__ double sqdist(const double* fi, const double* fj, const double* il,
                                         int d) {
  double r2 = 0.0;
  for (int k = 0; k < d; ++k) {
    const double df = (fi[k] - fj[k]) * il[k];
    r2 = fma(df, df, r2);
  }
  return r2;
}

// ------------------------------------------------------------------ the diagonal tile
// kernels_batch.hip's fused sweep on the nn live rows of the tile in LDS (lower triangle): X_kk =
// L_kk⁻¹ replaces it, L_kk's diagonal goes to piv.  Returns 0, or the 1-based order within the
// tile of the pivot that is not > 0 (a NaN included) — the same value in every thread.  Ends
// synchronised.
__device__ __forceinline__ int sweep(const Lds& s, int nn, double* piv) {
  constexpr int BR = 4;
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15, nb = (nn + 15) >> 4;
  double* A = s.tile;
  double* w = s.sw;       // step k: X_kj/L_kk (j < k), 1/L_kk (j = k), L_jk (j > k)
  double* lc = s.sw + T;  // step k: L_ik (i > k)
  int ci[BR], cj[BR];
#pragma unroll
  for (int a = 0; a < BR; ++a) {
    ci[a] = min(ti + 16 * a, nn - 1);
    cj[a] = min(tj + 16 * a, nn - 1);
  }
  for (int k = 0; k < nn; ++k) {
    const double dk = A[k * TL + k];
    if (!(dk > 0.0)) return k + 1;
    const double is = rsqrt(dk);
    if (t < nn) {
      if (t < k) {
        const double x = A[k * TL + t] * is;
        w[t] = x;
        A[k * TL + t] = x;
      } else if (t == k) {
        w[t] = is;
        piv[k] = dk * is;
      } else {
        const double l = A[t * TL + k] * is;
        w[t] = l;
        lc[t] = l;
        A[t * TL + k] = 0.0;  // the update below then writes X_tk = 0 − L_tk/L_kk like any entry
      }
    }
    __syncthreads();
    if (t == 0) A[k * TL + k] = is;  // row k is not read below, the next pivot is A[k+1][k+1]
    const int kb = k >> 4, k15 = k & 15;
    double wj[BR], nl[BR], old[BR][BR];
#pragma unroll
    for (int a = 0; a < BR; ++a) {
      wj[a] = w[cj[a]];
      nl[a] = -lc[ci[a]];
    }
    // every load first, then the stores (all of it is one LDS array); clamped rows are read and
    // never stored, a diagonal tile's upper half is read and dropped
#pragma unroll
    for (int a = 0; a < BR; ++a)
      if (a >= kb && a < nb) {
#pragma unroll
        for (int b = 0; b < BR; ++b)
          if (b <= a) old[a][b] = A[ci[a] * TL + tj + 16 * b];
      }
#pragma unroll
    for (int a = 0; a < BR; ++a)
      if (a >= kb && a < nb) {
        const int i = ti + 16 * a;
        if (i < nn && (a > kb || ti > k15)) {
#pragma unroll
          for (int b = 0; b < BR; ++b)
            if (b < a || (b == a && tj <= ti))
              A[i * TL + tj + 16 * b] = fma(nl[a], wj[b], old[a][b]);
        }
      }
    __syncthreads();
  }
  return 0;
}

// The factorise and invert steps on any padded sub-workspace: A (nb×nb tiles, row stride ld, the
// lower tiles and whole diagonal tiles given, n live rows, the identity in the padding) → the
// off-diagonal blocks of L in A's place, X = L⁻¹ in the lower block triangle of Xo (same stride),
// L's diagonal in piv[0..n).  Returns 0, or the 1-based order of the leading minor whose pivot is
// not > 0 — the same value in every thread.  Ends synchronised.  These are forward()'s factorise
// and invert steps with the workspace as parameters; forward() keeps its own copy of the text,
// because calling this from it changes batch_full_tall_kernel's register allocation (104 AGPRs
// for 106), and that kernel is to compile as it did.  Keep the two in step.
__device__ __forceinline__ int factor_invert(const Lds& s, double* A, double* Xo, int64_t ld,
                                             int nb, int n, double* piv) {
  const int t = threadIdx.x;
  // factorise, one block column at a time
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = kb * T, nn = min(T, n - k0);
    if (kb > 0) {
      for (int bi = kb; bi < nb; ++bi) {
        d4 acc[2][2];
        acc_zero(acc);
        tile_mma<XMAJ, XMAJ, false>(acc, A + bi * T * ld, ld, A + k0 * ld, ld, 0, k0, nullptr,
                                    s.pan);
        acc_store<true>(acc, A + bi * T * ld + k0, ld, 1.0);
      }
      __syncthreads();
    }
    for (int e = t; e < T * T; e += BT) {
      const int i = e >> 6, j = e & 63;
      s.tile[i * TL + j] = A[(k0 + i) * ld + k0 + j];
    }
    __syncthreads();
    const int bad = sweep(s, nn, piv + k0);
    if (bad) return k0 + bad;
    for (int e = t; e < T * T; e += BT) {
      const int i = e >> 6, j = e & 63;
      Xo[(k0 + i) * ld + k0 + j] = i < nn ? (j <= i ? s.tile[i * TL + j] : 0.0) : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int bi = kb + 1; bi < nb; ++bi) {  // the panel: L_i,kb = A_i,kb X_kkᵀ
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, XMAJ, false>(acc, A + bi * T * ld + k0, ld, Xo + k0 * ld + k0, ld, 0, T,
                                  nullptr, s.pan);
      acc_store<false>(acc, A + bi * T * ld + k0, ld, 1.0);
    }
    __syncthreads();
  }
  // invert: X_ij = −X_ii Σ_{j <= k < i} L_ik X_kj (rows above row block bi are final)
  for (int bi = 1; bi < nb; ++bi)
    for (int bj = 0; bj < bi; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, A + bi * T * ld, ld, Xo + bj * T, ld, bj * T, bi * T,
                                  nullptr, s.pan);
      double* xij = Xo + bi * T * ld + bj * T;
      acc_store<false>(acc, xij, ld, 1.0);
      __syncthreads();
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, Xo + bi * T * ld + bi * T, ld, xij, ld, 0, T, nullptr,
                                  s.pan);
      acc_store<false>(acc, xij, ld, -1.0);
      __syncthreads();
    }
  return 0;
}

// dst = XᵀX for the lower block triangular X (nb×nb tiles, row stride ld for both): lower tiles
// (k clipped to >= the row block, X_k,bi is zero above row block bi), stored to both triangles.
// Ends synchronised.
__device__ __forceinline__ void gram_lower(const Lds& s, const double* X, double* dst, int64_t ld,
                                           int nb) {
  const int np = nb * T;
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<KMAJ, KMAJ, false>(acc, X + bi * T, ld, X + bj * T, ld, bi * T, np, nullptr, s.pan);
      acc_store<false>(acc, dst + bi * T * ld + bj * T, ld, 1.0);
      if (bi != bj) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              dst[(bj * T + acc_col(ni)) * ld + bi * T + acc_row(mi, r)] = acc[mi][ni][r];
      }
    }
  __syncthreads();
}

// A = K + σ²I → X = L⁻¹ in W1 (L's off-diagonal blocks in W0), β, α, d and the objectives.
// Returns 0, or the 1-based order of the leading minor whose pivot is not > 0 — the same value in
// every thread.  Ends synchronised.
__device__ __forceinline__ int forward(const Lds& s, const double* x, double* W0, double* W1, int n,
                                       int np, int d, double sf2, double sn2,
                                       double obj[GPS_N_OBJ]) {
  const int t = threadIdx.x, nb = np / T, dp = d | 1;
  const int64_t ld = np;
  const double* il = s.th + 20;
  double* fi = s.pan;
  double* fj = s.pan + T * dp;
  // build: tile (bi, bj), bj <= bi; a diagonal tile whole (it is symmetric), the padding the identity's
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      stage_feat(fi, x, bi * T, n - bi * T, d, dp);
      stage_feat(fj, x, bj * T, n - bj * T, d, dp);
      __syncthreads();
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(mi, r), gi = bi * T + row;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int col = acc_col(ni), gj = bj * T + col;
            double a;
            if (gi < n && gj < n)
              a = sf2 * exp(-0.5 * sqdist(fi + row * dp, fj + col * dp, il, d)) +
                  (gi == gj ? sn2 : 0.0);
            else
              a = gi == gj ? 1.0 : 0.0;
            W0[gi * ld + gj] = a;
          }
        }
      __syncthreads();
    }
  // factorise, one block column at a time
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = kb * T, nn = min(T, n - k0);
    if (kb > 0) {
      for (int bi = kb; bi < nb; ++bi) {
        d4 acc[2][2];
        acc_zero(acc);
        tile_mma<XMAJ, XMAJ, false>(acc, W0 + bi * T * ld, ld, W0 + k0 * ld, ld, 0, k0, nullptr,
                                    s.pan);
        acc_store<true>(acc, W0 + bi * T * ld + k0, ld, 1.0);
      }
      __syncthreads();
    }
    for (int e = t; e < T * T; e += BT) {
      const int i = e >> 6, j = e & 63;
      s.tile[i * TL + j] = W0[(k0 + i) * ld + k0 + j];
    }
    __syncthreads();
    const int bad = sweep(s, nn, s.piv + k0);
    if (bad) return k0 + bad;
    for (int e = t; e < T * T; e += BT) {
      const int i = e >> 6, j = e & 63;
      W1[(k0 + i) * ld + k0 + j] = i < nn ? (j <= i ? s.tile[i * TL + j] : 0.0) : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int bi = kb + 1; bi < nb; ++bi) {  // the panel: L_i,kb = A_i,kb X_kkᵀ
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, XMAJ, false>(acc, W0 + bi * T * ld + k0, ld, W1 + k0 * ld + k0, ld, 0, T,
                                  nullptr, s.pan);
      acc_store<false>(acc, W0 + bi * T * ld + k0, ld, 1.0);
    }
    __syncthreads();
  }
  // invert: X_ij = −X_ii Σ_{j <= k < i} L_ik X_kj (rows above row block bi are final)
  for (int bi = 1; bi < nb; ++bi)
    for (int bj = 0; bj < bi; ++bj) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, W0 + bi * T * ld, ld, W1 + bj * T, ld, bj * T, bi * T,
                                  nullptr, s.pan);
      double* xij = W1 + bi * T * ld + bj * T;
      acc_store<false>(acc, xij, ld, 1.0);
      __syncthreads();
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, W1 + bi * T * ld + bi * T, ld, xij, ld, 0, T, nullptr,
                                  s.pan);
      acc_store<false>(acc, xij, ld, -1.0);
      __syncthreads();
    }
  // β = Xy: a wave per row, lanes over the columns
  {
    const int lane = t & 63, wv = t >> 6;
    for (int i = wv; i < n; i += BT / 64) {
      double b = 0.0;
      for (int j = lane; j <= i; j += 64) b = fma(W1[i * ld + j], s.y[j], b);
      b = wave_sum(b);
      if (lane == 0) s.beta[i] = b;
    }
  }
  __syncthreads();
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // Σ crps, Σ logs, Σ β², Σ log L_kk
  for (int j = t; j < n; j += BT) {    // α = Xᵀβ, d = colsum(X∘X): a thread per column
    double a = 0.0, dj = 0.0;
#pragma unroll 4
    for (int i = j; i < n; ++i) {
      const double xv = W1[i * ld + j];
      a = fma(xv, s.beta[i], a);
      dj = fma(xv, xv, dj);
    }
    s.alpha[j] = a;
    s.dinv[j] = dj;
    const double yy = s.y[j], m = yy - a / dj, c = 1.0 / dj;
    v[0] += crps_term(m, c, yy);
    v[1] += logs_term(m, c, yy);
    v[2] += s.beta[j] * s.beta[j];
    v[3] += log(s.piv[j]);
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

// The threads that hold lower tile (bi, bj) of a product in their accumulators contract M with
// ∂A/∂θ on the spot into g (K_ij and Δ_k² from the features, staged here): with vab, M_ij =
// −acc_ij − ½(v_iα_j + α_iv_j) (the LOO and block-LOO form), without, ½(acc_ij − α_iα_j) (NLML).
// The images must be free on entry; ends synchronised.
__device__ __forceinline__ void contract_tile(const Lds& s, const double* x, const d4 (&acc)[2][2],
                                              int bi, int bj, int n, int d, double sf2, bool vab,
                                              double (&g)[BG]) {
  const int dp = d | 1;
  const double* il = s.th + 20;
  double* fi = s.pan;
  double* fj = s.pan + T * dp;
  stage_feat(fi, x, bi * T, n - bi * T, d, dp);
  stage_feat(fj, x, bj * T, n - bj * T, d, dp);
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = acc_row(mi, r), i = bi * T + row;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = acc_col(ni), j = bj * T + col;
        if (i >= n || j > i) continue;  // (j <= i < n; an off-diagonal tile lies below whole)
        const double* xi = fi + row * dp;
        const double* xj = fj + col * dp;
        const double K = sf2 * exp(-0.5 * sqdist(xi, xj, il, d));
        const double ai = s.alpha[i], aj = s.alpha[j], pij = acc[mi][ni][r];
        const double m = vab ? fma(-0.5, s.v[i] * aj + ai * s.v[j], -pij)
                             : 0.5 * (pij - ai * aj);
        const double mk = (i == j ? 1.0 : 2.0) * m * K;  // the lower triangle stands for both
        g[0] += mk;
        if (i == j) g[1] += m;
#pragma unroll
        for (int q = 0; q < GPS_BATCH_MAX_D; ++q)
          if (q < d) {
            const double df = (xi[q] - xj[q]) * il[q];
            g[2 + q] = fma(mk, df * df, g[2 + q]);
          }
      }
    }
  __syncthreads();
}

// After forward(): g = [ΣMK, tr M, ΣMKΔ_k²/ℓ_k² (k < d)] over the full symmetric M, valid in every
// thread.  Overwrites W0 (L) with P.  Ends synchronised.
__device__ __forceinline__ void gradient(const Lds& s, const double* x, double* W0,
                                         const double* W1, int n, int np, int d, int objective,
                                         double sf2, double (&g)[BG]) {
  const int t = threadIdx.x, nb = np / T;
  const int64_t ld = np;
  const bool loo = objective != GPS_OBJ_NLML;
  if (loo)
    for (int j = t; j < np; j += BT) {  // score_derivs of the MEAN score, then u and c̃
      double uu = 0.0, cc = 0.0;       // (the padding scales P's identity block away)
      if (j < n) {
        const double dd = s.dinv[j], a = s.alpha[j];
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
        uu = -gm / dd;
        cc = (gm * a - gc) / (dd * dd);
      }
      s.u[j] = uu;
      s.ct[j] = cc;
    }
  gram_lower(s, W1, W0, ld, nb);  // P = XᵀX
  if (loo) {
    for (int i = t; i < n; i += BT) {  // v = Pu: a thread per column of the symmetric P
      double vv = 0.0;
#pragma unroll 4
      for (int j = 0; j < n; ++j) vv = fma(W0[j * ld + i], s.u[j], vv);
      s.v[i] = vv;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < BG; ++q) g[q] = 0.0;
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      d4 acc[2][2];  // (P diag(c̃) P)_ij, or P_ij
      if (loo) {
        acc_zero(acc);
        tile_mma<KMAJ, KMAJ, true>(acc, W0 + bi * T, ld, W0 + bj * T, ld, 0, np, s.ct, s.pan);
      } else {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc[mi][ni][r] = W0[(bi * T + acc_row(mi, r)) * ld + bj * T + acc_col(ni)];
      }
      contract_tile(s, x, acc, bi, bj, n, d, sf2, loo, g);
    }
  block_sum<BG>(g, s.sh);
}

// The block-LOO objectives' gradient() (kernels_batch_full_tall_block.hip), which only
// the BLOCK instantiation of tall_body calls: the objective's value (and the folds' values to
// fold_values where given) and g as gradient(); W2 is the third workspace array.  Returns 0, or n
// + the 1-based global row whose pivot in its fold's P_f is not > 0.
__device__ __forceinline__ int block_gradient(const Lds& s, const double* x, double* W0,
                                              double* W1, double* W2, int n, int np, int d,
                                              int objective, int nfold, double sf2,
                                              double (&g)[BG], double& value, double* fold_values);

// The predictive at `cnt` rows `rows` ([cnt][d]) after forward(): X in W1, α in LDS, W0 free (L is
// dead).  Rows in blocks of T: K*ᵀ (np×T, zero in the padding) into the first T columns of W0, V =
// X K*ᵀ tile by tile, μ* = k*·α, var* = σ² + sf² − the column norms of V; thread (grp, c) sums the
// rows of column c that fall to its group, the four groups are added in order.  μ* / var* go to
// mu / var where given, and with targets `yr` each row's six score terms are added to thread c's
// sums.  This is the final pass's test-row loop in tall_body (which keeps its own copy of the text,
// as forward() keeps factor_invert's: the VA = false kernels are to compile as they did, DESIGN
// §34) — keep the two in step, a validation row is bitwise a test row of an itr = 0 call.  Scratch:
// s.tile, s.pan and those columns of W0; nothing either gradient reads.  The caller arrives
// synchronised; ends synchronised.
__device__ __forceinline__ void predict_rows(const Lds& s, const double* x, double* W0,
                                             const double* W1, int n, int np, int d, double sf2,
                                             double sn2, const double* rows, const double* yr,
                                             int cnt, double* mu_out, double* var_out, double ymean,
                                             double yvar, double triv_c, double (&sums)[6]) {
  const int t = threadIdx.x, nb = np / T, dp = d | 1;
  const int64_t ld = np;
  const double* il = s.th + 20;
  const int grp = t >> 6, c = t & 63;
  double* fi = s.pan;
  double* fj = s.pan + T * dp;
  for (int c0 = 0; c0 < cnt; c0 += T) {
    const int ntb = min(T, cnt - c0);
    for (int bi = 0; bi < nb; ++bi) {
      stage_feat(fi, x, bi * T, n - bi * T, d, dp);
      stage_feat(fj, rows, c0, ntb, d, dp);
      __syncthreads();
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(mi, r), gi = bi * T + row;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int col = acc_col(ni);
            W0[gi * ld + col] = gi < n && col < ntb
                ? sf2 * exp(-0.5 * sqdist(fi + row * dp, fj + col * dp, il, d)) : 0.0;
          }
        }
      __syncthreads();
    }
    double mu = 0.0, q = 0.0;
    for (int i = grp; i < n; i += BT / 64) mu = fma(W0[i * ld + c], s.alpha[i], mu);
    for (int bi = 0; bi < nb; ++bi) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, W1 + bi * T * ld, ld, W0, ld, 0, (bi + 1) * T, nullptr,
                                  s.pan);
      acc_store<false>(acc, s.tile, TL, 1.0);
      __syncthreads();
      for (int r = grp * 16; r < grp * 16 + 16; ++r) {
        const double vv = s.tile[r * TL + c];
        q = fma(vv, vv, q);
      }
      __syncthreads();
    }
    s.tile[t] = mu;
    s.tile[BT + t] = q;
    __syncthreads();
    if (t < ntb) {
      double m = 0.0, qq = 0.0;
      for (int w = 0; w < BT / 64; ++w) {
        m += s.tile[w * 64 + t];
        qq += s.tile[BT + w * 64 + t];
      }
      const double cv = (sn2 + sf2) - qq;
      if (mu_out) {
        mu_out[c0 + t] = m;
        var_out[c0 + t] = cv;
      }
      if (yr) {
        const double yv = yr[c0 + t];
        score_row_add(sums, m, cv, yv, ymean, yvar, triv_c);
      }
    }
    __syncthreads();
  }
}

// batch_driver.h's scores_store with the destination and the row count as parameters: the block's
// six sums → six GPS_SC_* entries at sc (one thread)
__device__ __forceinline__ void scores_store_to(double* sc, double cnt, const double (&tot)[6]) {
  sc[GPS_SC_CRPS] = tot[0] / cnt;
  sc[GPS_SC_LOGS] = tot[1] / cnt;
  sc[GPS_SC_MSLL] = tot[2] / cnt;
  sc[GPS_SC_SMSE] = tot[3] / tot[4];
  sc[GPS_SC_MSE] = tot[3] / cnt;
  sc[GPS_SC_COVER] = tot[5] / cnt;
}

// A kernel's whole body: the SGD loop (or the one evaluation of BATCH_MODE_GRAD), the final pass
// and the outputs.  BLOCK: the objective is GPS_BLOCK_DSS / GPS_BLOCK_KC over nfold folds, the
// workspace has a third array behind W1 (w1 doubles), and BATCH_MODE_GRAD also writes value and
// fold_values; without it those four arguments are unused.
//
// VA (BATCH_MODE_TRAIN only): the problem's validation rows p.xv / p.yv (nv of them)
// are scored inside the fit.  A training step whose global index i = step0 + st is a multiple of
// p.va_every is a checkpoint: between forward() and the gradient — X in W1, α in LDS, W0 free until
// the gradient rebuilds it — predict_rows forms the predictive at the validation rows at that
// forward's parameters (θ before step i, its own σ²) and the six GPS_SC_* entries go to
// va_sc[pb][i / va_every].  The final pass adds row nva − 1 (nva = ceil(itr / va_every) + 1) at its
// own parameters (so with stale_noise its σ² is the stale one), then the test rows; both run
// inside the step loop, through the one call of predict_rows.  A failed problem gets NaN in every
// row from the first checkpoint it did not reach.  Without VA the body is the text it was.
template <bool BLOCK, bool VA = false>
__device__ __forceinline__ void tall_body(const BatchParams& p, double* ws, int64_t ws_stride,
                                          int nfold, int64_t w1, double* value,
                                          double* fold_values) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = p.n, d = p.d, t = threadIdx.x;
  const int np = T * ((n + T - 1) / T), nb = np / T, dp = d | 1;
  const int64_t ld = np;
  const int nth = 2 + p.n_ell;
  const int64_t pb = blockIdx.x;
  const Lds s = carve(sm, np);
  double* il = s.th + 20;
  const double* x = p.x + pb * n * d;
  double* W0 = ws + pb * ws_stride;
  double* W1 = W0 + ld * ld;
  int info = p.info[pb];
  int done = p.steps_done[pb];
  double stale = p.stale[pb];
  for (int e = t; e < n; e += BT) s.y[e] = p.y[pb * n + e];
  if (t < nth) s.th[t] = p.theta[pb * nth + t];
  const double bscale = p.kind == GPS_RBF ? 0.5 : 1.0;
  double obj[GPS_N_OBJ];
  // the training steps of this launch, then (do_final) one more forward: the final pass at the
  // final kernel parameters, whose noise is the final σ² or, with stale_noise, the σ² the last
  // step's forward used
  const int ntrain = p.mode == BATCH_MODE_GRAD ? 1 : p.nsteps;
  const int neval = ntrain + (p.mode == BATCH_MODE_TRAIN && p.do_final ? 1 : 0);
  double sf2 = 0.0, sn2 = 0.0;
  // VA: the train-target mean and unbiased variance once a launch, in gps_full_set_data's order
  // (the final pass's own lines below), and the first step whose checkpoint is still to come
  [[maybe_unused]] double va_ymean = 0.0, va_yvar = 0.0, va_triv = 0.0;
  [[maybe_unused]] int va_reach = done > p.step0 ? done : p.step0;
  if constexpr (VA) {
    __syncthreads();  // y is visible
    double ysum = 0.0, yss = 0.0;
    for (int i = 0; i < n; ++i) ysum += s.y[i];
    va_ymean = ysum / n;
    for (int i = 0; i < n; ++i) yss += (s.y[i] - va_ymean) * (s.y[i] - va_ymean);
    va_yvar = yss / (n - 1);
    va_triv = 0.5 * log(6.28318530717958647692 * va_yvar);
  }
  for (int st = 0; st < neval && info == 0; ++st) {
    const bool fin = st == ntrain;
    __syncthreads();  // θ (loaded, or the previous step's update) is visible
    const double lsn = s.th[nth - 1];
    sf2 = exp(s.th[0]);
    sn2 = exp(fin && p.stale_noise ? stale : lsn);
    const double bq = t < d ? s.th[1 + (p.n_ell == 1 ? 0 : t)] : 0.0;
    if (t < d) il[t] = p.kind == GPS_ARD ? exp(-bq) : exp(-0.5 * bq);
    __syncthreads();
    if (!fin) stale = lsn;
    info = forward(s, x, W0, W1, n, np, d, sf2, sn2, obj);
    if constexpr (VA) {
      // a checkpoint's validation rows (sums only); in the final pass the last validation row,
      // then the test rows (μ / var stored, scored with yt)
      const int gi = p.step0 + st;
      const int64_t nva = (p.itr + p.va_every - 1) / p.va_every + 1;
      const bool pred = p.xt != nullptr && p.nt > 0;
      const int npass = info ? 0 : fin ? (pred ? 2 : 1) : gi % p.va_every == 0 ? 1 : 0;
      for (int ps = 0; ps < npass; ++ps) {
        const bool te = ps == 1;
        const double* yr = te ? (p.yt ? p.yt + pb * p.nt : nullptr) : p.yv + pb * p.nv;
        const int cnt = te ? p.nt : p.nv;
        double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // as score_rows_kernel; thread c's rows
        predict_rows(s, x, W0, W1, n, np, d, sf2, sn2,
                     te ? p.xt + pb * p.nt * d : p.xv + pb * p.nv * d, yr, cnt,
                     te ? p.mu + pb * p.nt : nullptr, te ? p.var + pb * p.nt : nullptr, va_ymean,
                     va_yvar, va_triv, sums);
        if (!yr) continue;
        block_sum<6>(sums, s.sh);
        if (t == 0)
          scores_store_to(te ? p.sc + pb * GPS_N_SC
                             : p.va_sc + (pb * nva + (fin ? nva - 1 : gi / p.va_every)) * GPS_N_SC,
                          (double)cnt, sums);
      }
      if (!info && !fin) va_reach = gi + 1;
    }
    if (info || fin) break;
    double g[BG];
    double bval = 0.0;
    if constexpr (BLOCK) {
      info = block_gradient(s, x, W0, W1, W1 + w1, n, np, d, p.objective, nfold, sf2, g, bval,
                            p.mode == BATCH_MODE_GRAD && fold_values ? fold_values + pb * nfold
                                                                     : nullptr);
      if (info) break;
    } else {
      gradient(s, x, W0, W1, n, np, d, p.objective, sf2, g);
    }
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
        if constexpr (BLOCK) value[pb] = bval;
      } else {
        const int64_t si = pb * p.itr + p.step0 + st;
        if constexpr (BLOCK)
          p.values[si] = bval;
        else
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
    if constexpr (BLOCK)
      if (info) {
        if (t == 0) value[pb] = batch_nan();
        if (fold_values && t < nfold) fold_values[pb * nfold + t] = batch_nan();
      }
    return;
  }
  train_write_back<BT>(p, pb, t, s.th, nullptr, info, done, stale);
  if (t == 0) p.info[pb] = info;
  if constexpr (VA) {
    // a failed problem (in this launch or an earlier one): NaN in this launch's checkpoint rows
    // from the first it did not reach, and in the final row; train_write_back's rule for values
    if (info) {
      const int64_t nva = (p.itr + p.va_every - 1) / p.va_every + 1;
      const int64_t r0 = (va_reach + p.va_every - 1) / p.va_every;
      const int64_t r1 = p.do_final ? nva : (p.step0 + p.nsteps + p.va_every - 1) / p.va_every;
      for (int64_t e = r0 * GPS_N_SC + t; e < r1 * GPS_N_SC; e += BT)
        p.va_sc[pb * nva * GPS_N_SC + e] = batch_nan();
    }
    // the final pass's rows ran inside the step loop
    if (p.do_final) final_outputs<BT>(p, pb, t, info, p.xt != nullptr && p.nt > 0, obj);
    return;
  }
  if (!p.do_final) return;
  const bool pred = p.xt != nullptr && p.nt > 0;
  if (!final_outputs<BT>(p, pb, t, info, pred, obj)) return;
  // train-target mean and unbiased variance, in gps_full_set_data's order
  double ysum = 0.0, yss = 0.0;
  for (int i = 0; i < n; ++i) ysum += s.y[i];
  const double ymean = ysum / n;
  for (int i = 0; i < n; ++i) yss += (s.y[i] - ymean) * (s.y[i] - ymean);
  const double yvar = yss / (n - 1);
  const double triv_c = 0.5 * log(6.28318530717958647692 * yvar);
  // test rows in blocks of T: K*ᵀ (np×T, zero in the padding) into W0 (L is dead), V = X K*ᵀ
  // tile by tile, μ* = k*·α, var* = σ² + sf² − the column norms of V.  Thread (grp, c) sums the
  // rows of column c that fall to its group; the four groups are added in order.
  const int grp = t >> 6, c = t & 63;
  const double* xt = p.xt + pb * p.nt * d;
  double* fi = s.pan;
  double* fj = s.pan + T * dp;
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // as score_rows_kernel; thread c's rows
  __syncthreads();
  for (int c0 = 0; c0 < p.nt; c0 += T) {
    const int ntb = min(T, p.nt - c0);
    for (int bi = 0; bi < nb; ++bi) {
      stage_feat(fi, x, bi * T, n - bi * T, d, dp);
      stage_feat(fj, xt, c0, ntb, d, dp);
      __syncthreads();
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(mi, r), gi = bi * T + row;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int col = acc_col(ni);
            W0[gi * ld + col] = gi < n && col < ntb
                ? sf2 * exp(-0.5 * sqdist(fi + row * dp, fj + col * dp, il, d)) : 0.0;
          }
        }
      __syncthreads();
    }
    double mu = 0.0, q = 0.0;
    for (int i = grp; i < n; i += BT / 64) mu = fma(W0[i * ld + c], s.alpha[i], mu);
    for (int bi = 0; bi < nb; ++bi) {
      d4 acc[2][2];
      acc_zero(acc);
      tile_mma<XMAJ, KMAJ, false>(acc, W1 + bi * T * ld, ld, W0, ld, 0, (bi + 1) * T, nullptr,
                                  s.pan);
      acc_store<false>(acc, s.tile, TL, 1.0);
      __syncthreads();
      for (int r = grp * 16; r < grp * 16 + 16; ++r) {
        const double vv = s.tile[r * TL + c];
        q = fma(vv, vv, q);
      }
      __syncthreads();
    }
    s.tile[t] = mu;
    s.tile[BT + t] = q;
    __syncthreads();
    if (t < ntb) {
      double m = 0.0, qq = 0.0;
      for (int w = 0; w < BT / 64; ++w) {
        m += s.tile[w * 64 + t];
        qq += s.tile[BT + w * 64 + t];
      }
      const double cv = (sn2 + sf2) - qq;
      const int64_t row = pb * p.nt + c0 + t;
      p.mu[row] = m;
      p.var[row] = cv;
      if (p.yt) {
        const double yv = p.yt[row];
        score_row_add(sums, m, cv, yv, ymean, yvar, triv_c);
      }
    }
    __syncthreads();
  }
  if (!p.yt) return;
  block_sum<6>(sums, s.sh);
  if (t == 0) {
    scores_store(p, pb, sums);
  }
}

}  // namespace

}  // namespace gps
