// Internal declarations shared by the gfx950 kernels and the C-ABI layer.
// Everything here is float64; all device matrices are row-major and every
// dimension handed to a kernel is padded to a multiple of GPS_TILE (128).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dag_task.h"

#define GPS_TILE 128
#define GPS_MAX_D 64

namespace gps {

inline int64_t pad_to(int64_t n, int64_t t = GPS_TILE) { return (n + t - 1) / t * t; }

// ---------------------------------------------------------------- kernel params
struct GramParams {
  const double* x;    // [n][d] raw features
  const double* xp;   // [m][d]
  double* out;        // [M_pad][ldo]
  int64_t ldo;
  int n, m;           // real rows / cols
  int M, N;           // padded rows / cols written
  int d;
  double sf2;
  double diag_add;    // added where i == j (real rows)
  int lower;          // write only j <= i (tile-granular skip + element mask)
  int pad_identity;   // 1.0 on the padded diagonal (i == j >= n)
  double inv_ell[GPS_MAX_D];
  int edge;           // (launch_gram) the diagonal-tile launch of a d = 16 build (kernels_gram.hip)
};

enum Layout { LAY_N = 0, LAY_T = 1 };
// triangular structure of an operand, expressed as a k-range restriction per tile
enum Tri {
  TRI_NONE = 0,
  TRI_K_LE_I = 1,  // k < (ti+1)*128   (A lower, A[i][k] != 0 only for k <= i)
  TRI_K_LE_J = 2,  // k < (tj+1)*128   (B = Lᵀ with L lower stored [j][k])
  TRI_K_GE_J = 3,  // k >= tj*128      (B lower stored [k][j])
  TRI_K_GE_I = 4,  // k >= ti*128      (A = Lᵀ with L lower stored [k][i])
  TRI_KR_J = 5,    // k in [kr[2g], kr[2g'+1]) over the 16-column groups g..g' of the tile
                   // (B block-diagonal with unaligned blocks: block-LOO gradients)
};
enum Epi { EPI_STORE = 0, EPI_ROWSQ = 1, EPI_COLRED = 2, EPI_ROWSQ_DOT = 3 };
// EPI_ROWSQ_DOT: EPI_ROWSQ plus, in the last column tile (the full K range), out1[row] = A[row,:]·w

struct GemmParams {
  const double* A; int64_t lda;
  const double* B; int64_t ldb;
  double* C; int64_t ldc;
  int64_t c_kslice_stride;   // split-K: slice s writes C + s*stride (beta must be 0)
  int M, N, K;               // multiples of 128 (K: multiple of 16 after tri clipping)
  double alpha, beta;
  const double* kscale;      // optional per-k scale applied to A (length K)
  const double* w;           // EPI_COLRED weights (length M)
  double* out0; double* out1; int64_t ld_out;
  int lower_out;             // enumerate only tiles with tj <= ti
  int ksplit;                // number of K slices (grid.y)
  int tri;
  int tri_off;               // global index of output row / column 0 for the tri clipping (a
                             // row or column block of a larger triangular product)
  const int* kr;            // TRI_KR_J: per 16-column group [k begin, k end) (multiples of 16)
  int tiles_m, tiles_n;
  int map_mode;              // tile order: 0 auto (see tile_of), 1 grouped raster only, 2 + XCD remap,
                             // 3 XCD-banded heaviest-first (auto for triangular), 4 pre-3 auto,
                             // 5 XCD-banded 8×8 patches, 6 paired column tiles (EPI_ROWSQ*)
  int tile;                  // output tile edge: 0 auto (gemm_plan), 64 or 128
  double* ws;                // split-K workspace: slabs + ordered reduction (auto plan only
  int64_t ws_cap;            //   splits while ksplit*M*N <= ws_cap doubles)
  int* sk_cnt;               // stream-K tail (launch_gemm): per-tile arrival tickets, zero at the
                             // launch and left zero; partial tiles go to ws.  NULL: no stream-K
  int sk_slots;              // workgroup slots of the chip (2 per CU for the 128-tile kernel)
  // set by launch_gemm for the stream-K tail: tiles [sk_dp, tiles) are split over sk_wgs blocks
  int sk_dp, sk_wgs;
  int prio;                  // 1: the mainloop's MFMA phase at raised wave priority (launch_gemm)
  int mirror;                // lower_out square launch: also write the strictly-lower 32-tiles'
                             // transposes above the diagonal (a symmetric result, in the split-K
                             // reduction when there is one, else by launch_sym_mirror)
  int slab_xcd;              // set by launch_gemm (g_slab_xcd): a split-K grid's (tile, slice)
                             // pairs dealt slice-major in contiguous runs per XCD
  int kend;                  // > 0 (a multiple of 16): A's columns k >= kend are zero (the FITC row
                             // norms: kend = m rounded to 16) — the K loop stops there
  int m_live, n_live;        // > 0 (multiples of 16): the caller's promise that output rows >=
                             // m_live are exact zeros before alpha/beta, resp. that output columns
                             // >= n_live are exact zeros there or never read (padding rows /
                             // columns whose operand rows are zero) — a 64/128-tile that crosses
                             // the extent skips the MFMA blocks beyond it (gemm_tile's edge loop;
                             // GPS_OPT_GEMM_LIVE).  0: the whole extent
  int sk_alone;              // the launch runs without a concurrent forked product (potrf_inv_rec's
                             // trailing update when nothing is forked beside it): the stream-K
                             // tail fills its last round (GPS_OPT_STREAM_K = 2, the default)
  int pipe;                  // 1: full 128-tiles of the store and column-reduction kernels run the
                             // pipelined steady-state loop (LDS stores under the MFMAs, issue
                             // order pinned: gemm_tile's mainloop_pipe; GPS_OPT_GEMM_PIPE, DESIGN
                             // §38).  Set by gemm(); cleared by launch_gemm where that loop is not
                             // compiled (64-tiles, the small kernel, the row-norm epilogues) or
                             // not taken (k-scaled launches, priority off).  Same bits either way
  // Row norms behind a running persistent factorisation (EPI_ROWSQ, TRI_K_LE_J, tri_off 0, 128
  // tiles, no split): column tile j needs row tile j of L⁻¹ only.
  //   dep_mode 1 (the dependent launch): each workgroup takes the heaviest column tile whose row
  //     is final (dep_sig[kSigRdy + j]) from the per-XCD queues dep_q, waiting for a row only once
  //     every workgroup of the factorisation has started (dep_sig[kSigStarted] >= dep_grid: they
  //     are resident, so the wait cannot starve them); otherwise it leaves the tile to
  //   dep_mode 2 (the completion launch, stream-ordered after the factorisation): block b is tile
  //     (b % tiles_m, tiles_n − 1 − b / tiles_m), skipped if the dependent launch took it.
  int* dep_sig; int* dep_q; int* dep_err; int dep_grid; int dep_mode;
};
// The signal block of a persistent factorisation with a dependent row-norm launch (int words,
// zeroed before the pair is launched; DagParams::sig, GemmParams::dep_sig / dep_q)
constexpr int kSigStarted = 0;   // workgroups of the factorisation that have started
constexpr int kSigRowCnt = 64;   // [64] per row tile of L⁻¹: FIN strips completed
constexpr int kSigRdy = 128;     // [64] per row tile: 1 once the row of L⁻¹ is final (2: and
                                 // every band of that column taken by the dependent launch)
constexpr int kSigQueue = 192;   // [8 XCDs][64 column tiles] queue heads of one dependent launch
constexpr int kSigInts = kSigQueue + 8 * 64;

// launch shape chosen for a GEMM (tile edge, K slices); exposed for the microbenchmark
struct GemmPlan { int tile, ksplit; };
GemmPlan gemm_plan(int epi, const GemmParams& p, int64_t ws_cap_doubles);
// what launch_gemm chose for one launch (diagnostics: gps_gemm_diag hands it to the tests, which
// assert the variant they name is the one that ran): tile edge (16/32: the small kernel), K slices
// (small kernel: waves per block), the tile order after the automatic choice, the stream-K tail's
// data-parallel tiles and workgroups (0: no tail), the slice-major XCD deal, the kernel's grid
struct GemmLaunchInfo { int tile, ksplit, map_mode, sk_dp, sk_wgs, slab_xcd, grid_x, grid_y; };
extern int g_gram_reg;   // 1: d in {1, 8, 16} Gram builds use the register-resident kernel; 2 (the
                         //    default): d in {8, 16} builds of every shape (square lower ones such
                         //    as K_ff and K̃mm included) on the matrix-core kernel — equal to 1
                         //    within the centred expansion's rounding, not bitwise (so K̃mm's
                         //    diagonal tiles are not bitwise symmetric there); d = 1 as in 1
extern int g_tiny_gemm;  // 1: the bottom-of-recursion GEMMs use the small kernel (gemm_plan)
extern int g_stream_k;   // stream-K tail of uniform-K 128-tile launches (launch_gemm): 0 never,
                         // 1 every eligible launch, 2 (default) those marked sk_alone
extern int g_slab_xcd;   // split-K launches: each XCD runs whole K slices (GPS_OPT_SLAB_XCD)
constexpr int kStreamKTiles = 4096;  // tickets per stream-K counter array (GemmParams::sk_cnt)

// ------------------------------------------------------------ device reductions
// fixed-order wave / block sums (no atomics anywhere: results are bitwise reproducible)
#ifdef __HIPCC__
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// block-wide sum of NV values per thread; result valid in every thread
template <int NV>
__device__ void block_sum(double (&v)[NV], double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < NV; ++q) sh[q * 16 + wave] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += sh[q * 16 + w];
    v[q] = t;
  }
  __syncthreads();
}

// exp(x) for x <= 0 — the Gaussian kernel's exp(−½r²) — table-driven (round 4): x = (j/64)·ln2 + r
// with j = rint(64x/ln2), |r| <= ln2/128 (Cody–Waite: ln2/64 as a 35-bit head, exact for
// |j| <= 2^17, plus a tail), exp(x) = 2^(j>>6) · 2^((j&63)/64) · e^r, e^r − 1 by its degree-5
// Taylor polynomial (truncation 3.5e-17), 2^(i/64) as a head/tail pair (the table below, from
// 200-bit arithmetic).  About 12 fp64 VALU operations and one LDS read against ~25 for the
// library exp, whose overflow / underflow selects a non-positive argument never needs; within
// 1 ulp of exp.  x < −746 gives 0 (as exp), a NaN propagates.  The table is staged in LDS by
// each kernel (exp_tab_stage) so the per-lane index is a conflict-light ds_read_b128.
__constant__ static const double g_exp_tab[64][2] = {
    {0x1.0000000000000p+0, 0x0.0p+0}, {0x1.02c9a3e778061p+0, -0x1.19083535b085dp-56},
    {0x1.059b0d3158574p+0, 0x1.d73e2a475b465p-55}, {0x1.0874518759bc8p+0, 0x1.186be4bb284ffp-57},
    {0x1.0b5586cf9890fp+0, 0x1.8a62e4adc610bp-54}, {0x1.0e3ec32d3d1a2p+0, 0x1.03a1727c57b53p-59},
    {0x1.11301d0125b51p+0, -0x1.6c51039449b3ap-54}, {0x1.1429aaea92de0p+0, -0x1.32fbf9af1369ep-54},
    {0x1.172b83c7d517bp+0, -0x1.19041b9d78a76p-55}, {0x1.1a35beb6fcb75p+0, 0x1.e5b4c7b4968e4p-55},
    {0x1.1d4873168b9aap+0, 0x1.e016e00a2643cp-54}, {0x1.2063b88628cd6p+0, 0x1.dc775814a8495p-55},
    {0x1.2387a6e756238p+0, 0x1.9b07eb6c70573p-54}, {0x1.26b4565e27cddp+0, 0x1.2bd339940e9d9p-55},
    {0x1.29e9df51fdee1p+0, 0x1.612e8afad1255p-55}, {0x1.2d285a6e4030bp+0, 0x1.0024754db41d5p-54},
    {0x1.306fe0a31b715p+0, 0x1.6f46ad23182e4p-55}, {0x1.33c08b26416ffp+0, 0x1.32721843659a6p-54},
    {0x1.371a7373aa9cbp+0, -0x1.63aeabf42eae2p-54}, {0x1.3a7db34e59ff7p+0, -0x1.5e436d661f5e3p-56},
    {0x1.3dea64c123422p+0, 0x1.ada0911f09ebcp-55}, {0x1.4160a21f72e2ap+0, -0x1.ef3691c309278p-58},
    {0x1.44e086061892dp+0, 0x1.89b7a04ef80d0p-59}, {0x1.486a2b5c13cd0p+0, 0x1.3c1a3b69062f0p-56},
    {0x1.4bfdad5362a27p+0, 0x1.d4397afec42e2p-56}, {0x1.4f9b2769d2ca7p+0, -0x1.4b309d25957e3p-54},
    {0x1.5342b569d4f82p+0, -0x1.07abe1db13cadp-55}, {0x1.56f4736b527dap+0, 0x1.9bb2c011d93adp-54},
    {0x1.5ab07dd485429p+0, 0x1.6324c054647adp-54}, {0x1.5e76f15ad2148p+0, 0x1.ba6f93080e65ep-54},
    {0x1.6247eb03a5585p+0, -0x1.383c17e40b497p-54}, {0x1.6623882552225p+0, -0x1.bb60987591c34p-54},
    {0x1.6a09e667f3bcdp+0, -0x1.bdd3413b26456p-54}, {0x1.6dfb23c651a2fp+0, -0x1.bbe3a683c88abp-57},
    {0x1.71f75e8ec5f74p+0, -0x1.16e4786887a99p-55}, {0x1.75feb564267c9p+0, -0x1.0245957316dd3p-54},
    {0x1.7a11473eb0187p+0, -0x1.41577ee04992fp-55}, {0x1.7e2f336cf4e62p+0, 0x1.05d02ba15797ep-56},
    {0x1.82589994cce13p+0, -0x1.d4c1dd41532d8p-54}, {0x1.868d99b4492edp+0, -0x1.fc6f89bd4f6bap-54},
    {0x1.8ace5422aa0dbp+0, 0x1.6e9f156864b27p-54}, {0x1.8f1ae99157736p+0, 0x1.5cc13a2e3976cp-55},
    {0x1.93737b0cdc5e5p+0, -0x1.75fc781b57ebcp-57}, {0x1.97d829fde4e50p+0, -0x1.d185b7c1b85d1p-54},
    {0x1.9c49182a3f090p+0, 0x1.c7c46b071f2bep-56}, {0x1.a0c667b5de565p+0, -0x1.359495d1cd533p-54},
    {0x1.a5503b23e255dp+0, -0x1.d2f6edb8d41e1p-54}, {0x1.a9e6b5579fdbfp+0, 0x1.0fac90ef7fd31p-54},
    {0x1.ae89f995ad3adp+0, 0x1.7a1cd345dcc81p-54}, {0x1.b33a2b84f15fbp+0, -0x1.2805e3084d708p-57},
    {0x1.b7f76f2fb5e47p+0, -0x1.5584f7e54ac3bp-56}, {0x1.bcc1e904bc1d2p+0, 0x1.23dd07a2d9e84p-55},
    {0x1.c199bdd85529cp+0, 0x1.11065895048ddp-55}, {0x1.c67f12e57d14bp+0, 0x1.2884dff483cadp-54},
    {0x1.cb720dcef9069p+0, 0x1.503cbd1e949dbp-56}, {0x1.d072d4a07897cp+0, -0x1.cbc3743797a9cp-54},
    {0x1.d5818dcfba487p+0, 0x1.2ed02d75b3707p-55}, {0x1.da9e603db3285p+0, 0x1.c2300696db532p-54},
    {0x1.dfc97337b9b5fp+0, -0x1.1a5cd4f184b5cp-54}, {0x1.e502ee78b3ff6p+0, 0x1.39e8980a9cc8fp-55},
    {0x1.ea4afa2a490dap+0, -0x1.e9c23179c2893p-54}, {0x1.efa1bee615a27p+0, 0x1.dc7f486a4b6b0p-54},
    {0x1.f50765b6e4540p+0, 0x1.9d3e12dd8a18bp-54}, {0x1.fa7c1819e90d8p+0, 0x1.74853f3a5931ep-55},
};
__device__ __forceinline__ void exp_tab_stage(double2* tab) {
  if (threadIdx.x < 64) tab[threadIdx.x] = make_double2(g_exp_tab[threadIdx.x][0], g_exp_tab[threadIdx.x][1]);
}
__device__ __forceinline__ double exp_neg(double x, const double2* tab) {
  x = x < -746.0 ? -746.0 : x;
  const double j = rint(x * 0x1.71547652b82fep+6);  // 64 / ln2
  const int n = (int)j;
  const double r = fma(-j, 0x1.1cf79abc9e3b4p-42, fma(-j, 0x1.62e42fef80000p-7, x));
  const double pr = r * fma(r, fma(r, fma(r, fma(r, 1.0 / 120.0, 1.0 / 24.0), 1.0 / 6.0), 0.5), 1.0);
  const double2 t = tab[n & 63];
  return ldexp(t.x + fma(t.x, pr, t.y), n >> 6);
}

// Gaussian CRPS and negative log density of one point (crps KF:60-68, logs KF:52-57; c is
// the VARIANCE)
__device__ __forceinline__ double crps_term(double m, double c, double y) {
  const double s = sqrt(c);
  const double z = (y - m) / s;
  const double cdf = 0.5 * (1.0 + erf(z * 0.70710678118654752440));
  const double pdf = 0.39894228040143267794 * exp(-z * z * 0.5);
  return s * (z * (2.0 * cdf - 1.0) + 2.0 * pdf - 0.56418958354775628695);
}
__device__ __forceinline__ double logs_term(double m, double c, double y) {
  const double e = y - m;
  return e * e / (2.0 * c) + log(sqrt(c)) + 0.91893853320467274178;
}
#endif

// gradient contraction: Σ_ij M_ij ∂A_ij/∂θ over the real n×n lower triangle with
// M_ij = a0·Ainv_ij + a1·α_iα_j + a2·½(v_iα_j + α_iv_j) + a3·Mx_ij (kernels_grad.hip)
struct GradParams {
  const double* x;          // [n][d] raw features
  int n, d;
  double sf2;
  double inv_ell[GPS_MAX_D];
  const double* Ainv; const double* Mx; int64_t ldm;
  const double* alpha; const double* v;
  double a0, a1, a2, a3;
  double* slab;             // grad_contract_slab_doubles(n, d)
};

// FITC gradient contraction (kernels_fitc_grad.hip): rows xr (nr), columns xc (nc),
// G_ij = Σ_t coef_t·(rs_t ? rs_t[i] : 1)·R_t[i][j] + Σ_q pc_q·pv_q[i]·qv_q[j]
struct FitcContractParams {
  const double* xr; const double* xc;   // [nr][d], [nc][d] raw features
  int nr, nc, nc_pad, d;
  double sf2;
  double inv_ell[GPS_MAX_D];
  int nt;                               // matrix terms (<= 4)
  const double* R[4]; int64_t ldr[4]; double coef[4]; const double* rs[4];
  double pc[2]; const double* pv[2]; const double* qv[2];  // rank-1 terms (pc = 0: off)
  double* slab;                         // fitc_contract_slab_doubles(nr, nc_pad, d)
  double* zslab;                        // set by the launcher
  int rchunk;                           // set by the launcher
};

// objective surfaces over a (length-scale, noise s.d.) grid (kernels_surface.hip, CP.R)
#define GPS_SURFACE_MAX_N 128
struct SurfaceParams {
  const double* x; const double* y;  // [n][d], [n]
  int n, d;
  double sf2;
  const double* ell; int nl;         // length-scales ℓ (not logs), grid columns
  const double* sd; int ns;          // noise standard deviations s (σ² = s²), grid rows
  int logs_add_noise;                // CP.R:81: LOO-LogS variance 1/d + s²
  double* out;                       // [4][ns][nl]: LOO-CRPS, in-sample CRPS, NLML, LOO-LogS
};

// batches of small full GPs, one workgroup per problem (kernels_batch.hip): value + gradient, or
// `nsteps` SGD steps and, with do_final, the final forward with the test predictive and scores.
// n <= GPS_SURFACE_MAX_N (the whole matrix in one CU's LDS, as the surface kernel), d <= GPS_BATCH_MAX_D
#define GPS_BATCH_MAX_D 16
constexpr int kBatchStepsPerLaunch = 64;  // SGD steps one launch may run
enum { BATCH_MODE_GRAD = 0, BATCH_MODE_TRAIN = 1 };
struct BatchParams {
  // the validation rows the tall full-GP VA kernels score inside the fit; every other
  // launcher ignores them.  They stand in FRONT: a tall kernel's arguments are this struct and its
  // workspace behind it, and the compiler fetches `sc` and the workspace pointer in one load; new
  // members between the two changed the register allocation of the kernels that never read them
  // (5 and 11 more SGPR spills), in front every kernel argument moves by 32 bytes and nothing else
  const double* xv; const double* yv; int nv;   // [nprob][nv][d], [nprob][nv]
  int va_every;                       // step i is a checkpoint when i % va_every == 0
  double* va_sc;                      // [nprob][ceil(itr / va_every) + 1][GPS_N_SC]
  const double* x; const double* y;   // [nprob][n][d], [nprob][n]
  int nprob, n, d, n_ell, kind, objective, mode;
  // per-problem state, kept on the device between the launches of one call
  double* theta;      // [nprob][2 + n_ell], read and (training) updated in place
  double* stale;      // [nprob] log σ² of the last forward a step ran (θ0's before the first)
  int* info;          // [nprob] 0, or the 1-based order of the leading minor that failed
  int* steps_done;    // [nprob]
  int step0, nsteps, itr;   // this launch runs steps [step0, step0 + nsteps) of itr
  double lr;
  int do_final, stale_noise;
  const double* xt; const double* yt; int nt;   // [nprob][nt][d], [nprob][nt]; NULL: none
  double* values; double* thetas;     // [nprob][itr], [nprob][itr][2 + n_ell]
  double* obj; double* grad;          // [nprob][GPS_N_OBJ], [nprob][2 + n_ell] (BATCH_MODE_GRAD)
  double* mu; double* var; double* sc;  // [nprob][nt] twice, [nprob][GPS_N_SC]
};
size_t batch_lds_bytes(int n, int d);

// batches of small FITC GPs, one workgroup per problem (kernels_batch_fitc.hip): as
// BatchParams, with m <= GPS_BATCH_FITC_MAX_M inducing inputs per problem that the SGD steps move
// too (z -= lr_z·∂/∂z).  ARD kernel only, jitter 1e-3 inside K̃mm (K20:32-39).
#define GPS_BATCH_FITC_MAX_M 32
struct BatchFitcParams {
  const double* x; const double* y;   // [nprob][n][d], [nprob][n]
  int nprob, n, d, m, n_ell, objective, mode;
  // per-problem state, kept on the device between the launches of one call
  double* theta;      // [nprob][2 + n_ell], read and (training) updated in place
  double* z;          // [nprob][m][d], read and (training) updated in place
  double* stale;      // [nprob] log σ² of the last forward a step ran (θ0's before the first)
  int* info;          // [nprob] 0, k (K̃mm's leading minor k failed) or m + k (B's)
  int* steps_done;    // [nprob]
  int step0, nsteps, itr;   // this launch runs steps [step0, step0 + nsteps) of itr
  double lr, lr_z;
  int do_final, stale_noise;
  const double* xt; const double* yt; int nt;   // [nprob][nt][d], [nprob][nt]; NULL: none
  double* values; double* thetas;     // [nprob][itr], [nprob][itr][2 + n_ell]
  double* obj; double* grad; double* grad_z;  // [nprob][GPS_N_OBJ]; BATCH_MODE_GRAD: [nprob][2 + n_ell], [nprob][m][d]
  double* mu; double* var; double* sc;  // [nprob][nt] twice, [nprob][GPS_N_SC]
};
size_t batch_fitc_lds_bytes(int n, int m, int d);

// batches of tall FITC GPs, one workgroup per problem (kernels_batch_fitc_tall.hip):
// BatchFitcParams' model and semantics with the n-sized arrays in a per-problem device workspace
// instead of LDS, so n is bounded by time, not by the CU's 160 KB.  Why 2048: one evaluation is
// about 10·n·m² FMAs on the one CU a problem owns (≈ 21 MFMA at m = 32, of the order of 0.3 ms at
// a realistic fraction of a CU's FP64 rate), which is where the launch- and PCIe-bound resident
// step (≈ 0.5 ms at any n this small) stops losing to it for a single problem; beyond
// it the resident path's 256 CUs win even for small batches.  That is a flop estimate, not a
// measurement: tools/fitc_tall_bench.py records the per-step time at n = 128..2048, and measured
//  the kernel is latency-bound, 1.8 ms a step at n = 2048, m = 20, so one problem
// alone breaks even near n = 650 and the limit is kept for batches: three problems of n = 2048
// already beat the sequential loop, and 256 cost what one costs.
#define GPS_BATCH_FITC_TALL_MAX_N 2048
constexpr int kBatchFitcTallChunk = 128;  // rows of a pass's LDS chunk: two chunk×(m|1) arrays and
                                          // the six m×m arrays must fit 160 KB at m = 32 (192 rows
                                          // would not), and a multiple of every column group's 64
                                          // lanes keeps the row order independent of the chunking
struct BatchFitcTallParams {
  BatchFitcParams b;
  double* ws;           // [nprob][ws_stride] V, U (n×(m|1) each), then nine n-vectors
  int64_t ws_stride;    // >= batch_fitc_tall_ws_doubles(n, m)
};
size_t batch_fitc_tall_lds_bytes(int n, int m, int d);
int64_t batch_fitc_tall_ws_doubles(int64_t n, int m);
// SGD steps one launch may run: a step's cost grows with the chunk count, so kBatchStepsPerLaunch
// is divided by it (64 up to n = 128, 16 at n = 500, 4 at n = 2048): a function of n alone
int batch_fitc_tall_steps(int64_t n);
hipError_t launch_batch_fitc_tall(const BatchFitcTallParams& p, hipStream_t s);

// the same batches on the block-LOO objectives GPS_BLOCK_DSS / GPS_BLOCK_KC over nfold folds
// (kernels_batch_fitc_tall_block.hip): b.objective is the GPS_BLOCK_* code, everything
// else in b means what it means above.  info is 0, k in 1..m (K̃mm), m + k (B) or (2 + f)·m + k
// (the leading minor of order k of fold f's B₋f = K̃mm + Σ_{g≠f} K_gᵀΛ_g⁻¹K_g is not > 0: an
// internal error, B₋f is K̃mm plus positive semidefinite terms).  GPS_BATCH_BLOCK_MAX_FOLDS is
// defined below, with the full-GP block path.
struct BatchFitcTallBlockParams {
  BatchFitcParams b;
  double* ws;           // [nprob][ws_stride] K, V, Ũ, F (n×(m|1) each), the nfold + 1 m×(m|1)
                        // blocks part_f and K̃mm, then eleven n-vectors
  int64_t ws_stride;    // >= batch_fitc_tall_block_ws_doubles(n, m, nfold)
  int nfold;            // 2..GPS_BATCH_BLOCK_MAX_FOLDS, <= n
  double* value;        // [nprob] BATCH_MODE_GRAD: the block objective
  double* fold_values;  // [nprob][nfold] BATCH_MODE_GRAD: each fold's term, or NULL
};
size_t batch_fitc_tall_block_lds_bytes(int n, int m, int d);
int64_t batch_fitc_tall_block_ws_doubles(int64_t n, int m, int nfold);
// SGD steps one launch may run: batch_fitc_tall_steps' rule divided by kBatchFitcTallBlockDiv,
// max(1, 32 / ceil(n / 128)) (32 up to n = 128, 8 at n = 500, 2 at n = 2048): a block step is about
// two tall steps' work, and undivided the corner's longest launch measured 31 ms: a
// function of n alone
constexpr int kBatchFitcTallBlockDiv = 2;
int batch_fitc_tall_block_steps(int64_t n);
hipError_t launch_batch_fitc_tall_block(const BatchFitcTallBlockParams& p, hipStream_t s);

// the two tall FITC paths with a validation set scored inside the fit (batch_fitc_tall_va_kernel,
// batch_fitc_tall_block_va_kernel).  The validation members live in structs of the new
// kernels' own that hold the old struct FIRST, so no argument of an old kernel moves (§34 found
// that new members inside a shared struct changed the register allocation of kernels that never
// read them).  Step i = step0 + st of a launch is a checkpoint when i % va_every == 0: directly
// after its forward() the kernel scores the nv validation rows at that forward's θ, Z and σ² into
// row i / va_every of va_sc and copies the current Z into va_z; the final pass adds row nva − 1,
// nva = ceil(itr / va_every) + 1.  A failed problem keeps the rows it reached and gets NaN in the
// rest.  LDS and workspace are the plain kernels'.
struct BatchVaParams {
  const double* xv; const double* yv;   // [nprob][nv][d], [nprob][nv]
  int nv, va_every;
  double* va_sc;                        // [nprob][nva][GPS_N_SC]
  double* va_z;                         // [nprob][nva][m][d], or NULL: no Z is kept
};
struct BatchFitcTallVaParams {
  BatchFitcTallParams t;
  BatchVaParams va;
};
struct BatchFitcTallBlockVaParams {
  BatchFitcTallBlockParams t;
  BatchVaParams va;
};
// SGD steps one VA launch may run: never more than the plain rule's, and at most
// kBatchFitcVaRowBudget validation rows streamed by its checkpoints, so that they add at most ~5 ms
// to a launch (a row measured 1.07 µs at m = 32, d = 16: 4.4 ms for the budget); always
// at least one step.  A window of k steps holds at most ceil(k / va_every) checkpoints, so k = max(1,
// floor(budget / nv)·va_every): a function of n, nv and va_every alone.
constexpr int64_t kBatchFitcVaRowBudget = 4096;
int batch_fitc_tall_va_steps(int64_t n, int64_t nv, int64_t va_every);
int batch_fitc_tall_block_va_steps(int64_t n, int64_t nv, int64_t va_every);
// BATCH_MODE_TRAIN only: refuse BATCH_MODE_GRAD, a NULL xv, yv or va_sc, nv < 1 and va_every < 1
hipError_t launch_batch_fitc_tall_va(const BatchFitcTallVaParams& p, hipStream_t s);
hipError_t launch_batch_fitc_tall_block_va(const BatchFitcTallBlockVaParams& p, hipStream_t s);

// batches of full GPs of up to 512 rows, one workgroup per problem (kernels_batch_full_tall.hip,
// DESIGN §24): BatchParams' model and semantics with the n×n arrays in a per-problem device
// workspace instead of LDS and the O(n³) work on the FP64 matrix instruction, tile by tile.  Why
// 512: a LOO step is about 630 tile products (1.7·10⁸ FMAs) at n = 512, an arithmetic floor of
// about 1.1 ms on the one CU a problem owns; it grows with n³, and beyond this the resident path's
// 256 CUs are the better home for all but very large batches.
#define GPS_BATCH_FULL_TALL_MAX_N 512
constexpr int kBatchFullTallTile = 64;  // tile edge T: n is padded to a multiple inside the workspace
struct BatchFullTallParams {
  BatchParams b;
  double* ws;           // [nprob][ws_stride]: A / L / P, then X = L⁻¹ (np×np each); 32-byte aligned
  int64_t ws_stride;    // >= batch_full_tall_ws_doubles(n), a multiple of 4
};
size_t batch_full_tall_lds_bytes(int n);
int64_t batch_full_tall_ws_doubles(int64_t n);
// SGD steps one launch may run: a step's cost grows with the cube of the block count nb =
// ceil(n / 64), so it is min(64, max(1, 1024 / nb³)) (64 up to n = 128, 16 at n = 256, 2 at n =
// 500): a function of n alone
int batch_full_tall_steps(int64_t n);
hipError_t launch_batch_full_tall(const BatchFullTallParams& p, hipStream_t s);
// the same launch with b.xv / b.yv scored at the checkpoints and in the final pass (b.va_sc;
// BATCH_MODE_TRAIN only): refuses a NULL xv, yv or va_sc, nv < 1 and va_every < 1
hipError_t launch_batch_full_tall_va(const BatchFullTallParams& p, hipStream_t s);

// the same batches on the block-LOO objectives GPS_BLOCK_DSS / GPS_BLOCK_KC over nfold folds
// (kernels_batch_full_tall_block.hip): b.objective is the GPS_BLOCK_* code, everything
// else in b means what it means above.  info is 0, k in 1..n (A's leading minor k failed) or n + k
// (the pivot of global row k of its fold's P_f = (A⁻¹)_ff is not > 0: an internal error, a positive
// definite A has positive definite P_f).
#define GPS_BATCH_BLOCK_MAX_FOLDS 32
struct BatchFullTallBlockParams {
  BatchParams b;
  double* ws;           // [nprob][ws_stride]: W0 (np²) | W1 (max(np², 2·bp²)) | W2 (np²), np and bp
                        // the padded n and largest fold; 32-byte aligned
  int64_t ws_stride;    // >= batch_full_tall_block_ws_doubles(n, nfold), a multiple of 4
  int nfold;            // 2..GPS_BATCH_BLOCK_MAX_FOLDS, <= n
  int64_t w1;           // W1's doubles, set by the launcher
  double* value;        // [nprob] BATCH_MODE_GRAD: the block objective
  double* fold_values;  // [nprob][nfold] BATCH_MODE_GRAD: each fold's term, or NULL
};
// LDS is batch_full_tall_lds_bytes(n) and a launch runs batch_full_tall_steps(n) steps: §24's
int64_t batch_full_tall_block_ws_doubles(int64_t n, int nfold);
hipError_t launch_batch_full_tall_block(const BatchFullTallBlockParams& p, hipStream_t s);
// with the validation rows, as launch_batch_full_tall_va
hipError_t launch_batch_full_tall_block_va(const BatchFullTallBlockParams& p, hipStream_t s);

// Scaled Newton–Schulz schedule for a spectrum of C/s inside [x0, 1] (api_block.hip's comment at
// ns_schedule has the derivation): β per step into beta[0..cap), host and device.  At most
// kNsScaledMax scaled or unscaled steps run until the lower bound reaches 1 − 4e-16, two unscaled
// steps follow.  Returns the step count, or −1 when it would exceed cap.
constexpr int kNsScaledMax = 200;
constexpr int kNsMaxSteps = kNsScaledMax + 2;  // the resident path's capacity: never exceeded
__host__ __device__ inline double ns_poly(double x) { return x * (3.0 - x) * (3.0 - x) / 4.0; }
__host__ __device__ inline int ns_schedule_fill(double x0, double* beta, int cap) {
  const double xl = x0 < 1e-300 ? 1e-300 : x0;  // max(x0, 1e-300)
  double l = 1.0 < xl ? 1.0 : xl, u = 1.0;      // min(.., 1)
  int cnt = 0;
  while (1.0 - l > 4e-16 && cnt < kNsScaledMax) {
    if (cnt + 3 > cap) return -1;
    double b = 1.0 / u;
    // scaled while the lower bound is small; from l = 0.5 on the unscaled step converges
    // quadratically (scaling there only chases rounding in the bounds)
    if (l < 0.5 && ns_poly(b * l) < ns_poly(b * u)) {  // bisect f(βl) = f(βu) on [1/u, 2.999/u]
      double lo = 1.0 / u, hi = 2.999 / u;
      for (int it = 0; it < 100; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (ns_poly(mid * l) < ns_poly(mid * u)) lo = mid;
        else hi = mid;
      }
      b = lo;
    }
    const double fl = ns_poly(b * l), fu = ns_poly(b * u);
    const double nl = fu < fl ? fu : fl;
    u = (b * l <= 1.0 && 1.0 <= b * u) ? 1.0 : (fl < fu ? fu : fl);
    l = u < nl ? u : nl;
    beta[cnt++] = b;
  }
  if (cnt + 2 > cap) return -1;
  beta[cnt++] = 1.0;
  beta[cnt++] = 1.0;
  return cnt;
}

// the same batches on the block-LOO energy score (kernels_batch_full_tall_es.hip): a
// step is a launch sequence — (A) forward and P per problem, (E) the fold work on one workgroup per
// (problem, fold), at most 256 of them a launch, (C) the tail and the θ update per problem — and
// the final pass is
// launch_batch_full_tall's with no steps.  info is 0, k in 1..n (A's leading minor), n + k (a
// fold's P_f pivot, as §26) or 2n + 1 + f (fold f's Newton–Schulz schedule needs more than
// kBatchEsNsCap steps: σ² is below ~1e-24 of ‖Π_f‖∞).
constexpr int kBatchEsNsCap = 40;        // Newton–Schulz steps a fold may run
#define GPS_BATCH_ES_MAX_FOLD 128        // rows of the largest fold: two tiles on a side
#define GPS_BATCH_ES_MAX_SIM 512
struct BatchFullTallEsParams {
  BatchParams b;        // b.objective is unused; b.nsteps is 0 or 1
  double* ws;           // [nprob][ws_stride], 32-byte aligned
  int64_t ws_stride;    // >= batch_full_tall_es_ws_doubles(n, nfold, num_sim), a multiple of 4
  int nfold, num_sim;
  double beta;
  const double* draws;  // device, [nprob][draw_sets][2·num_sim·n]; step i reads set i mod draw_sets
  int64_t draw_sets;
  double* value;        // [nprob] BATCH_MODE_GRAD
  double* fold_values;  // [nprob][nfold] BATCH_MODE_GRAD, or NULL
};
// 3·np² + 2·np + 72 + nfold·(11·bp² + 6·Sp·bp + Sp²) doubles a problem: np, bp the padded n and
// largest fold, Sp = 64·⌈(num_sim + 1)/64⌉ (the forward iterates are recomputed, not stored)
int64_t batch_full_tall_es_ws_doubles(int64_t n, int nfold, int num_sim);
// one launch of the sequence: ES_FORWARD, ES_FOLDS, ES_TAIL (a step, or the one evaluation of
// BATCH_MODE_GRAD; nothing with b.nsteps = 0) and ES_FINAL (nothing without b.do_final)
enum { ES_FORWARD = 0, ES_FOLDS = 1, ES_TAIL = 2, ES_FINAL = 3, ES_PHASES = 4 };
hipError_t launch_batch_full_tall_es(const BatchFullTallEsParams& p, int phase, hipStream_t s);

// ------------------------------------------------------------------ launchers
// raises `kernel`'s dynamic-LDS limit to `bytes` on the current device, once per (device, kernel)
// (kernels_surface.hip); every launcher of a kernel that may need more than 64 KB calls it first
hipError_t raise_dynamic_lds(const void* kernel, size_t bytes);
hipError_t launch_surface(const SurfaceParams& p, hipStream_t s);
hipError_t launch_batch(const BatchParams& p, hipStream_t s);
hipError_t launch_batch_fitc(const BatchFitcParams& p, hipStream_t s);
hipError_t launch_gram(const GramParams& p, hipStream_t s);
// C = alpha * op(A) op(B) + beta * C with the epilogue selected by `epi`
// (info, if given, receives the launch's shape; it changes nothing of the launch)
// (resolved, if given, receives the kernel's arguments instead of a launch: gemm_schedule)
hipError_t launch_gemm(int alay, int blay, int epi, const GemmParams& p, hipStream_t s,
                       GemmLaunchInfo* info = nullptr, GemmParams* resolved = nullptr);
constexpr int kGemmItemInts = 8;
int64_t gemm_schedule(int alay, int blay, int epi, const GemmParams& p, GemmLaunchInfo& info,
                      int32_t* items, int64_t cap);

// leaf of the recursive Cholesky: the diagonal 128×128 block, Cholesky + triangular inverse
// in one workgroup (kernels_potrf.hip).  Reads the lower triangle of A (lda), writes L⁻¹
// (lower, zeros above the diagonal) into Linv (ldl), L into Lout (optional), log(L_ii) into
// logdiag[0..127]; sets *info (atomicMin) to the 1-based global index of the first
// non-positive pivot.
hipError_t launch_potrf_leaf(const double* A, int64_t lda, double* Linv, int64_t ldl,
                             double* Lout, int64_t ldlo, double* logdiag, int* info,
                             int base, int n_real_in_block, hipStream_t s);

// persistent tiled factorisation of a diagonal block of T tiles (kernels_potrf.hip): L⁻¹ into
// Linv, L into A's strictly-lower tiles (and Lout if given), logdiag, info[0] as the leaf;
// info[1] != 0x7f7f7f7f on a lost dependency (bounded spin).  cnt: 16 + 2·T² ints, zero at the
// launch and left zero by it (its last workgroup resets them); tasks: dag_task_list(T, ..) on the device.
struct DagParams {
  double* A; int64_t lda;
  double* Linv; int64_t ldl;
  double* Lout; int64_t ldlo;
  double* logdiag; int* info; int base; int nreal;
  int T;
  const uint32_t* tasks; int ntasks;
  int* cnt;
  unsigned long long spin_ticks;   // 100 MHz s_memrealtime ticks a dependency wait may take
  unsigned long long* trace = nullptr;  // diagnostics only (tools/dag_bench.cpp): 4 words per slot
  int group = 3;                   // 16-deep operand chunks per load group of a strip task (2..4)
  int* sig = nullptr;              // row-ready signals for a dependent row-norm launch (kSig*):
                                   // +1 per started workgroup, row tile i flagged once L⁻¹'s row
                                   // tile i is final (LEAF(0); the last FIN(i, ·) strip)
  int kbatch = 1;                  // the longest K batch in the task list (1..8; host-side bound
                                   // check of the batched strips' buffer descriptors only)
};
hipError_t launch_potrf_dag(const DagParams& p, int nwg, hipStream_t s);
// (dag_task_list, g_dag_weights, dag_cnt_ints: dag_task.h, included above)

// y[i] = sum_k L[i][k] x[k] over the tile-lower part (rows < n_pad)
hipError_t launch_gemv_lower(const double* L, int64_t ldl, const double* x, double* y,
                             int n_pad, hipStream_t s);
// y[i] = sum_k M[i][k] x[k], full rows
hipError_t launch_gemv_full(const double* M, int64_t ldm, const double* x, double* y,
                            int rows, int cols, hipStream_t s);
// column reductions over rows i (tile-lower if lower != 0):
//   s1[k] = sum_i M[i][k] w[i]   (if s1 != null)     s2[k] = sum_i M[i][k]^2 (if s2 != null)
// rowscale (optional) multiplies M[i][k] by rowscale[i] before both sums.
// Uses slab (>= nchunks*cols*2 doubles) and reduces into s1/s2.
hipError_t launch_colred(const double* M, int64_t ldm, int rows, int cols, int lower,
                         const double* w, const double* rowscale, double* s1, double* s2,
                         double* slab, hipStream_t s, int crows = 256);
// out[j] = sum_{s < nslab} slab[s*ld + j] (+ init[j] if init), j < len
hipError_t launch_slab_sum(const double* slab, int64_t ld, int nslab, int64_t len,
                           const double* init, double* out, hipStream_t s);
// sum of B slices into dst lower tiles + add (optional) base matrix; zero strict-upper tiles
hipError_t launch_sym_slab_sum(const double* slab, int64_t slice_stride, int nslab, int M,
                               const double* base, double* dst, hipStream_t s);

// symmetric m×m accumulator <-> lower-packed m(m+1)/2 (the FITC all-reduce payload):
// packed = Σ_q slab_q (lower, row-major; rows [r0, r1) only);  dst (M×M) = base +
// unpack(packed), lower 128-tiles (strict-upper tiles zero) or, with full, both triangles
hipError_t launch_sym_pack(const double* slab, int64_t slice_stride, int nslab, int r0, int r1,
                           int M, double* packed, hipStream_t s);
hipError_t launch_sym_unpack(const double* packed, int m, int M, const double* base, int full,
                             double* dst, hipStream_t s);
// full-GP LOO finalize (one workgroup): see kernels_vec.hip
// full-GP LOO: α, d = diag(A⁻¹) summed from the column pass's nslab chunk partials (slab:
// [α chunks | d chunks], ld apart), stored, then μ/σ² LOO and obj = [nlml, loo_crps, loo_logs,
// logdet, quad] (obj + 8: 4 scratch sums; part: ⌈n_pad/256⌉·4 doubles)
hipError_t launch_full_loo(const double* y, const double* slab, int nslab, int64_t ld,
                           const double* beta, const double* logdiag, int n, double* alpha,
                           double* dinv, double* mu_loo, double* var_loo, double* obj,
                           double* part, hipStream_t s);
// CP.R surface point from a resident fit: sums [Σ in-sample CRPS, Σ LOO-LogS (+ s² if add_noise)]
hipError_t launch_surface_point_sums(const double* y, const double* alpha, const double* dinv,
                                     int n, double s2, int add_noise, double* sums, double* part,
                                     hipStream_t s);
int launch_colred_partials(const double* M, int64_t ldm, int rows, int cols, int lower,
                           const double* w, double* slab, hipStream_t s);
// predictive variance finalize + test-score partial sums
hipError_t launch_pred_finalize(const double* s1, const double* s2, int nt, double base_var,
                                double* mu, double* var, hipStream_t s);
hipError_t launch_fitc_pred_finalize(const double* qm, const double* qb, int nt, double base_var,
                                     double* var, hipStream_t s);
// sums: [crps, logs, msll, sq_err, sq_err_trivial, cover]
// (part: scratch of ⌈nt/256⌉·6 doubles for the per-workgroup partials)
hipError_t launch_score_sums(const double* mu, const double* var, const double* y, int nt,
                             double ytr_mean, double ytr_var, double* sums, double* part,
                             hipStream_t s);
// FITC: q_i = Σ_t slab[t·ld + i] (nslab row-norm partials), λ_i = sf2 − q_i + σ² (real rows),
// 1 on pad rows; inv_lam = 1/λ; ys = y/λ; scalars: [Σ log λ, Σ y²/λ]
// (part: scratch of ⌈n_pad/256⌉·2 doubles)
hipError_t launch_fitc_lambda(const double* slab, int64_t ld, int nslab, const double* y, int n,
                              int n_pad, double sf2, double sn2, double* q, double* lam,
                              double* inv_lam, double* ys, double* scal, double* part,
                              hipStream_t s);
// FITC LOO: r_i = Σ_t slab[t·ld + i], d = 1/λ − r/λ², α = (y − g)/λ → μ, σ²; sums [Σ crps, Σ logs]
hipError_t launch_fitc_loo(const double* y, const double* lam, const double* slab, int64_t ld,
                           int nslab, const double* g, int n, int n_pad, double* r,
                           double* mu_loo, double* var_loo, double* sums, double* part,
                           hipStream_t s);
// small dense triangular mat-vec on the device: y = op(L) x with L lower (n_pad)
hipError_t launch_trmv_lower(const double* L, int64_t ldl, const double* x, double* y,
                             int n_pad, int trans, hipStream_t s);
hipError_t launch_dot(const double* a, const double* b, int n, double* out, hipStream_t s);
// dst (rows_pad × cols_pad) = src zero-padded; pad_identity puts 1 on the padded
// diagonal (embedding an SPD matrix as diag(A, I))
hipError_t launch_pad_copy(const double* src, int64_t lds, double* dst, int64_t ldd, int rows,
                           int cols, int rows_pad, int cols_pad, int pad_identity, hipStream_t s);

// --- gradients (kernels_grad.hip)
// u = −g_μ/d, ct = (g_μα − g_c)/d² of the mean LOO score `obj` (GPS_OBJ_LOO_CRPS / _LOGS)
hipError_t launch_loo_grad_terms(const double* y, const double* alpha, const double* dinv, int n,
                                 int n_pad, int obj, double* u, double* ct, hipStream_t s);
// strictly-upper 32-tiles := transpose of the strictly-lower ones
hipError_t launch_sym_mirror(double* M, int64_t ld, int n_pad, hipStream_t s);
// *out = max_i Σ_j |A_ij| over the n×n block (the ∞-norm; rowsum: n doubles of scratch)
hipError_t launch_norm_inf(const double* A, int64_t lda, int n, double* rowsum, double* out,
                           hipStream_t s);
int grad_contract_passes(int d);
int64_t grad_contract_slab_doubles(int n, int d);
// out[pass*18 + q]: q = 0 Σ w m K, 1 Σ_diag m, 2+k Σ w m K Δ²_(16·pass+k)
hipError_t launch_grad_contract(const GradParams& p, double* out, hipStream_t s);

// --- block-LOO (kernels_block.hip)
hipError_t launch_fold_terms(const double* y, const double* r, const double* c, int b, double* gm,
                             double* gc, double* out, hipStream_t s);
hipError_t launch_fold_grad(const double* PI, int64_t ldp, const double* H, int64_t ldh,
                            const double* r, const double* w, int b, double c0, double c1,
                            double c2, double c3, double gr, double gw, double* G, int64_t ldg,
                            double* g, hipStream_t s);
hipError_t launch_row_scale(double* M, int64_t ld, int rows, int cols, const double* scale,
                            hipStream_t s);
hipError_t launch_vec_mul(const double* a, const double* b, int n, double* out, hipStream_t s);
// dst = base (+ base2) + sgn·Σ_{g ≠ skip} slab_g (len doubles, slabs `stride` apart, fixed order)
hipError_t launch_fold_sum(const double* slab, int64_t stride, int nslab, int skip, const double* base,
                           const double* base2, double sgn, double* dst, int64_t len, hipStream_t s);
// *out = Σ ldf[<m] − Σ ldb[<m] − ½Σ log lam[<b]: −½log|C_f| of a FITC block-LOO fold covariance
// the in-process communicator's device sum (kernels_vec.hip): up to kLocalSumMax ranks' staging
// buffers summed in rank order
constexpr int kLocalSumMax = 64;
struct LocalSumPtrs {
  const double* p[kLocalSumMax];
};
hipError_t launch_local_sum(const LocalSumPtrs& sp, int n, int64_t count, double* out, hipStream_t s);
// FITC block-LOO in low rank (kernels_block.hip): per-row dots of a b×m W, the fold vectors, and
// the F̃ rows as a base product plus rank-one terms
hipError_t launch_row_dots(const double* A, int64_t lda, const double* B, int64_t ldb,
                           const double* t, int rows, int cols, double* at, double* ab,
                           hipStream_t s);
hipError_t launch_lr_fold_vec(int mode, int b, int bp, const double* lam, const double* x,
                              const double* at, const double* ab, const double* r, const double* c,
                              const double* w, const double* gc, const double* q, double* o1,
                              double* o2, hipStream_t s);
hipError_t launch_lr_combine(const double* X, int64_t ldx, const double* Y, int64_t ldy,
                             const double* lam, const double* rs, double c0, const double* u1,
                             const double* v1, double c1, const double* u2, const double* v2,
                             double c2, int rows, int rows_pad, int cols, double* out, int64_t ldo,
                             hipStream_t s);
hipError_t launch_fold_logdet(const double* ldf, const double* ldb, int m, const double* lam, int b,
                              double* out, hipStream_t s);
// FITC block-LOO gradient (whitened): M_ii, the V Lm⁻¹ row scale and Y = −2Λ⁻¹F̃ + 2ŨS̃
// (see kernels_block.hip; Y may alias US)
hipError_t launch_blk_mdiag(const double* F, int64_t ldf, const double* US, int64_t ldus,
                            const double* U, int64_t ldu, int m_pad, const double* gd,
                            const double* lam, const double* v, const double* alpha, int n,
                            int n_pad, double* md, double* sc, double* Y, int64_t ldy,
                            hipStream_t s);
// energy score: Newton–Schulz steps, distances, reduction
hipError_t launch_ns_init(const double* C, int64_t ldc, int b, int bp, double scale, double pad,
                          double* Y, hipStream_t s);
hipError_t launch_diag_add_const(double* M, int64_t ld, int n, double c, hipStream_t s);
hipError_t launch_sym_avg(double* M, int64_t ld, int n, hipStream_t s);
hipError_t launch_scaled_row(const double* src, int b, int bp, double scale, double* dst,
                             hipStream_t s);
hipError_t launch_row_axpy(double* C, int64_t ldc, const double* Z, int64_t ldz, const double* sv,
                           int rows, int cols, hipStream_t s);
hipError_t launch_ns_resid(const double* T, int64_t ld, int n, double* out, hipStream_t s);
hipError_t launch_es_dist(const double* Z, const double* Zh, int64_t ld, int S, int bp, double* D,
                          int64_t ldd, hipStream_t s);
hipError_t launch_es_reduce(double* D, int64_t ldd, int S, int Sp, double beta, int grad,
                            double* rs, double* cs, double* out, hipStream_t s);

// --- joint test predictive (kernels_joint.hip)
// The covariance finisher: Sigma (bp×bp, ld bp, both triangles, diag(Sigma_b, I) on the padding) =
// sf2·exp(−½‖(x_i − x_j)/ℓ‖²) + sn2·δ_ij − Σ_q slab_q[i][j] over the block's b rows x ([b][d]);
// slab: ks slices of bp×bp, `stride` apart, lower 128-tiles valid, summed in slice order
struct JointCovParams {
  const double* x;
  int b, bp, d;
  double sf2, sn2;
  double inv_ell[GPS_MAX_D];
  const double* slab; int64_t stride; int ks;
  double* out;
};
hipError_t launch_joint_cov(const JointCovParams& p, hipStream_t s);
// r[i] = y[i] − mu[i] (i < b), 0 on the padding (i < bp)
hipError_t launch_joint_resid(const double* y, const double* mu, int b, int bp, double* r,
                              hipStream_t s);
// *out = ½b·log2π + Σ_{i<b} logdiag[i] + ½Σ_{i<b} t[i]² (dss KF:103-108 with logdiag = log L_ii,
// t = L⁻¹r)
hipError_t launch_joint_dss(const double* logdiag, const double* t, int b, double* out,
                            hipStream_t s);
// dst[i] = +1 (i < npos), −1 (npos <= i < n): the per-k scale of the stacked FITC product
hipError_t launch_sign_fill(double* dst, int npos, int n, hipStream_t s);
// M[i][j] += mu[j] (i < rows, j < cols)
hipError_t launch_row_add(double* M, int64_t ld, const double* mu, int rows, int cols,
                          hipStream_t s);

// --- FITC gradients (kernels_fitc_grad.hip)
hipError_t launch_fitc_grad_terms(const double* y, const double* lam, const double* r,
                                  const double* g, int n, int n_pad, int obj, double n_total,
                                  double* alpha, double* dinv, double* v, double* ulam, double* h,
                                  double* hl2, hipStream_t s);
hipError_t launch_fitc_grad_v(const double* ulam, const double* z, const double* lam, int n,
                              double* v, hipStream_t s);
hipError_t launch_fitc_grad_mdiag(const double* KN, int64_t ldkn, const double* K, int64_t ldk,
                                  int m_pad, const double* lam, const double* r, const double* dinv,
                                  const double* alpha, const double* v, const double* h, double a,
                                  int n, int n_pad, double* mdiag, double* s1, double* s2,
                                  double* s3, hipStream_t s);
hipError_t launch_fitc_grad_y(const double* U, const double* UP, int64_t ld, const double* s1,
                              const double* s2, int rows, int cols, double* Y, hipStream_t s);
int fitc_contract_passes(int d);
int64_t fitc_contract_slab_doubles(int nr, int nc_pad, int d);
// out[pass*17 + q]: q = 0 Σ GK, 1+k Σ GK Δ²_(16·pass+k);  zout[j*d + k] = Σ_i GK Δ_k (real j)
hipError_t launch_fitc_grad_contract(FitcContractParams p, double* out, double* zout,
                                     hipStream_t s);

}  // namespace gps
