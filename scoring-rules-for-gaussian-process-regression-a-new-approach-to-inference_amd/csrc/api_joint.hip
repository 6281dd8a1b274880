// C-ABI, the joint test predictive: the full covariance of a block of the resident test rows
// (cal_mean_and_cov KF:121-126, spgp_cal_mean_and_cov K20:76-83 — gps_*_predict keeps only its
// diagonal), the multivariate scores of held-out data on it (dss KF:103-108 as called at
// KF:556-563, ES KF:70-101 as called at KF:677-684) and joint posterior draws (as SD:174 draws
// its data).  Everything on ctx->stream, in buffers of these calls' own (ctx->j*): the fit, the
// buffers of gps_*_predict and the FITC test pre-pass are only read.
//
//   full GP  Sigma = sigma²I + K** − VᵀV,            V = L⁻¹K_bᵀ            (n_pad × b_pad)
//   FITC     Sigma = sigma²I + K** − V₁ᵀV₁ + V₂ᵀV₂,  V = [Lm⁻¹K_bmᵀ; Lb⁻¹K_bmᵀ] (2·m_pad × b_pad)
// K_b is the block's OWN cross Gram (b_pad rows, zero padding): the resident Ksf / Ksm hold other
// test points past the block's last row.  S = VᵀV (FITC: Vᵀdiag(+1.., −1..)V, one launch) is a
// split-K SYRK-shaped launch of the FP64 MFMA GEMM into slabs; the finisher (kernels_joint.hip)
// sums them, subtracts from K** + sigma²I evaluated on the fly, mirrors and pads in one pass.
#include "api_internal.h"

namespace gpsapi {

enum { JOINT_FULL = 0, JOINT_FITC = 1 };
constexpr int64_t kJointMaxRows = 16384;
constexpr double kJointMaxVBytes = 8.0 * 1024 * 1024 * 1024;

// the vectors of a block in ctx->jvec (bp doubles each), then the per-block scalars
struct JointVec {
  double *mu, *r, *t, *ld, *w, *rowsum, *vals, *norms;
};
static JointVec joint_vec(gps_ctx* ctx, int64_t bp) {
  double* v = ctx->jvec.d();
  return {v, v + bp, v + 2 * bp, v + 3 * bp, v + 4 * bp, v + 5 * bp, v + 6 * bp, v + 6 * bp + 64};
}

// refusals shared by the six entry points (after bind)
static int joint_ready(gps_ctx* ctx, int model) {
  ARGCHK(!sharded(ctx), "the joint test predictive is not available on a context with a "
                        "communicator (sharded joint scores are not implemented)");
  if (model == JOINT_FULL) {
    ARGCHK(ctx->fitted, "gps_full_fit first");
    ARGCHK(ctx->have_test, "gps_full_set_test first");
  } else {
    ARGCHK(ctx->f_fitted, "gps_fitc_fit first");
    ARGCHK(ctx->f_test, "gps_fitc_set_test first");
  }
  return 0;
}

static int joint_rows_ok(gps_ctx* ctx, int model, int64_t r0, int64_t r1) {
  const int64_t nt = model == JOINT_FULL ? ctx->nt : ctx->fnt;
  ARGCHK(r0 >= 0 && r0 < r1 && r1 <= nt, "rows must satisfy 0 <= r0 < r1 <= nt");
  ARGCHK(r1 - r0 <= kJointMaxRows, "a block may hold at most 16384 rows: use smaller blocks");
  return 0;
}

// K slices of the S = VᵀV launch: about two workgroups per CU over the lower 128-tiles, slices at
// least 256 deep, at least 2 (the finisher is the reduction) and at most 32
static int joint_ksplit(const gps_ctx* ctx, int64_t bp, int64_t kv) {
  const int64_t T = bp / GPS_TILE, tiles = T * (T + 1) / 2;
  int64_t ks = (2 * (int64_t)std::max(ctx->ncu, 1) + tiles - 1) / tiles;
  ks = std::min<int64_t>(ks, kv / 256);
  return (int)std::max<int64_t>(2, std::min<int64_t>(ks, 32));
}

// mu_b (jvec) and the padded Sigma_b (jS: bp×bp, both triangles, diag(Sigma_b, I)) of test rows
// [r0, r1) on the device; bp >= pad_to(r1 − r0), a multiple of 128
static int joint_cov_block(gps_ctx* ctx, int model, int64_t r0, int64_t r1, int64_t bp) {
  hipStream_t s = ctx->stream;
  const bool fitc = model == JOINT_FITC;
  const int64_t b = r1 - r0;
  const Theta& th = fitc ? ctx->fth : ctx->th;
  const int d = fitc ? ctx->fd : ctx->d;
  const double* xt = (fitc ? ctx->fXt.d() : ctx->Xt.d()) + r0 * d;
  const int64_t kin = fitc ? ctx->m_pad : ctx->n_pad;  // columns of the cross Gram
  const int64_t kv = fitc ? 2 * kin : kin;             // rows of V
  ARGCHK((double)kv * (double)bp * 8.0 <= kJointMaxVBytes,
         "the block's V buffer would exceed 8 GiB: use smaller blocks");
  HIPCHK(ensure(ctx, ctx->jK, (size_t)bp * kin * 8));
  HIPCHK(ensure(ctx, ctx->jV, (size_t)kv * bp * 8));
  HIPCHK(ensure(ctx, ctx->jS, (size_t)bp * bp * 8));
  HIPCHK(ensure(ctx, ctx->jvec, (size_t)(6 * kJointMaxRows + 256 + 2 * kin) * 8));
  const JointVec jv = joint_vec(ctx, bp);
  int rc;
  // 1. the block's own cross Gram (zero pad rows and columns) and the mean
  if ((rc = gram(ctx, "gram_joint", xt, (int)b, fitc ? ctx->Z.d() : ctx->X.d(),
                 (int)(fitc ? ctx->m : ctx->n), d, th, 0.0, 0, 0, ctx->jK.d(), kin, (int)bp,
                 (int)kin)))
    return rc;
  HIPCHK(launch_gemv_full(ctx->jK.d(), kin, fitc ? ctx->c.d() : ctx->alpha.d(), jv.mu, (int)bp,
                          (int)kin, s));
  // 2. V = L⁻¹K_bᵀ (the TRMM pred_rows launches, stored); FITC: Lm⁻¹ above Lb⁻¹
  const double* Ls[2] = {fitc ? ctx->Lm.d() : ctx->Linv.d(), ctx->Lb.d()};
  for (int w = 0; w < (fitc ? 2 : 1); ++w) {
    GemmParams p = gp0();
    p.A = Ls[w]; p.lda = kin; p.B = ctx->jK.d(); p.ldb = kin;
    p.C = ctx->jV.d() + (int64_t)w * kin * bp; p.ldc = bp;
    p.M = (int)kin; p.N = (int)bp; p.K = (int)kin; p.tri = TRI_K_LE_I;
    if ((rc = gemm(ctx, LAY_N, LAY_T, EPI_STORE, p))) return rc;
  }
  // 3. S = VᵀV in K slices (lower 128-tiles of each slab): the stream's workspace, or the calls'
  //    own slabs (2 slices) when the block is too large for it
  int ks = joint_ksplit(ctx, bp, kv);
  HIPCHK(ensure(ctx, ctx->ws_main, (size_t)kSplitWsDoubles * 8));
  double* slab = ctx->ws_main.d();
  while (ks > 2 && (int64_t)ks * bp * bp > kSplitWsDoubles) --ks;
  if ((int64_t)ks * bp * bp > kSplitWsDoubles) {
    HIPCHK(ensure(ctx, ctx->jslab, (size_t)ks * bp * bp * 8));
    slab = ctx->jslab.d();
  }
  const double* kscale = nullptr;
  if (fitc) {  // (+1.., −1..) over the stacked K range: V₁ᵀV₁ − V₂ᵀV₂ in one launch
    double* sg = ctx->jvec.d() + 6 * kJointMaxRows + 256;
    HIPCHK(launch_sign_fill(sg, (int)kin, (int)kv, s));
    kscale = sg;
  }
  {
    GemmParams p = gp0();
    p.A = ctx->jV.d(); p.lda = bp; p.B = ctx->jV.d(); p.ldb = bp;
    p.C = slab; p.ldc = bp; p.c_kslice_stride = bp * bp;
    p.M = (int)bp; p.N = (int)bp; p.K = (int)kv; p.kscale = kscale;
    p.lower_out = 1; p.ksplit = ks;
    if ((rc = gemm(ctx, LAY_T, LAY_N, EPI_STORE, p))) return rc;
  }
  // 4. the finisher: slices summed, K** + sigma²I on the fly, both triangles, identity padding
  JointCovParams q;
  memset(&q, 0, sizeof(q));
  q.x = xt; q.b = (int)b; q.bp = (int)bp; q.d = d; q.sf2 = th.sf2; q.sn2 = th.sn2;
  for (int k = 0; k < d; ++k) q.inv_ell[k] = th.inv_ell[k];
  q.slab = slab; q.stride = bp * bp; q.ks = ks; q.out = ctx->jS.d();
  Prof pr(ctx, "joint_cov_finish", 0, 8.0 * (0.5 * ks + 1.0) * (double)bp * bp);
  HIPCHK(launch_joint_cov(q, s));
  return 0;
}

// the zeroed factor buffers and the workspace of a bp-sized potrf_inv of Sigma_b
static int joint_factor_bufs(gps_ctx* ctx, int64_t bp, bool want_L) {
  hipStream_t s = ctx->stream;
  for (DBuf* f : {&ctx->jL, want_L ? &ctx->jLo : nullptr}) {
    if (!f) continue;
    if (f->cap < (size_t)bp * bp * 8 || !factor_zeroed(ctx, f->d(), bp)) {
      HIPCHK(ensure(ctx, *f, (size_t)bp * bp * 8));
      HIPCHK(zero_factor(ctx, f->d(), bp, s));
    }
  }
  HIPCHK(ensure(ctx, ctx->jW, potrf_ws_doubles(bp) * 8));
  return 0;
}

static int predict_cov(gps_ctx* ctx, int model, int64_t r0, int64_t r1, double* mu, double* cov,
                       int64_t ldc) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = joint_ready(ctx, model)) return rc;
  if (int rc = joint_rows_ok(ctx, model, r0, r1)) return rc;
  const int64_t b = r1 - r0, bp = pad_to(b);
  ARGCHK(cov != nullptr && ldc >= b, "cov is NULL or ldc < r1 - r0");
  if (int rc = joint_cov_block(ctx, model, r0, r1, bp)) return rc;
  hipStream_t s = ctx->stream;
  if (mu) HIPCHK(hipMemcpyAsync(mu, joint_vec(ctx, bp).mu, b * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpy2DAsync(cov, (size_t)ldc * 8, ctx->jS.p, (size_t)bp * 8, (size_t)b * 8, (size_t)b,
                          hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

static int predict_joint(gps_ctx* ctx, int model, int nblock, int objective, int num_sim,
                         double beta, const double* draws, double* value, double* block_values) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = joint_ready(ctx, model)) return rc;
  const bool fitc = model == JOINT_FITC, es = objective == GPS_JOINT_ES;
  const int64_t nt = fitc ? ctx->fnt : ctx->nt;
  ARGCHK(fitc ? ctx->f_have_yt : ctx->have_yt, "the test set was set without targets (yt)");
  ARGCHK(objective == GPS_JOINT_DSS || objective == GPS_JOINT_ES,
         "objective must be GPS_JOINT_DSS or GPS_JOINT_ES");
  ARGCHK(nblock >= 1 && nblock <= 64, "nblock must be in 1..64");
  ARGCHK(nt >= nblock, "fewer test rows than blocks");
  ARGCHK(value != nullptr, "value is NULL");
  if (es) {
    ARGCHK(num_sim >= 2 && num_sim <= 8192, "num_sim must be in 2..8192");
    ARGCHK(beta > 0.0 && beta <= 2.0, "beta must be in (0, 2]");
    ARGCHK(draws != nullptr, "draws is NULL");
  }
  const std::vector<int64_t> bnd = fold_bounds(nt, nblock);
  int64_t bmax = 1;
  for (int f = 0; f < nblock; ++f) bmax = std::max(bmax, bnd[f + 1] - bnd[f]);
  ARGCHK(bmax <= kJointMaxRows, "a block may hold at most 16384 rows: use more blocks");
  const int64_t bp = pad_to(bmax);
  hipStream_t s = ctx->stream;
  const Theta& th = fitc ? ctx->fth : ctx->th;
  const double* yt = fitc ? ctx->fyt.d() : ctx->yt.d();
  int rc;
  if (es) {
    const int64_t cnt = 2 * (int64_t)num_sim * nt;
    HIPCHK(ensure(ctx, ctx->jdraws, (size_t)cnt * 8));
    HIPCHK(hipMemcpyAsync(ctx->jdraws.p, draws, (size_t)cnt * 8, hipMemcpyHostToDevice, s));
  } else {
    if ((rc = joint_factor_bufs(ctx, bp, false))) return rc;
    if ((rc = reset_info(ctx))) return rc;
  }
  for (int f = 0; f < nblock; ++f) {
    const int64_t a = bnd[f], b = bnd[f + 1] - bnd[f];
    if ((rc = joint_cov_block(ctx, model, a, a + b, bp))) return rc;
    const JointVec jv = joint_vec(ctx, bp);
    HIPCHK(launch_joint_resid(yt + a, jv.mu, (int)b, (int)bp, jv.r, s));
    if (!es) {  // ½b·log2π + ½log|Sigma| + ½‖L⁻¹r‖²
      if ((rc = potrf_inv(ctx, ctx->jS.d(), bp, ctx->jL.d(), ctx->jW.d(), jv.ld, (int)b, nullptr,
                          FactorReq{})))
        return rc;
      HIPCHK(launch_gemv_lower(ctx->jL.d(), bp, jv.r, jv.t, (int)bp, s));
      HIPCHK(launch_joint_dss(jv.ld, jv.t, (int)b, jv.vals + f, s));
      continue;
    }
    // ES: Sigma − sigma²I is positive semidefinite for both models, so lam_min >= sigma²; the
    // scale of the Newton–Schulz iteration is ‖Sigma_b‖∞ (one host read per block)
    HIPCHK(launch_norm_inf(ctx->jS.d(), bp, (int)b, jv.rowsum, jv.norms + f, s));
    HIPCHK(hipMemcpyAsync(ctx->hsmall, jv.norms + f, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    EsArgs ea;
    ea.S = num_sim;
    ea.beta = beta;
    ea.draws = ctx->jdraws.d();
    ea.lam_lb = th.sn2;
    ea.diag_ub = th.sf2 + th.sn2;
    ea.scale = ctx->hsmall[0] * (1.0 + 1e-12);
    ARGCHK(ea.scale > 0.0 && std::isfinite(ea.scale), "the block's covariance is not finite");
    if ((rc = es_fold(ctx, s, ctx->jE, false, ea, ea.draws + 2 * (int64_t)num_sim * a, b, bp,
                      ctx->jS.d(), jv.r, 0.0, jv.w, nullptr, 0, nullptr, jv.vals + f)))
      return rc;
  }
  HIPCHK(hipMemcpyAsync(ctx->hsmall, joint_vec(ctx, bp).vals, (size_t)nblock * 8,
                        hipMemcpyDeviceToHost, s));
  if (es)
    HIPCHK(hipStreamSynchronize(s));
  else if ((rc = check_info(ctx)))
    return rc;
  double tot = 0.0;
  for (int f = 0; f < nblock; ++f) {
    tot += ctx->hsmall[f];
    if (block_values) block_values[f] = ctx->hsmall[f];
  }
  *value = tot;
  return 0;
}

static int predict_draws(gps_ctx* ctx, int model, int64_t r0, int64_t r1, int nsamp,
                         const double* xi, double* out) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = joint_ready(ctx, model)) return rc;
  if (int rc = joint_rows_ok(ctx, model, r0, r1)) return rc;
  ARGCHK(xi != nullptr && out != nullptr, "xi or out is NULL");
  ARGCHK(nsamp >= 1 && nsamp <= (1 << 20), "nsamp must be in 1..2^20");
  const int64_t b = r1 - r0, bp = pad_to(b), sp = pad_to(nsamp);
  ARGCHK((double)sp * (double)bp * 8.0 <= kJointMaxVBytes,
         "the draws' buffer would exceed 8 GiB: draw fewer samples per call");
  hipStream_t s = ctx->stream;
  int rc;
  if ((rc = joint_factor_bufs(ctx, bp, true))) return rc;
  HIPCHK(ensure(ctx, ctx->jxi, (size_t)sp * bp * 8));
  HIPCHK(ensure(ctx, ctx->jout, (size_t)sp * bp * 8));
  if ((rc = joint_cov_block(ctx, model, r0, r1, bp))) return rc;
  const JointVec jv = joint_vec(ctx, bp);
  if ((rc = reset_info(ctx))) return rc;
  if ((rc = potrf_inv(ctx, ctx->jS.d(), bp, ctx->jL.d(), ctx->jW.d(), jv.ld, (int)b,
                      ctx->jLo.d(), FactorReq{})))
    return rc;
  if ((rc = check_info(ctx))) return rc;
  HIPCHK(hipMemsetAsync(ctx->jxi.p, 0, (size_t)sp * bp * 8, s));
  HIPCHK(hipMemcpy2DAsync(ctx->jxi.p, (size_t)bp * 8, xi, (size_t)b * 8, (size_t)b * 8,
                          (size_t)nsamp, hipMemcpyHostToDevice, s));
  {  // xi·Lᵀ: L lower, stored [j][k], nonzero for k <= j
    GemmParams p = gp0();
    p.A = ctx->jxi.d(); p.lda = bp; p.B = ctx->jLo.d(); p.ldb = bp; p.C = ctx->jout.d(); p.ldc = bp;
    p.M = (int)sp; p.N = (int)bp; p.K = (int)bp; p.tri = TRI_K_LE_J;
    if ((rc = gemm(ctx, LAY_N, LAY_T, EPI_STORE, p))) return rc;
  }
  HIPCHK(launch_row_add(ctx->jout.d(), bp, jv.mu, nsamp, (int)b, s));
  HIPCHK(hipMemcpy2DAsync(out, (size_t)b * 8, ctx->jout.p, (size_t)bp * 8, (size_t)b * 8,
                          (size_t)nsamp, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

}  // namespace gpsapi

extern "C" {

int gps_full_predict_cov(gps_ctx* ctx, int64_t r0, int64_t r1, double* mu, double* cov,
                         int64_t ldc) {
  return predict_cov(ctx, JOINT_FULL, r0, r1, mu, cov, ldc);
}
int gps_fitc_predict_cov(gps_ctx* ctx, int64_t r0, int64_t r1, double* mu, double* cov,
                         int64_t ldc) {
  return predict_cov(ctx, JOINT_FITC, r0, r1, mu, cov, ldc);
}
int gps_full_predict_joint(gps_ctx* ctx, int nblock, int objective, int num_sim, double beta,
                           const double* draws, double* value, double* block_values) {
  return predict_joint(ctx, JOINT_FULL, nblock, objective, num_sim, beta, draws, value,
                       block_values);
}
int gps_fitc_predict_joint(gps_ctx* ctx, int nblock, int objective, int num_sim, double beta,
                           const double* draws, double* value, double* block_values) {
  return predict_joint(ctx, JOINT_FITC, nblock, objective, num_sim, beta, draws, value,
                       block_values);
}
int gps_full_predict_draws(gps_ctx* ctx, int64_t r0, int64_t r1, int nsamp, const double* xi,
                           double* out) {
  return predict_draws(ctx, JOINT_FULL, r0, r1, nsamp, xi, out);
}
int gps_fitc_predict_draws(gps_ctx* ctx, int64_t r0, int64_t r1, int nsamp, const double* xi,
                           double* out) {
  return predict_draws(ctx, JOINT_FITC, r0, r1, nsamp, xi, out);
}

}  // extern "C"
