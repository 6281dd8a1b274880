// C-ABI, batches of full GPs of up to 512 training rows, one workgroup per problem
// (kernels_batch_full_tall.hip): gps_full_grad_batch / gps_full_train_batch's argument
// lists, checks, copies and semantics for the shape of "kin40k-FULL-compare.py" (n = 500, d = 8).
// The calls use the batch calls' own device buffers (btin, btstate, btint, btout, laid out as
// api_batch.hip lays them out; every call uploads all it reads, so nothing is carried from one
// batch call to the next) and carve the kernel's per-problem workspace (two np×np arrays) from
// btstate behind θ and the stale σ²; the resident full-GP / FITC data, any fit and the test
// buffers are not touched, nothing is sharded, and the context gains no member.
#include "api_internal.h"

namespace {

int tall_args(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
              const double* y, int64_t n, int d, const double* theta, int n_ell) {
  ARGCHK(X && y && theta, "NULL argument");
  ARGCHK(kind == GPS_ARD || kind == GPS_RBF, "kind must be GPS_ARD or GPS_RBF");
  ARGCHK(objective == GPS_OBJ_NLML || objective == GPS_OBJ_LOO_CRPS ||
             objective == GPS_OBJ_LOO_LOGS,
         "objective must be GPS_OBJ_NLML, GPS_OBJ_LOO_CRPS or GPS_OBJ_LOO_LOGS");
  ARGCHK(nprob >= 1 && nprob <= (1 << 20), "batch: nprob must be in 1..2^20");
  ARGCHK(n >= 1 && n <= GPS_BATCH_FULL_TALL_MAX_N, "batch: n must be in 1..512");
  ARGCHK(d >= 1 && d <= GPS_BATCH_MAX_D, "batch: d must be in 1..16");
  ARGCHK(n_ell == 1 || n_ell == d, "n_ell must be 1 or d");
  return 0;
}

// state layout in btstate: θ (nprob·nth), stale log σ² (nprob), padding to a multiple of 8
// doubles (the workspace is read in 16-byte pieces), then the workspace
// (nprob·batch_full_tall_ws_doubles(n))
int64_t state_head(int64_t nprob, int64_t nth) { return (nprob * (nth + 1) + 7) / 8 * 8; }

BatchFullTallParams tall_params(gps_ctx* ctx, int kind, int objective, int64_t nprob, int64_t n,
                                int d, int n_ell) {
  BatchFullTallParams tp;
  memset(&tp, 0, sizeof(tp));
  BatchParams& p = tp.b;
  p.nprob = (int)nprob; p.n = (int)n; p.d = d; p.n_ell = n_ell; p.kind = kind;
  p.objective = objective;
  p.x = ctx->btin.d();
  p.y = p.x + nprob * n * d;
  p.theta = ctx->btstate.d();
  p.stale = p.theta + nprob * (2 + n_ell);
  p.info = static_cast<int*>(ctx->btint.p);
  p.steps_done = p.info + nprob;
  tp.ws = p.theta + state_head(nprob, 2 + n_ell);
  tp.ws_stride = batch_full_tall_ws_doubles(n);
  return tp;
}

}  // namespace

extern "C" {

int gps_full_grad_tall(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                       const double* y, int64_t n, int d, const double* theta, int n_ell,
                       double* obj, double* grad, int* info) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = tall_args(ctx, kind, objective, nprob, X, y, n, d, theta, n_ell)) return rc;
  ARGCHK(grad && info, "NULL argument");
  const int64_t nth = 2 + n_ell;
  const int64_t n_ws = nprob * batch_full_tall_ws_doubles(n);
  ARGCHK(nprob * n * (d + 1) <= ((int64_t)1 << 30) && n_ws <= ((int64_t)1 << 30),
         "batch: more than 8 GiB of inputs or outputs, split the batch");
  hipStream_t s = ctx->stream;
  HIPCHK(ensure(ctx, ctx->btin, (size_t)(nprob * n * (d + 1)) * 8));
  HIPCHK(ensure(ctx, ctx->btstate, (size_t)(state_head(nprob, nth) + n_ws) * 8));
  HIPCHK(ensure(ctx, ctx->btint, (size_t)(2 * nprob) * sizeof(int)));
  HIPCHK(ensure(ctx, ctx->btout, (size_t)(nprob * (GPS_N_OBJ + nth)) * 8));
  BatchFullTallParams tp = tall_params(ctx, kind, objective, nprob, n, d, n_ell);
  BatchParams& p = tp.b;
  p.mode = BATCH_MODE_GRAD;
  p.obj = ctx->btout.d();
  p.grad = p.obj + nprob * GPS_N_OBJ;
  HIPCHK(hipMemcpyAsync((void*)p.x, X, (size_t)(nprob * n * d) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync((void*)p.y, y, (size_t)(nprob * n) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.theta, theta, (size_t)(nprob * nth) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(p.stale, 0, (size_t)nprob * 8, s));
  HIPCHK(hipMemsetAsync(p.info, 0, (size_t)(2 * nprob) * sizeof(int), s));
  {
    Prof pr(ctx, "batch_full_tall_grad", 0, 0);
    HIPCHK(launch_batch_full_tall(tp, s));
  }
  if (obj)
    HIPCHK(hipMemcpyAsync(obj, p.obj, (size_t)(nprob * GPS_N_OBJ) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(grad, p.grad, (size_t)(nprob * nth) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(info, p.info, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int gps_full_train_tall(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* theta0, int n_ell,
                        int64_t itr, double lr, const double* Xt, const double* yt, int64_t nt,
                        int flags, double* theta_out, double* values, double* thetas, double* obj,
                        double* mu, double* var, double* sc, int* info, int* steps_done) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = tall_args(ctx, kind, objective, nprob, X, y, n, d, theta0, n_ell)) return rc;
  ARGCHK(theta_out && info && steps_done, "NULL argument");
  ARGCHK(itr >= 0 && itr <= (1 << 20), "batch: itr must be in 0..2^20");
  ARGCHK(std::isfinite(lr), "batch: lr must be finite");
  ARGCHK(nt >= 0 && nt <= (1 << 24), "batch: nt must be in 0..2^24");
  ARGCHK((flags & ~GPS_BATCH_STALE_NOISE) == 0, "unknown batch flag");
  const bool pred = Xt != nullptr && nt > 0;
  if (!pred) nt = 0;
  const bool scored = pred && yt != nullptr;
  const int64_t nth = 2 + n_ell;
  const int64_t n_in = nprob * n * (d + 1) + nprob * nt * (d + 1);
  const int64_t n_out = nprob * itr * (1 + nth) + nprob * (GPS_N_OBJ + 2 * nt + GPS_N_SC);
  const int64_t n_ws = nprob * batch_full_tall_ws_doubles(n);
  ARGCHK(n_in <= ((int64_t)1 << 30) && n_out <= ((int64_t)1 << 30) && n_ws <= ((int64_t)1 << 30),
         "batch: more than 8 GiB of inputs or outputs, split the batch");
  hipStream_t s = ctx->stream;
  HIPCHK(ensure(ctx, ctx->btin, (size_t)n_in * 8));
  HIPCHK(ensure(ctx, ctx->btstate, (size_t)(state_head(nprob, nth) + n_ws) * 8));
  HIPCHK(ensure(ctx, ctx->btint, (size_t)(2 * nprob) * sizeof(int)));
  HIPCHK(ensure(ctx, ctx->btout, (size_t)n_out * 8));
  BatchFullTallParams tp = tall_params(ctx, kind, objective, nprob, n, d, n_ell);
  BatchParams& p = tp.b;
  p.mode = BATCH_MODE_TRAIN;
  p.itr = (int)itr;
  p.lr = lr;
  p.stale_noise = (flags & GPS_BATCH_STALE_NOISE) != 0;
  p.nt = (int)nt;
  double* xt_dev = const_cast<double*>(p.y) + nprob * n;
  double* yt_dev = xt_dev + nprob * nt * d;
  p.xt = pred ? xt_dev : nullptr;
  p.yt = scored ? yt_dev : nullptr;
  p.values = ctx->btout.d();
  p.thetas = p.values + nprob * itr;
  p.obj = p.thetas + nprob * itr * nth;
  p.mu = p.obj + nprob * GPS_N_OBJ;
  p.var = p.mu + nprob * nt;
  p.sc = p.var + nprob * nt;
  std::vector<double> stale((size_t)nprob);  // before any step: θ0's own noise
  for (int64_t q = 0; q < nprob; ++q) stale[(size_t)q] = theta0[q * nth + nth - 1];
  HIPCHK(hipMemcpyAsync((void*)p.x, X, (size_t)(nprob * n * d) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync((void*)p.y, y, (size_t)(nprob * n) * 8, hipMemcpyHostToDevice, s));
  if (pred)
    HIPCHK(hipMemcpyAsync(xt_dev, Xt, (size_t)(nprob * nt * d) * 8, hipMemcpyHostToDevice, s));
  if (scored)
    HIPCHK(hipMemcpyAsync(yt_dev, yt, (size_t)(nprob * nt) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.theta, theta0, (size_t)(nprob * nth) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.stale, stale.data(), (size_t)nprob * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(p.info, 0, (size_t)(2 * nprob) * sizeof(int), s));
  {
    // no launch runs more than batch_full_tall_steps(n) steps; θ, the stale σ², info and
    // steps_done stay in device memory between the launches, the last one adds the final pass
    Prof pr(ctx, "batch_full_tall_train", 0, 0);
    const int64_t per = batch_full_tall_steps(n);
    int64_t step = 0;
    do {
      const int64_t ns = std::min<int64_t>(itr - step, per);
      p.step0 = (int)step;
      p.nsteps = (int)ns;
      p.do_final = step + ns == itr;
      HIPCHK(launch_batch_full_tall(tp, s));
      step += ns;
    } while (step < itr);
  }
  HIPCHK(hipMemcpyAsync(theta_out, p.theta, (size_t)(nprob * nth) * 8, hipMemcpyDeviceToHost, s));
  if (values && itr)
    HIPCHK(hipMemcpyAsync(values, p.values, (size_t)(nprob * itr) * 8, hipMemcpyDeviceToHost, s));
  if (thetas && itr)
    HIPCHK(hipMemcpyAsync(thetas, p.thetas, (size_t)(nprob * itr * nth) * 8, hipMemcpyDeviceToHost,
                          s));
  if (obj)
    HIPCHK(hipMemcpyAsync(obj, p.obj, (size_t)(nprob * GPS_N_OBJ) * 8, hipMemcpyDeviceToHost, s));
  if (pred && mu)
    HIPCHK(hipMemcpyAsync(mu, p.mu, (size_t)(nprob * nt) * 8, hipMemcpyDeviceToHost, s));
  if (pred && var)
    HIPCHK(hipMemcpyAsync(var, p.var, (size_t)(nprob * nt) * 8, hipMemcpyDeviceToHost, s));
  if (scored && sc)
    HIPCHK(hipMemcpyAsync(sc, p.sc, (size_t)(nprob * GPS_N_SC) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(info, p.info, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(steps_done, p.steps_done, (size_t)nprob * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
