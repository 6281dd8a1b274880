// C-ABI, the seven "one workgroup per problem" batch paths (DESIGN §19, §20, §22, §24, §25, §26,
// §27, §32):
//   gps_full_{grad,train}_batch  small full GPs, n <= 128            kernels_batch.hip
//   gps_fitc_{grad,train}_batch  small FITC GPs, n <= 128, m <= 32   kernels_batch_fitc.hip
//   gps_fitc_{grad,train}_tall   FITC GPs, n <= 2048                 kernels_batch_fitc_tall.hip
//   gps_full_{grad,train}_tall   full GPs, n <= 512                  kernels_batch_full_tall.hip
//   gps_full_blockloo_{grad,train}_tall  the same on the block-LOO DSS / KC objectives
//                                                                    kernels_batch_full_tall_block.hip
//   gps_fitc_blockloo_{grad,train}_tall  the tall FITC GPs on the block-LOO DSS / KC objectives
//                                                                    kernels_batch_fitc_tall_block.hip
//   gps_fitc_train_tall_va, gps_fitc_blockloo_train_tall_va  the two tall FITC fits with a
//                                  validation set scored inside the fit, same files
//   gps_full_es_{grad,train}_tall  the tall full GPs on the block-LOO energy score, the fold work
//                                  on one workgroup per (problem, fold)
//                                                                    kernels_batch_full_tall_es.hip
// value + gradient of every problem at its own θ (and Z), and the SGD fit loops of the scripts'
// replicate loops for a whole batch with the final predictive and score bundle.  The calls own
// their device buffers:
//   btin     X | y | Xt | yt | the energy score's draws | Xv | yv (the gps_*_va calls)
//   btstate  θ (nprob·nth) | stale log σ² (nprob) | Z (nprob·m·d, FITC) | the tall kernels'
//            per-problem workspace; the full-tall path pads the head to a multiple of 8 doubles
//            (its workspace is read in 16-byte pieces)
//   btint    info | steps_done
//   btout    GRAD: obj | grad | grad_z | value | fold_values (the last two: block-LOO);
//            TRAIN: values | thetas | obj | mu | var | sc | va_sc | va_z (FITC VA, when asked for)
// Every call uploads all it reads, so nothing is carried from one batch call to the next; the
// resident full-GP / FITC data, any fit and the test buffers are not touched, and nothing is
// sharded, so a communicator does not matter.  A path is one Path constant: its limit on n, its
// objective rule, its workspace, its steps-per-launch rule, its launcher and its profiling tags;
// everything else is the two routines grad_call and train_call.
#include <type_traits>

#include "api_internal.h"

namespace {

constexpr int64_t kMaxDoubles = (int64_t)1 << 30;  // 8 GiB of doubles
const char* const kTooBig = "batch: more than 8 GiB of inputs or outputs, split the batch";

template <class P>
constexpr bool kFitc = std::is_same<P, BatchFitcParams>::value;

// what only the block-LOO paths have: the fold count and BATCH_MODE_GRAD's two extra outputs; the
// energy score's draws (device), their sets per problem, num_sim and β
struct Block {
  int nfold;
  double *value, *fold_values;
  const double* draws = nullptr;
  int64_t draw_sets = 0;
  int num_sim = 0;
  double beta = 0.0;
  BatchVaParams va = {};  // the FITC VA paths' validation rows and outputs (device)
};

template <class P>
struct Path {
  int64_t max_n;
  const char* n_msg;
  const char *grad_tag, *train_tag;
  // workspace doubles per problem behind the state, or NULL
  int64_t (*ws)(int64_t n, int m, int nfold, int num_sim);
  bool pad;                         // the state's head is padded to a multiple of 8 doubles
  int (*steps)(int64_t n);          // SGD steps one launch may run
  // (ctx: for a path that times the launches of its sequence one by one)
  hipError_t (*launch)(gps_ctx* ctx, const P& p, double* ws, int64_t ws_stride, const Block& b,
                       hipStream_t s);
  bool block;                       // the objective is a GPS_BLOCK_* code over nfold folds
  bool es = false;                  // that code is GPS_BLOCK_ES: draws, num_sim and β come with it
  // a VA path whose steps-per-launch rule also caps the validation rows a launch streams
  int (*va_steps)(int64_t n, int64_t nv, int64_t va_every) = nullptr;
};

const Path<BatchParams> kFull = {
    GPS_SURFACE_MAX_N, "batch: n must be in 1..128", "batch_grad", "batch_train", nullptr, false,
    [](int64_t) { return kBatchStepsPerLaunch; },
    [](gps_ctx*, const BatchParams& p, double*, int64_t, const Block&, hipStream_t s) {
      return launch_batch(p, s);
    },
    false};
const Path<BatchFitcParams> kFitcSmall = {
    GPS_SURFACE_MAX_N, "batch: n must be in 1..128", "batch_fitc_grad", "batch_fitc_train", nullptr,
    false, [](int64_t) { return kBatchStepsPerLaunch; },
    [](gps_ctx*, const BatchFitcParams& p, double*, int64_t, const Block&, hipStream_t s) {
      return launch_batch_fitc(p, s);
    },
    false};
const Path<BatchFitcParams> kFitcTall = {
    GPS_BATCH_FITC_TALL_MAX_N, "batch: n must be in 1..2048", "batch_fitc_tall_grad",
    "batch_fitc_tall_train", [](int64_t n, int m, int, int) { return batch_fitc_tall_ws_doubles(n, m); },
    false, batch_fitc_tall_steps,
    [](gps_ctx*, const BatchFitcParams& p, double* ws, int64_t stride, const Block&,
       hipStream_t s) {
      return launch_batch_fitc_tall(BatchFitcTallParams{p, ws, stride}, s);
    },
    false};
const Path<BatchParams> kFullTall = {
    GPS_BATCH_FULL_TALL_MAX_N, "batch: n must be in 1..512", "batch_full_tall_grad",
    "batch_full_tall_train", [](int64_t n, int, int, int) { return batch_full_tall_ws_doubles(n); },
    true, batch_full_tall_steps,
    [](gps_ctx*, const BatchParams& p, double* ws, int64_t stride, const Block&, hipStream_t s) {
      return launch_batch_full_tall(BatchFullTallParams{p, ws, stride}, s);
    },
    false};
const Path<BatchParams> kFullTallBlock = {
    GPS_BATCH_FULL_TALL_MAX_N, "batch: n must be in 1..512", "batch_full_tall_block_grad",
    "batch_full_tall_block_train",
    [](int64_t n, int, int nfold, int) { return batch_full_tall_block_ws_doubles(n, nfold); }, true,
    batch_full_tall_steps,
    [](gps_ctx*, const BatchParams& p, double* ws, int64_t stride, const Block& b,
       hipStream_t s) {
      return launch_batch_full_tall_block(
          BatchFullTallBlockParams{p, ws, stride, b.nfold, 0, b.value, b.fold_values}, s);
    },
    true};
// the two tall full-GP paths with a validation set scored inside the fit: training
// calls only, the grad tags are never used
const Path<BatchParams> kFullTallVa = {
    GPS_BATCH_FULL_TALL_MAX_N, "batch: n must be in 1..512", "batch_full_tall_va_grad",
    "batch_full_tall_va_train", [](int64_t n, int, int, int) { return batch_full_tall_ws_doubles(n); },
    true, batch_full_tall_steps,
    [](gps_ctx*, const BatchParams& p, double* ws, int64_t stride, const Block&, hipStream_t s) {
      return launch_batch_full_tall_va(BatchFullTallParams{p, ws, stride}, s);
    },
    false};
const Path<BatchParams> kFullTallBlockVa = {
    GPS_BATCH_FULL_TALL_MAX_N, "batch: n must be in 1..512", "batch_full_tall_block_va_grad",
    "batch_full_tall_block_va_train",
    [](int64_t n, int, int nfold, int) { return batch_full_tall_block_ws_doubles(n, nfold); }, true,
    batch_full_tall_steps,
    [](gps_ctx*, const BatchParams& p, double* ws, int64_t stride, const Block& b,
       hipStream_t s) {
      return launch_batch_full_tall_block_va(
          BatchFullTallBlockParams{p, ws, stride, b.nfold, 0, b.value, b.fold_values}, s);
    },
    true};
const Path<BatchFitcParams> kFitcTallBlock = {
    GPS_BATCH_FITC_TALL_MAX_N, "batch: n must be in 1..2048", "batch_fitc_tall_block_grad",
    "batch_fitc_tall_block_train",
    [](int64_t n, int m, int nfold, int) { return batch_fitc_tall_block_ws_doubles(n, m, nfold); },
    false, batch_fitc_tall_block_steps,
    [](gps_ctx*, const BatchFitcParams& p, double* ws, int64_t stride, const Block& b,
       hipStream_t s) {
      return launch_batch_fitc_tall_block(
          BatchFitcTallBlockParams{p, ws, stride, b.nfold, b.value, b.fold_values}, s);
    },
    true};
// the two tall FITC paths with a validation set scored inside the fit: training calls
// only, the grad tags are never used; the validation members travel in Block
const Path<BatchFitcParams> kFitcTallVa = {
    GPS_BATCH_FITC_TALL_MAX_N, "batch: n must be in 1..2048", "batch_fitc_tall_va_grad",
    "batch_fitc_tall_va_train",
    [](int64_t n, int m, int, int) { return batch_fitc_tall_ws_doubles(n, m); }, false,
    batch_fitc_tall_steps,
    [](gps_ctx*, const BatchFitcParams& p, double* ws, int64_t stride, const Block& b,
       hipStream_t s) {
      return launch_batch_fitc_tall_va(BatchFitcTallVaParams{{p, ws, stride}, b.va}, s);
    },
    false, false, batch_fitc_tall_va_steps};
const Path<BatchFitcParams> kFitcTallBlockVa = {
    GPS_BATCH_FITC_TALL_MAX_N, "batch: n must be in 1..2048", "batch_fitc_tall_block_va_grad",
    "batch_fitc_tall_block_va_train",
    [](int64_t n, int m, int nfold, int) { return batch_fitc_tall_block_ws_doubles(n, m, nfold); },
    false, batch_fitc_tall_block_steps,
    [](gps_ctx*, const BatchFitcParams& p, double* ws, int64_t stride, const Block& b,
       hipStream_t s) {
      return launch_batch_fitc_tall_block_va(
          BatchFitcTallBlockVaParams{{p, ws, stride, b.nfold, b.value, b.fold_values}, b.va}, s);
    },
    true, false, batch_fitc_tall_block_va_steps};
const Path<BatchParams> kFullTallEs = {
    GPS_BATCH_FULL_TALL_MAX_N, "batch: n must be in 1..512", "batch_full_tall_es_grad",
    "batch_full_tall_es_train",
    [](int64_t n, int, int nfold, int num_sim) {
      return batch_full_tall_es_ws_doubles(n, nfold, num_sim);
    },
    true, [](int64_t) { return 1; },  // a step is a launch sequence of its own
    [](gps_ctx* ctx, const BatchParams& p, double* ws, int64_t stride, const Block& b,
       hipStream_t s) {
      const BatchFullTallEsParams tp = {p, ws, stride, b.nfold, b.num_sim, b.beta, b.draws,
                                        b.draw_sets, b.value, b.fold_values};
      // the sequence's launches under tags of their own, inside the call's: what the launch-length
      // rule is held against
      static const char* const tags[ES_PHASES] = {"batch_full_tall_es_forward",
                                                  "batch_full_tall_es_folds",
                                                  "batch_full_tall_es_tail",
                                                  "batch_full_tall_es_final"};
      for (int ph = 0; ph < ES_PHASES; ++ph) {
        Prof pr(ctx, tags[ph], 0, 0);
        const hipError_t e = launch_batch_full_tall_es(tp, ph, s);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    },
    true, true};

// what every entry is given; Z and m are NULL and 0, and kind is unused, where the entry has none
struct Problem {
  int kind, objective;
  int64_t nprob;
  const double *X, *y;
  int64_t n;
  int d;
  const double* Z;
  int m;
  const double* theta;
  int n_ell;
  int nfold = 0;  // the block-LOO path's fold count
  // the energy score: num_sim, β, the draws (host) and their sets per problem
  int num_sim = 0;
  double beta = 0.0;
  const double* draws = nullptr;
  int64_t draw_sets = 0;
  int64_t n_draws() const { return draws ? nprob * draw_sets * 2 * num_sim * n : 0; }
};

template <class P>
int check_problem(gps_ctx* ctx, const Path<P>& path, const Problem& a) {
  ARGCHK(a.X && a.y && (!kFitc<P> || a.Z) && a.theta, "NULL argument");
  if (!kFitc<P>) ARGCHK(a.kind == GPS_ARD || a.kind == GPS_RBF, "kind must be GPS_ARD or GPS_RBF");
  if (path.es)
    ARGCHK(a.draws, "NULL argument");
  else if (path.block)
    ARGCHK(a.objective == GPS_BLOCK_DSS || a.objective == GPS_BLOCK_KC,
           "objective must be GPS_BLOCK_DSS or GPS_BLOCK_KC");
  else
    ARGCHK(a.objective == GPS_OBJ_NLML || a.objective == GPS_OBJ_LOO_CRPS ||
               a.objective == GPS_OBJ_LOO_LOGS,
           "objective must be GPS_OBJ_NLML, GPS_OBJ_LOO_CRPS or GPS_OBJ_LOO_LOGS");
  ARGCHK(a.nprob >= 1 && a.nprob <= (1 << 20), "batch: nprob must be in 1..2^20");
  ARGCHK(a.n >= 1 && a.n <= path.max_n, path.n_msg);
  if (path.block)
    ARGCHK(a.nfold >= 2 && a.nfold <= GPS_BATCH_BLOCK_MAX_FOLDS && a.nfold <= a.n,
           "batch: nfold must be in 2..32 and at most n");
  if (kFitc<P>) ARGCHK(a.m >= 1 && a.m <= GPS_BATCH_FITC_MAX_M, "batch: m must be in 1..32");
  ARGCHK(a.d >= 1 && a.d <= GPS_BATCH_MAX_D, "batch: d must be in 1..16");
  ARGCHK(a.n_ell == 1 || a.n_ell == a.d, "n_ell must be 1 or d");
  if (path.es) {
    ARGCHK((a.n + a.nfold - 1) / a.nfold <= GPS_BATCH_ES_MAX_FOLD,
           "batch: an energy-score fold holds at most 128 rows (ceil(n / nfold) <= 128: a fold's "
           "O(b^3) square-root work has to fit one launch of ~20 ms), use more folds");
    ARGCHK(a.num_sim >= 2 && a.num_sim <= GPS_BATCH_ES_MAX_SIM, "batch: num_sim must be in 2..512");
    ARGCHK(a.beta > 0.0 && a.beta <= 2.0, "beta must be in (0, 2]");
    ARGCHK(a.draw_sets >= 1, "batch: draw_sets must be at least 1");
  }
  return 0;
}

// the validation set of a gps_*_va call: rows, targets, their count a problem, the checkpoint
// spacing and the output
struct Va {
  const double *Xv, *yv;
  int64_t nv, va_every;
  double* va_sc;
  double* va_z = nullptr;  // the FITC calls' Z of every row, or NULL
};

// Sizes the four buffers (nt test rows and nv validation rows a problem, n_out output doubles, n_ws
// workspace doubles in all) and fills p with the problem and the carving of btin, btstate and btint; *ws is the
// workspace behind the state's head.
template <class P>
int carve(gps_ctx* ctx, const Path<P>& path, const Problem& a, int64_t nt, int64_t n_out,
          int64_t n_ws, P& p, double** ws, int64_t nv = 0) {
  const int64_t nprob = a.nprob, nth = 2 + a.n_ell, nz = (int64_t)a.m * a.d;
  int64_t head = nprob * (nth + 1 + nz);
  if (path.pad) head = (head + 7) / 8 * 8;
  HIPCHK(ensure(ctx, ctx->btin,
                (size_t)(nprob * a.n * (a.d + 1) + nprob * (nt + nv) * (a.d + 1) + a.n_draws()) *
                    8));
  HIPCHK(ensure(ctx, ctx->btstate, (size_t)(head + n_ws) * 8));
  HIPCHK(ensure(ctx, ctx->btint, (size_t)(2 * nprob) * sizeof(int)));
  HIPCHK(ensure(ctx, ctx->btout, (size_t)n_out * 8));
  memset(&p, 0, sizeof(p));
  p.nprob = (int)nprob; p.n = (int)a.n; p.d = a.d; p.n_ell = a.n_ell;
  p.objective = a.objective;
  p.x = ctx->btin.d();
  p.y = p.x + nprob * a.n * a.d;
  p.theta = ctx->btstate.d();
  p.stale = p.theta + nprob * nth;
  if constexpr (kFitc<P>) {
    p.m = a.m;
    p.z = p.stale + nprob;
  } else {
    p.kind = a.kind;
  }
  p.info = static_cast<int*>(ctx->btint.p);
  p.steps_done = p.info + nprob;
  *ws = p.theta + head;
  return 0;
}

// X, y, the test rows where given, θ, Z and the stale σ² (zero without `stale`) to the device;
// info and steps_done start at zero
template <class P>
int upload(gps_ctx* ctx, const Problem& a, const P& p, const double* Xt, const double* yt,
           const double* stale) {
  const int64_t nprob = a.nprob, nth = 2 + a.n_ell;
  hipStream_t s = ctx->stream;
  HIPCHK(hipMemcpyAsync((void*)p.x, a.X, (size_t)(nprob * a.n * a.d) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync((void*)p.y, a.y, (size_t)(nprob * a.n) * 8, hipMemcpyHostToDevice, s));
  if (p.xt)
    HIPCHK(hipMemcpyAsync((void*)p.xt, Xt, (size_t)(nprob * p.nt * a.d) * 8, hipMemcpyHostToDevice,
                          s));
  if (p.yt)
    HIPCHK(hipMemcpyAsync((void*)p.yt, yt, (size_t)(nprob * p.nt) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.theta, a.theta, (size_t)(nprob * nth) * 8, hipMemcpyHostToDevice, s));
  if constexpr (kFitc<P>)
    HIPCHK(hipMemcpyAsync(p.z, a.Z, (size_t)(nprob * a.m * a.d) * 8, hipMemcpyHostToDevice, s));
  if (stale)
    HIPCHK(hipMemcpyAsync(p.stale, stale, (size_t)nprob * 8, hipMemcpyHostToDevice, s));
  else
    HIPCHK(hipMemsetAsync(p.stale, 0, (size_t)nprob * 8, s));
  HIPCHK(hipMemsetAsync(p.info, 0, (size_t)(2 * nprob) * sizeof(int), s));
  if (a.draws)  // behind the test rows
    HIPCHK(hipMemcpyAsync((void*)(p.y + nprob * a.n + nprob * p.nt * (a.d + 1)), a.draws,
                          (size_t)a.n_draws() * 8, hipMemcpyHostToDevice, s));
  return 0;
}

// count elements of T back to the host; an output that is NULL or empty is skipped
template <class T>
int download(gps_ctx* ctx, T* dst, const T* src, int64_t count) {
  if (dst && count > 0)
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

template <class P>
int grad_call(gps_ctx* ctx, const Path<P>& path, const Problem& a, double* obj, double* grad,
              double* grad_z, int* info, double* value = nullptr, double* fold_values = nullptr) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = check_problem(ctx, path, a)) return rc;
  ARGCHK(grad && (!kFitc<P> || grad_z) && info && (!path.block || value), "NULL argument");
  const int64_t nprob = a.nprob, nth = 2 + a.n_ell, nz = (int64_t)a.m * a.d;
  const int64_t stride = path.ws ? path.ws(a.n, a.m, a.nfold, a.num_sim) : 0;
  const int64_t n_ws = nprob * stride;
  const int64_t n_blk = path.block ? nprob * (1 + a.nfold) : 0;
  if (path.ws)  // the small paths' value + gradient calls have no such guard
    ARGCHK(nprob * a.n * (a.d + 1) + nprob * nz + a.n_draws() <= kMaxDoubles &&
               n_ws <= kMaxDoubles, kTooBig);
  P p;
  double* ws;
  if (int rc = carve(ctx, path, a, 0, nprob * (GPS_N_OBJ + nth + nz) + n_blk, n_ws, p, &ws))
    return rc;
  p.mode = BATCH_MODE_GRAD;
  p.obj = ctx->btout.d();
  p.grad = p.obj + nprob * GPS_N_OBJ;
  if constexpr (kFitc<P>) p.grad_z = p.grad + nprob * nth;
  Block blk = {a.nfold, nullptr, nullptr, p.y + nprob * a.n, a.draw_sets, a.num_sim, a.beta};
  if (path.block) {
    blk.value = p.grad + nprob * (nth + nz);
    blk.fold_values = blk.value + nprob;
  }
  if (int rc = upload(ctx, a, p, nullptr, nullptr, nullptr)) return rc;
  {
    Prof pr(ctx, path.grad_tag, 0, 0);
    HIPCHK(path.launch(ctx, p, ws, stride, blk, ctx->stream));
  }
  if (path.block) {
    if (int rc = download(ctx, value, blk.value, nprob)) return rc;
    if (int rc = download(ctx, fold_values, blk.fold_values, nprob * a.nfold)) return rc;
  }
  if (int rc = download(ctx, obj, p.obj, nprob * GPS_N_OBJ)) return rc;
  if (int rc = download(ctx, grad, p.grad, nprob * nth)) return rc;
  if constexpr (kFitc<P>)
    if (int rc = download(ctx, grad_z, p.grad_z, nprob * nz)) return rc;
  if (int rc = download(ctx, info, p.info, nprob)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

template <class P>
int train_call(gps_ctx* ctx, const Path<P>& path, const Problem& a, int64_t itr, double lr,
               double lr_z, const double* Xt, const double* yt, int64_t nt, int flags,
               double* theta_out, double* z_out, double* values, double* thetas, double* obj,
               double* mu, double* var, double* sc, int* info, int* steps_done,
               const Va* va = nullptr) {
  if (int rc = bind(ctx)) return rc;
  if (int rc = check_problem(ctx, path, a)) return rc;
  ARGCHK(theta_out && (!kFitc<P> || z_out) && info && steps_done, "NULL argument");
  ARGCHK(itr >= 0 && itr <= (1 << 20), "batch: itr must be in 0..2^20");
  ARGCHK(std::isfinite(lr), "batch: lr must be finite");
  if (kFitc<P>) ARGCHK(std::isfinite(lr_z), "batch: lr_z must be finite");
  ARGCHK(nt >= 0 && nt <= (1 << 24), "batch: nt must be in 0..2^24");
  if (va) {
    ARGCHK(va->nv >= 1 && va->nv <= (1 << 24), "batch: nv must be in 1..2^24");
    ARGCHK(va->va_every >= 1 && va->va_every <= (1 << 20), "batch: va_every must be in 1..2^20");
    ARGCHK(va->Xv, "batch: Xv is NULL, a validated fit needs its validation rows");
    ARGCHK(va->yv, "batch: yv is NULL, a validated fit needs its validation targets");
    ARGCHK(va->va_sc, "batch: va_sc is NULL, a validated fit needs room for its score rows");
  }
  ARGCHK((flags & ~GPS_BATCH_STALE_NOISE) == 0, "unknown batch flag");
  if (path.es)
    ARGCHK(a.draw_sets <= std::max<int64_t>(itr, 1), "batch: draw_sets must be at most max(itr, 1)");
  const bool pred = Xt != nullptr && nt > 0;
  if (!pred) nt = 0;
  const bool scored = pred && yt != nullptr;
  const int64_t nprob = a.nprob, nth = 2 + a.n_ell, nz = (int64_t)a.m * a.d;
  // the validation rows and the rows of va_sc: the checkpoints and the final pass
  const int64_t nv = va ? va->nv : 0;
  const int64_t nva = va ? (itr + va->va_every - 1) / va->va_every + 1 : 0;
  const int64_t n_in =
      nprob * a.n * (a.d + 1) + nprob * (nt + nv) * (a.d + 1) + nprob * nz + a.n_draws();
  const int64_t n_out = nprob * itr * (1 + nth) + nprob * (GPS_N_OBJ + 2 * nt + GPS_N_SC) +
                        nprob * nva * GPS_N_SC + (va && va->va_z ? nprob * nva * nz : 0);
  const int64_t stride = path.ws ? path.ws(a.n, a.m, a.nfold, a.num_sim) : 0;
  const int64_t n_ws = nprob * stride;
  ARGCHK(n_in <= kMaxDoubles && n_out <= kMaxDoubles && n_ws <= kMaxDoubles, kTooBig);
  P p;
  double* ws;
  if (int rc = carve(ctx, path, a, nt, n_out, n_ws, p, &ws, nv)) return rc;
  p.mode = BATCH_MODE_TRAIN;
  p.itr = (int)itr;
  p.lr = lr;
  if constexpr (kFitc<P>) p.lr_z = lr_z;
  p.stale_noise = (flags & GPS_BATCH_STALE_NOISE) != 0;
  p.nt = (int)nt;
  const double* xt_dev = p.y + nprob * a.n;
  p.xt = pred ? xt_dev : nullptr;
  p.yt = scored ? xt_dev + nprob * nt * a.d : nullptr;
  p.values = ctx->btout.d();
  p.thetas = p.values + nprob * itr;
  p.obj = p.thetas + nprob * itr * nth;
  p.mu = p.obj + nprob * GPS_N_OBJ;
  p.var = p.mu + nprob * nt;
  p.sc = p.var + nprob * nt;
  BatchVaParams dv = {};
  if (va) {  // Xv | yv behind the test rows and the draws, va_sc | va_z behind sc
    dv.xv = xt_dev + nprob * nt * (a.d + 1) + a.n_draws();
    dv.yv = dv.xv + nprob * nv * a.d;
    dv.nv = (int)nv;
    dv.va_every = (int)va->va_every;
    dv.va_sc = p.sc + nprob * GPS_N_SC;
    dv.va_z = va->va_z ? dv.va_sc + nprob * nva * GPS_N_SC : nullptr;
    if constexpr (!kFitc<P>) {
      p.xv = dv.xv;
      p.yv = dv.yv;
      p.nv = dv.nv;
      p.va_every = dv.va_every;
      p.va_sc = dv.va_sc;
    }
  }
  std::vector<double> stale((size_t)nprob);  // before any step: θ0's own noise
  for (int64_t q = 0; q < nprob; ++q) stale[(size_t)q] = a.theta[q * nth + nth - 1];
  if (int rc = upload(ctx, a, p, Xt, yt, stale.data())) return rc;
  if (va) {
    HIPCHK(hipMemcpyAsync((void*)dv.xv, va->Xv, (size_t)(nprob * nv * a.d) * 8,
                          hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync((void*)dv.yv, va->yv, (size_t)(nprob * nv) * 8, hipMemcpyHostToDevice,
                          ctx->stream));
  }
  {
    // no launch runs more than path.steps(n) steps; θ, Z, the stale σ², info and steps_done stay
    // in device memory between the launches, the last one adds the final pass
    Prof pr(ctx, path.train_tag, 0, 0);
    const int64_t per =
        va && path.va_steps ? path.va_steps(a.n, nv, va->va_every) : path.steps(a.n);
    int64_t step = 0;
    do {
      const int64_t ns = std::min<int64_t>(itr - step, per);
      p.step0 = (int)step;
      p.nsteps = (int)ns;
      p.do_final = step + ns == itr;
      HIPCHK(path.launch(ctx, p, ws, stride,
                         Block{a.nfold, nullptr, nullptr, p.y + nprob * a.n + nprob * nt * (a.d + 1),
                               a.draw_sets, a.num_sim, a.beta, dv},
                         ctx->stream));
      step += ns;
    } while (step < itr);
  }
  if (int rc = download(ctx, theta_out, p.theta, nprob * nth)) return rc;
  if constexpr (kFitc<P>)
    if (int rc = download(ctx, z_out, p.z, nprob * nz)) return rc;
  if (int rc = download(ctx, values, p.values, nprob * itr)) return rc;
  if (int rc = download(ctx, thetas, p.thetas, nprob * itr * nth)) return rc;
  if (int rc = download(ctx, obj, p.obj, nprob * GPS_N_OBJ)) return rc;
  if (int rc = download(ctx, mu, p.mu, nprob * nt)) return rc;
  if (int rc = download(ctx, var, p.var, nprob * nt)) return rc;
  if (int rc = download(ctx, scored ? sc : nullptr, p.sc, nprob * GPS_N_SC)) return rc;
  if (va) {
    if (int rc = download(ctx, va->va_sc, dv.va_sc, nprob * nva * GPS_N_SC)) return rc;
    if (int rc = download(ctx, va->va_z, dv.va_z, nprob * nva * nz)) return rc;
  }
  if (int rc = download(ctx, info, p.info, nprob)) return rc;
  if (int rc = download(ctx, steps_done, p.steps_done, nprob)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // namespace

extern "C" {

int gps_full_grad_batch(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* theta, int n_ell,
                        double* obj, double* grad, int* info) {
  return grad_call(ctx, kFull, {kind, objective, nprob, X, y, n, d, nullptr, 0, theta, n_ell}, obj,
                   grad, nullptr, info);
}

int gps_full_train_batch(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                         const double* y, int64_t n, int d, const double* theta0, int n_ell,
                         int64_t itr, double lr, const double* Xt, const double* yt, int64_t nt,
                         int flags, double* theta_out, double* values, double* thetas, double* obj,
                         double* mu, double* var, double* sc, int* info, int* steps_done) {
  return train_call(ctx, kFull, {kind, objective, nprob, X, y, n, d, nullptr, 0, theta0, n_ell},
                    itr, lr, 0.0, Xt, yt, nt, flags, theta_out, nullptr, values, thetas, obj, mu,
                    var, sc, info, steps_done);
}

int gps_full_grad_tall(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                       const double* y, int64_t n, int d, const double* theta, int n_ell,
                       double* obj, double* grad, int* info) {
  return grad_call(ctx, kFullTall, {kind, objective, nprob, X, y, n, d, nullptr, 0, theta, n_ell},
                   obj, grad, nullptr, info);
}

int gps_full_train_tall(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* theta0, int n_ell,
                        int64_t itr, double lr, const double* Xt, const double* yt, int64_t nt,
                        int flags, double* theta_out, double* values, double* thetas, double* obj,
                        double* mu, double* var, double* sc, int* info, int* steps_done) {
  return train_call(ctx, kFullTall, {kind, objective, nprob, X, y, n, d, nullptr, 0, theta0, n_ell},
                    itr, lr, 0.0, Xt, yt, nt, flags, theta_out, nullptr, values, thetas, obj, mu,
                    var, sc, info, steps_done);
}

int gps_full_blockloo_grad_tall(gps_ctx* ctx, int kind, int objective, int nfold, int64_t nprob,
                                const double* X, const double* y, int64_t n, int d,
                                const double* theta, int n_ell, double* value,
                                double* fold_values, double* obj, double* grad, int* info) {
  return grad_call(ctx, kFullTallBlock,
                   {kind, objective, nprob, X, y, n, d, nullptr, 0, theta, n_ell, nfold}, obj, grad,
                   nullptr, info, value, fold_values);
}

int gps_full_blockloo_train_tall(gps_ctx* ctx, int kind, int objective, int nfold, int64_t nprob,
                                 const double* X, const double* y, int64_t n, int d,
                                 const double* theta0, int n_ell, int64_t itr, double lr,
                                 const double* Xt, const double* yt, int64_t nt, int flags,
                                 double* theta_out, double* values, double* thetas, double* obj,
                                 double* mu, double* var, double* sc, int* info, int* steps_done) {
  return train_call(ctx, kFullTallBlock,
                    {kind, objective, nprob, X, y, n, d, nullptr, 0, theta0, n_ell, nfold}, itr, lr,
                    0.0, Xt, yt, nt, flags, theta_out, nullptr, values, thetas, obj, mu, var, sc,
                    info, steps_done);
}

int gps_full_train_tall_va(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                           const double* y, int64_t n, int d, const double* theta0, int n_ell,
                           int64_t itr, double lr, const double* Xv, const double* yv, int64_t nv,
                           int64_t va_every, const double* Xt, const double* yt, int64_t nt,
                           int flags, double* theta_out, double* values, double* thetas,
                           double* obj, double* mu, double* var, double* sc, double* va_sc,
                           int* info, int* steps_done) {
  const Va va = {Xv, yv, nv, va_every, va_sc};
  return train_call(ctx, kFullTallVa,
                    {kind, objective, nprob, X, y, n, d, nullptr, 0, theta0, n_ell}, itr, lr, 0.0,
                    Xt, yt, nt, flags, theta_out, nullptr, values, thetas, obj, mu, var, sc, info,
                    steps_done, &va);
}

int gps_full_blockloo_train_tall_va(gps_ctx* ctx, int kind, int objective, int nfold,
                                    int64_t nprob, const double* X, const double* y, int64_t n,
                                    int d, const double* theta0, int n_ell, int64_t itr, double lr,
                                    const double* Xv, const double* yv, int64_t nv,
                                    int64_t va_every, const double* Xt, const double* yt,
                                    int64_t nt, int flags, double* theta_out, double* values,
                                    double* thetas, double* obj, double* mu, double* var,
                                    double* sc, double* va_sc, int* info, int* steps_done) {
  const Va va = {Xv, yv, nv, va_every, va_sc};
  return train_call(ctx, kFullTallBlockVa,
                    {kind, objective, nprob, X, y, n, d, nullptr, 0, theta0, n_ell, nfold}, itr, lr,
                    0.0, Xt, yt, nt, flags, theta_out, nullptr, values, thetas, obj, mu, var, sc,
                    info, steps_done, &va);
}

int gps_full_es_grad_tall(gps_ctx* ctx, int kind, int nfold, int num_sim, double beta,
                          int64_t nprob, const double* X, const double* y, int64_t n, int d,
                          const double* theta, int n_ell, const double* draws, double* value,
                          double* fold_values, double* obj, double* grad, int* info) {
  return grad_call(ctx, kFullTallEs,
                   {kind, GPS_BLOCK_ES, nprob, X, y, n, d, nullptr, 0, theta, n_ell, nfold, num_sim,
                    beta, draws, 1},
                   obj, grad, nullptr, info, value, fold_values);
}

int gps_full_es_train_tall(gps_ctx* ctx, int kind, int nfold, int num_sim, double beta,
                           int64_t nprob, const double* X, const double* y, int64_t n, int d,
                           const double* theta0, int n_ell, int64_t itr, double lr,
                           const double* Xt, const double* yt, int64_t nt, int flags,
                           const double* draws, int64_t draw_sets, double* theta_out,
                           double* values, double* thetas, double* obj, double* mu, double* var,
                           double* sc, int* info, int* steps_done) {
  return train_call(ctx, kFullTallEs,
                    {kind, GPS_BLOCK_ES, nprob, X, y, n, d, nullptr, 0, theta0, n_ell, nfold,
                     num_sim, beta, draws, draw_sets},
                    itr, lr, 0.0, Xt, yt, nt, flags, theta_out, nullptr, values, thetas, obj, mu,
                    var, sc, info, steps_done);
}

int gps_fitc_grad_batch(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* Z, int m,
                        const double* theta, int n_ell, double* obj, double* grad, double* grad_z,
                        int* info) {
  return grad_call(ctx, kFitcSmall, {0, objective, nprob, X, y, n, d, Z, m, theta, n_ell}, obj,
                   grad, grad_z, info);
}

int gps_fitc_train_batch(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                         const double* y, int64_t n, int d, const double* Z0, int m,
                         const double* theta0, int n_ell, int64_t itr, double lr, double lr_z,
                         const double* Xt, const double* yt, int64_t nt, int flags,
                         double* theta_out, double* z_out, double* values, double* thetas,
                         double* obj, double* mu, double* var, double* sc, int* info,
                         int* steps_done) {
  return train_call(ctx, kFitcSmall, {0, objective, nprob, X, y, n, d, Z0, m, theta0, n_ell}, itr,
                    lr, lr_z, Xt, yt, nt, flags, theta_out, z_out, values, thetas, obj, mu, var, sc,
                    info, steps_done);
}

int gps_fitc_grad_tall(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                       const double* y, int64_t n, int d, const double* Z, int m,
                       const double* theta, int n_ell, double* obj, double* grad, double* grad_z,
                       int* info) {
  return grad_call(ctx, kFitcTall, {0, objective, nprob, X, y, n, d, Z, m, theta, n_ell}, obj, grad,
                   grad_z, info);
}

int gps_fitc_train_tall(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* Z0, int m,
                        const double* theta0, int n_ell, int64_t itr, double lr, double lr_z,
                        const double* Xt, const double* yt, int64_t nt, int flags,
                        double* theta_out, double* z_out, double* values, double* thetas,
                        double* obj, double* mu, double* var, double* sc, int* info,
                        int* steps_done) {
  return train_call(ctx, kFitcTall, {0, objective, nprob, X, y, n, d, Z0, m, theta0, n_ell}, itr,
                    lr, lr_z, Xt, yt, nt, flags, theta_out, z_out, values, thetas, obj, mu, var, sc,
                    info, steps_done);
}

int gps_fitc_blockloo_grad_tall(gps_ctx* ctx, int objective, int nfold, int64_t nprob,
                                const double* X, const double* y, int64_t n, int d,
                                const double* Z, int m, const double* theta, int n_ell,
                                double* value, double* fold_values, double* obj, double* grad,
                                double* grad_z, int* info) {
  return grad_call(ctx, kFitcTallBlock,
                   {0, objective, nprob, X, y, n, d, Z, m, theta, n_ell, nfold}, obj, grad, grad_z,
                   info, value, fold_values);
}

int gps_fitc_blockloo_train_tall(gps_ctx* ctx, int objective, int nfold, int64_t nprob,
                                 const double* X, const double* y, int64_t n, int d,
                                 const double* Z0, int m, const double* theta0, int n_ell,
                                 int64_t itr, double lr, double lr_z, const double* Xt,
                                 const double* yt, int64_t nt, int flags, double* theta_out,
                                 double* z_out, double* values, double* thetas, double* obj,
                                 double* mu, double* var, double* sc, int* info, int* steps_done) {
  return train_call(ctx, kFitcTallBlock,
                    {0, objective, nprob, X, y, n, d, Z0, m, theta0, n_ell, nfold}, itr, lr, lr_z,
                    Xt, yt, nt, flags, theta_out, z_out, values, thetas, obj, mu, var, sc, info,
                    steps_done);
}

int gps_fitc_train_tall_va(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                           const double* y, int64_t n, int d, const double* Z0, int m,
                           const double* theta0, int n_ell, int64_t itr, double lr, double lr_z,
                           const double* Xv, const double* yv, int64_t nv, int64_t va_every,
                           const double* Xt, const double* yt, int64_t nt, int flags,
                           double* theta_out, double* z_out, double* values, double* thetas,
                           double* obj, double* mu, double* var, double* sc, double* va_sc,
                           double* va_z, int* info, int* steps_done) {
  const Va va = {Xv, yv, nv, va_every, va_sc, va_z};
  return train_call(ctx, kFitcTallVa, {0, objective, nprob, X, y, n, d, Z0, m, theta0, n_ell}, itr,
                    lr, lr_z, Xt, yt, nt, flags, theta_out, z_out, values, thetas, obj, mu, var, sc,
                    info, steps_done, &va);
}

int gps_fitc_blockloo_train_tall_va(gps_ctx* ctx, int objective, int nfold, int64_t nprob,
                                    const double* X, const double* y, int64_t n, int d,
                                    const double* Z0, int m, const double* theta0, int n_ell,
                                    int64_t itr, double lr, double lr_z, const double* Xv,
                                    const double* yv, int64_t nv, int64_t va_every,
                                    const double* Xt, const double* yt, int64_t nt, int flags,
                                    double* theta_out, double* z_out, double* values,
                                    double* thetas, double* obj, double* mu, double* var,
                                    double* sc, double* va_sc, double* va_z, int* info,
                                    int* steps_done) {
  const Va va = {Xv, yv, nv, va_every, va_sc, va_z};
  return train_call(ctx, kFitcTallBlockVa,
                    {0, objective, nprob, X, y, n, d, Z0, m, theta0, n_ell, nfold}, itr, lr, lr_z,
                    Xt, yt, nt, flags, theta_out, z_out, values, thetas, obj, mu, var, sc, info,
                    steps_done, &va);
}

}  // extern "C"
