// Diagnostics of the GEMM launcher (include/gpscore.h: gps_gemm_diag / gps_gemm_diag_check): one
// internal launch on host arrays, so the tests can drive every kernel variant alone and compare
// it exactly (tests/test_gpu_gemm_modes.py); and of the factorisation
// (gps_potrf_diag): gps_potrf's own path with every buffer it wrote copied back whole
// (tests/test_gpu_factor.py); and of the gradient layer (gps_grad_terms_diag,
// gps_grad_contract_diag, gps_fitc_contract_diag): one production launch_* call each on host
// arrays (tests/test_gpu_grad_terms.py); and of the vector layer (gps_vec_diag: the
// launchers of kernels_vec.hip, tests/test_gpu_vec.py).  Nothing here is on a
// production path.
#include "api_internal.h"

// (the binding's ctypes structure is checked against the same size: tests/test_gemm_diag_args.py)
static_assert(sizeof(gps_gemm_desc) == 128, "gps_gemm_desc layout");

namespace gpsapi {

// extents of the caller's arrays (doubles; kr in ints), 0 where the launch does not use one
struct DiagExtents {
  int64_t a, b, c, kscale, w, kr, out0, out1;
};

// The device-less validator: refuses (with a reason) every description whose launch could read
// or write outside the arrays the caller hands over, every combination launch_gemm rejects, and
// the dependent launch mode.  On success the arrays' extents.
static bool diag_check(const gps_gemm_desc& d, bool have_c, bool have_kscale, bool have_w,
                       const int32_t* kr, bool have_out0, bool have_out1, DiagExtents& x,
                       std::string& why) {
#define DIAG_REQ(cond, msg) \
  do {                      \
    if (!(cond)) {          \
      why = msg;            \
      return false;         \
    }                       \
  } while (0)
  DIAG_REQ(d.dep_mode == 0, "dep_mode: the dependent row-norm launch cannot run alone");
  DIAG_REQ((d.lay_a == LAY_N || d.lay_a == LAY_T) && (d.lay_b == LAY_N || d.lay_b == LAY_T),
           "layouts must be 0 or 1");
  DIAG_REQ(d.epi == EPI_STORE || d.epi == EPI_ROWSQ || d.epi == EPI_COLRED || d.epi == EPI_ROWSQ_DOT,
           "unknown epilogue");
  DIAG_REQ(d.M > 0 && d.N > 0 && d.K > 0 && d.M % GPS_TILE == 0 && d.N % GPS_TILE == 0 && d.K % 16 == 0,
           "M and N must be positive multiples of 128, K of 16");
  DIAG_REQ(d.M <= (1 << 18) && d.N <= (1 << 18) && (int64_t)d.M * d.N <= ((int64_t)1 << 27) &&
               d.K <= 65536,
           "M, N <= 2^18 with M*N <= 2^27, and K <= 65536");
  DIAG_REQ(d.lda > 0 && d.lda % 2 == 0 && d.lda >= (d.lay_a == LAY_N ? d.K : d.M) && d.lda <= (1 << 20),
           "lda must be even and at least A's stored row length");
  DIAG_REQ(d.ldb > 0 && d.ldb % 2 == 0 && d.ldb >= (d.lay_b == LAY_N ? d.N : d.K) && d.ldb <= (1 << 20),
           "ldb must be even and at least B's stored row length");
  DIAG_REQ(d.tri >= TRI_NONE && d.tri <= TRI_KR_J, "unknown tri mode");
  DIAG_REQ(d.tri_off >= 0 && d.tri_off % 16 == 0 && d.tri_off <= (1 << 24),
           "tri_off must be a non-negative multiple of 16");
  DIAG_REQ(d.tri_off == 0 || (d.tri >= TRI_K_LE_I && d.tri <= TRI_K_GE_I),
           "tri_off needs one of the four triangular k-range modes");
  if (d.tri == TRI_KR_J) {
    DIAG_REQ(kr != nullptr, "TRI_KR_J needs kr");
    for (int g = 0; g < 2 * (d.N / 16); ++g)
      DIAG_REQ(kr[g] >= 0 && kr[g] <= d.K && kr[g] % 16 == 0,
               "kr entries must be multiples of 16 in [0, K]");
  }
  DIAG_REQ(d.kend >= 0 && d.kend % 16 == 0, "kend must be 0 or a positive multiple of 16");
  // the live-extent hints: dead_m16 | dead_n16 << 8 trailing dead 16-blocks of M and N
  DIAG_REQ(d.reserved >= 0 && (d.reserved >> 16) == 0 && (d.reserved & 128) == 0 &&
               (d.reserved >> 8 & 128) == 0,
           "reserved must be dead_m16 | dead_n16 << 8 with both in 0..127");
  DIAG_REQ((d.reserved & 127) <= d.M / 16 && (d.reserved >> 8 & 127) <= d.N / 16,
           "reserved: more dead 16-blocks than M/16 or N/16");
  DIAG_REQ((d.lower_out == 0 || d.lower_out == 1) && (d.mirror == 0 || d.mirror == 1),
           "lower_out and mirror are flags");
  DIAG_REQ(!d.lower_out || d.M == d.N, "lower_out needs a square output");
  DIAG_REQ(!d.mirror || d.lower_out, "mirror needs lower_out");
  DIAG_REQ(d.tile == 0 || d.tile == 16 || d.tile == 32 || d.tile == 64 || d.tile == 128,
           "tile must be 0, 16, 32, 64 or 128");
  DIAG_REQ(d.ksplit >= 1 && d.ksplit <= 8, "ksplit must be in 1..8");
  DIAG_REQ(d.map_mode >= 0 && d.map_mode <= 6, "map_mode must be in 0..6");
  DIAG_REQ(d.map_mode != 3 || (!d.lower_out && d.tri >= TRI_K_LE_I && d.tri <= TRI_K_GE_I),
           "map_mode 3 needs a triangular operand and a full output");
  const bool small = d.tile == 16 || d.tile == 32;
  if (small) {
    DIAG_REQ(d.epi == EPI_STORE && !have_kscale, "the small kernel has no epilogue and no kscale");
    DIAG_REQ(d.ksplit == 1 || d.ksplit == 2 || d.ksplit == 4,
             "the small kernel runs 1, 2 or 4 waves per block");
  }
  DIAG_REQ(d.tile != 64 || d.epi == EPI_STORE, "the epilogues run on 128-tiles");
  x = DiagExtents{};
  x.a = (int64_t)(d.lay_a == LAY_N ? d.M : d.K) * d.lda;
  x.b = (int64_t)(d.lay_b == LAY_N ? d.K : d.N) * d.ldb;
  x.kscale = have_kscale ? d.K : 0;
  x.kr = d.tri == TRI_KR_J ? 2 * (d.N / 16) : 0;
  const bool split = !small && d.ksplit > 1;
  if (d.epi == EPI_STORE) {
    DIAG_REQ(have_c, "C is NULL");
    DIAG_REQ(d.ldc > 0 && d.ldc % 2 == 0 && d.ldc >= d.N && d.ldc <= (1 << 20),
             "ldc must be even and at least N");
    x.c = (int64_t)d.M * d.ldc;
    if (split && d.use_ws) {
      DIAG_REQ((int64_t)d.ksplit * d.M * d.N <= kSplitWsDoubles, "the slabs exceed the workspace");
    } else if (split) {
      // (gemm() gives every 64-tile split the stream's slabs, so the unslabbed form is 128-tile)
      DIAG_REQ(d.tile == 0 || d.tile == 128, "the unslabbed split runs on 128-tiles");
      DIAG_REQ(d.beta == 0.0 && !d.mirror, "the unslabbed split needs beta 0 and no mirror");
      DIAG_REQ(d.c_kslice_stride % 2 == 0 && d.c_kslice_stride >= x.c &&
                   d.c_kslice_stride <= ((int64_t)1 << 32),
               "c_kslice_stride must be even and at least M*ldc");
      x.c = (int64_t)d.ksplit * d.c_kslice_stride;
    }
  } else {
    DIAG_REQ(d.lay_a == LAY_N && d.lay_b == LAY_T, "the epilogues exist for A [i][k], B [j][k] only");
    DIAG_REQ(d.tile == 0 || d.tile == 128, "the epilogues run on 128-tiles");
    DIAG_REQ(d.ksplit == 1 && !d.mirror, "the epilogues take no split and no mirror");
    DIAG_REQ(have_out0 && d.ld_out > 0 && d.ld_out <= (1 << 20), "out0 / ld_out missing");
    if (d.epi == EPI_COLRED) {
      DIAG_REQ(have_w && have_out1, "EPI_COLRED needs w and out1");
      DIAG_REQ(d.ld_out >= d.N, "ld_out must be at least N");
      x.w = d.M;
      x.out0 = x.out1 = (int64_t)(d.M / GPS_TILE) * d.ld_out;
    } else {
      DIAG_REQ(d.ld_out >= d.M, "ld_out must be at least M");
      x.out0 = (int64_t)(d.N / GPS_TILE) * d.ld_out;
      if (d.epi == EPI_ROWSQ_DOT) {
        DIAG_REQ(have_w && have_out1, "EPI_ROWSQ_DOT needs w and out1");
        DIAG_REQ(d.tri == TRI_K_LE_J && d.K == d.tri_off + d.N,
                 "EPI_ROWSQ_DOT needs TRI_K_LE_J with K = tri_off + N");
        x.w = d.K;
        x.out1 = d.M;
      }
    }
  }
#undef DIAG_REQ
  return true;
}

// the description's scalar fields as GemmParams (the callers add the arrays)
static GemmParams desc_params(const gps_gemm_desc& d) {
  GemmParams p = gp0();
  p.lda = d.lda; p.ldb = d.ldb; p.ldc = d.ldc; p.c_kslice_stride = d.c_kslice_stride;
  p.M = d.M; p.N = d.N; p.K = d.K; p.alpha = d.alpha; p.beta = d.beta; p.ld_out = d.ld_out;
  p.lower_out = d.lower_out; p.ksplit = d.ksplit; p.tri = d.tri; p.tri_off = d.tri_off;
  p.map_mode = d.map_mode; p.tile = d.tile; p.mirror = d.mirror; p.kend = d.kend;
  p.sk_alone = d.sk_alone;
  // (all dead gives 0, the whole extent: nothing is skipped then)
  if (d.reserved & 127) p.m_live = d.M - 16 * (d.reserved & 127);
  if (d.reserved >> 8 & 127) p.n_live = d.N - 16 * (d.reserved >> 8 & 127);
  return p;
}
// a slabbed 128-tile split names its slabs itself (gemm() hands the stream's workspace only to
// unsplit launches and 64-tile splits)
static bool own_slabs(const gps_gemm_desc& d) {
  return d.ksplit > 1 && d.tile != 16 && d.tile != 32 && d.tile != 64 && d.use_ws;
}

}  // namespace gpsapi

extern "C" {

int gps_gemm_diag_check(const gps_gemm_desc* d, int have_c, int have_kscale, int have_w,
                        const int32_t* kr, int have_out0, int have_out1) {
  if (!d) return fail(nullptr, -1, "description is NULL");
  DiagExtents x;
  std::string why;
  if (!diag_check(*d, have_c != 0, have_kscale != 0, have_w != 0, kr, have_out0 != 0,
                  have_out1 != 0, x, why))
    return fail(nullptr, -1, "gps_gemm_diag: " + why);
  return 0;
}

int gps_gemm_diag(gps_ctx* ctx, const gps_gemm_desc* d, const double* A, const double* B,
                  double* C, const double* kscale, const double* w, const int32_t* kr,
                  double* out0, double* out1, int32_t* plan) {
  // the description is judged first, without a device; only a runnable one reaches bind()
  if (!d || !A || !B || !plan) return fail(ctx, -1, "gps_gemm_diag: NULL argument");
  DiagExtents x;
  std::string why;
  if (!diag_check(*d, C != nullptr, kscale != nullptr, w != nullptr, kr, out0 != nullptr,
                  out1 != nullptr, x, why))
    return fail(ctx, -1, "gps_gemm_diag: " + why);
  if (int rc = bind(ctx)) return rc;
  hipStream_t s = ctx->stream;
  auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };  // 16-byte aligned sub-buffers
  HIPCHK(ensure(ctx, ctx->t0, (size_t)(even(x.a) + even(x.b)) * 8));
  HIPCHK(ensure(ctx, ctx->t1, (size_t)std::max<int64_t>(even(x.c), 2) * 8));
  HIPCHK(ensure(ctx, ctx->t2, (size_t)(even(x.kscale) + even(x.w) + even(x.out0) + even(x.out1) +
                                       even((x.kr + 1) / 2) + 2) * 8));
  double* dA = ctx->t0.d();
  double* dB = dA + even(x.a);
  double* dC = ctx->t1.d();
  double* dks = ctx->t2.d();
  double* dw = dks + even(x.kscale);
  double* do0 = dw + even(x.w);
  double* do1 = do0 + even(x.out0);
  int* dkr = reinterpret_cast<int*>(do1 + even(x.out1));
  auto up = [&](void* dst, const void* src, int64_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  HIPCHK(up(dA, A, x.a * 8));
  HIPCHK(up(dB, B, x.b * 8));
  HIPCHK(up(dC, C, x.c * 8));
  HIPCHK(up(dks, kscale, x.kscale * 8));
  HIPCHK(up(dw, w, x.w * 8));
  HIPCHK(up(do0, out0, x.out0 * 8));
  HIPCHK(up(do1, out1, x.out1 * 8));
  HIPCHK(up(dkr, kr, x.kr * 4));
  GemmParams p = desc_params(*d);
  p.A = dA; p.B = dB; p.C = x.c ? dC : nullptr;
  p.kscale = x.kscale ? dks : nullptr;
  p.w = x.w ? dw : nullptr;
  p.out0 = x.out0 ? do0 : nullptr; p.out1 = x.out1 ? do1 : nullptr;
  p.kr = x.kr ? dkr : nullptr;
  if (own_slabs(*d)) {
    HIPCHK(ensure(ctx, ctx->ws_main, (size_t)kSplitWsDoubles * 8));
    p.ws = ctx->ws_main.d();
    p.ws_cap = kSplitWsDoubles;
  }
  GemmLaunchInfo info{};
  if (int rc = gemm(ctx, d->lay_a, d->lay_b, d->epi, p, nullptr, &info)) return rc;
  auto down = [&](void* dst, const void* src, int64_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
  };
  HIPCHK(down(C, dC, x.c * 8));
  HIPCHK(down(out0, do0, x.out0 * 8));
  HIPCHK(down(out1, do1, x.out1 * 8));
  HIPCHK(hipStreamSynchronize(s));
  const int v[GPS_N_GEMM_PLAN] = {info.tile, info.ksplit, info.map_mode, info.sk_dp,
                                  info.sk_wgs, info.slab_xcd, info.grid_x, info.grid_y};
  for (int i = 0; i < GPS_N_GEMM_PLAN; ++i) plan[i] = v[i];
  return 0;
}

int gps_potrf_diag(gps_ctx* ctx, int64_t n, const double* A, int64_t lda, double* L, double* Linv,
                   double* logdiag, int32_t* info, int32_t* plan) {
  // judged first, before anything touches the device
  if (!A || !L || !Linv || !logdiag || !info || !plan)
    return fail(ctx, -1, "gps_potrf_diag: NULL argument");
  if (n <= 0 || lda < n || n > (1 << 20)) return fail(ctx, -1, "gps_potrf_diag: bad shape");
  if (int rc = bind(ctx)) return rc;
  // gps_potrf's own path: the same buffers, options, capture and replay
  const int rc = factor_user(ctx, n, A, lda, true);
  if (rc < 0) return rc;
  *info = rc;  // 0, or the first non-PD minor (the launches completed; NaNs from that pivot on)
  const int64_t np = pad_to(n);
  hipStream_t s = ctx->stream;
  HIPCHK(hipMemcpyAsync(logdiag, ctx->t4.d(), (size_t)np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(L, ctx->t4.d() + np, (size_t)np * np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(Linv, ctx->t2.d(), (size_t)np * np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const gps_ctx::FactorPlan& fp = ctx->fplan;
  const int v[GPS_N_POTRF_PLAN] = {(int)np, fp.leaves, fp.dags, fp.dag_tmin, fp.dag_tmax, fp.gemms,
                                   fp.replayed, 0};
  for (int i = 0; i < GPS_N_POTRF_PLAN; ++i) plan[i] = v[i];
  return 0;
}

// ---- the gradient layer's launches on host arrays (tests/test_gpu_grad_terms.py).
// Each call judges its arguments, binds, carves device space from the compat scratch (t0: inputs,
// t1 / t2: matrices, gslab / gout: the contractions' slabs and outputs), fills what the kernel
// must write or must not read with NaN (bytes of 0xFF), calls the production launch_* and copies
// back.  No context member is added.
#define DIAG_REQ(cond, msg) \
  do {                      \
    if (!(cond)) return fail(ctx, -1, std::string(kWho) + msg); \
  } while (0)

int gps_grad_terms_diag(gps_ctx* ctx, int which, int obj, int64_t n, int64_t n_pad, int64_t m_pad,
                        double scal, const double* const* in, double* const* out) {
  static const char kWho[] = "gps_grad_terms_diag: ";
  DIAG_REQ(in && out, "NULL argument");
  DIAG_REQ(which >= 0 && which <= 3, "which must be 0..3");
  DIAG_REQ(n >= 1 && n <= (1 << 20), "n must be in 1..2^20");
  DIAG_REQ(std::isfinite(scal), "the scalar must be finite");
  // per call: inputs (count, each n long unless a matrix), outputs (count, each n_pad long)
  int n_in = 0, n_out = 0;
  int64_t in_len[8] = {0}, out_len[6] = {0};
  bool in_opt[8] = {false}, out_opt[6] = {false};
  if (which == 2) {
    DIAG_REQ(n_pad == n, "the fold terms have no padding: n_pad must equal n");
    n_in = 3; n_out = 3;
    out_len[0] = out_len[1] = n; out_len[2] = 1;
    out_opt[0] = out_opt[1] = true;
    DIAG_REQ(!out[0] || out[1], "gm without gc");
  } else {
    DIAG_REQ(n_pad >= n && n_pad <= (1 << 20), "n_pad must be in n..2^20");
    if (which == 0) {
      DIAG_REQ(obj == GPS_OBJ_LOO_CRPS || obj == GPS_OBJ_LOO_LOGS, "objective must be LOO-CRPS or LOO-LogS");
      n_in = 3; n_out = 2;
    } else if (which == 1) {
      DIAG_REQ(obj == GPS_OBJ_NLML || obj == GPS_OBJ_LOO_CRPS || obj == GPS_OBJ_LOO_LOGS,
               "objective must be NLML, LOO-CRPS or LOO-LogS");
      DIAG_REQ(scal > 0.0, "n_total must be positive");
      n_in = 4; n_out = 6;
    } else {
      DIAG_REQ(m_pad >= 2 && m_pad % 2 == 0 && m_pad <= 4096, "m_pad must be even, in 2..4096");
      DIAG_REQ(n * m_pad <= ((int64_t)1 << 24), "n*m_pad <= 2^24");
      n_in = 8; n_out = 4;
      in_opt[0] = in_opt[7] = true;
      DIAG_REQ(!in[0] || in[1], "KN without K");
      in_opt[1] = !in[0];
    }
    for (int q = 0; q < n_out; ++q) out_len[q] = n_pad;
  }
  for (int q = 0; q < n_in; ++q) {
    in_len[q] = which == 3 && q < 2 ? n * m_pad : n;
    DIAG_REQ(in[q] || in_opt[q], "NULL input array");
  }
  for (int q = 0; q < n_out; ++q) DIAG_REQ(out[q] || out_opt[q], "NULL output array");
  if (int rc = bind(ctx)) return rc;
  hipStream_t s = ctx->stream;
  auto even = [](int64_t v) { return (v + 1) & ~(int64_t)1; };
  int64_t tot_in = 2, tot_out = 2;
  for (int q = 0; q < n_in; ++q) tot_in += even(in_len[q]);
  for (int q = 0; q < n_out; ++q) tot_out += even(out_len[q]);
  HIPCHK(ensure(ctx, ctx->t0, (size_t)tot_in * 8));
  HIPCHK(ensure(ctx, ctx->t1, (size_t)tot_out * 8));
  HIPCHK(hipMemsetAsync(ctx->t1.d(), 0xFF, (size_t)tot_out * 8, s));
  const double* di[8] = {nullptr};
  double* dout[6] = {nullptr};
  double* w = ctx->t0.d();
  for (int q = 0; q < n_in; ++q) {
    if (in[q]) {
      HIPCHK(hipMemcpyAsync(w, in[q], (size_t)in_len[q] * 8, hipMemcpyHostToDevice, s));
      di[q] = w;
    }
    w += even(in_len[q]);
  }
  w = ctx->t1.d();
  for (int q = 0; q < n_out; ++q) {
    if (out[q]) dout[q] = w;
    w += even(out_len[q]);
  }
  const int ni = (int)n, np = (int)n_pad;
  switch (which) {
    case 0:
      HIPCHK(launch_loo_grad_terms(di[0], di[1], di[2], ni, np, obj, dout[0], dout[1], s));
      break;
    case 1:
      HIPCHK(launch_fitc_grad_terms(di[0], di[1], di[2], di[3], ni, np, obj, scal, dout[0], dout[1],
                                    dout[2], dout[3], dout[4], dout[5], s));
      break;
    case 2:
      HIPCHK(launch_fold_terms(di[0], di[1], di[2], ni, dout[0], dout[1], dout[2], s));
      break;
    default:
      HIPCHK(launch_fitc_grad_mdiag(di[0], m_pad, di[1], m_pad, (int)m_pad, di[2], di[3], di[4], di[5],
                                    di[6], di[7], scal, ni, np, dout[0], dout[1], dout[2], dout[3], s));
      break;
  }
  for (int q = 0; q < n_out; ++q)
    if (out[q])
      HIPCHK(hipMemcpyAsync(out[q], dout[q], (size_t)out_len[q] * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int gps_grad_contract_diag(gps_ctx* ctx, int64_t n, int d, const double* X, const double* inv_ell,
                           double sf2, const double* Ainv, const double* Mx, int64_t ld,
                           const double* alpha, const double* v, const double* a, double* out) {
  static const char kWho[] = "gps_grad_contract_diag: ";
  DIAG_REQ(X && inv_ell && alpha && a && out, "NULL argument");
  DIAG_REQ(d >= 1 && d <= GPS_MAX_D, "d must be in 1..64");
  DIAG_REQ(n >= 1 && n <= 8192, "n must be in 1..8192");
  DIAG_REQ(ld >= n && ld <= 16384, "ld must be in n..16384");
  DIAG_REQ(std::isfinite(sf2) && std::isfinite(a[0]) && std::isfinite(a[1]) &&
               std::isfinite(a[2]) && std::isfinite(a[3]),
           "sf2 and the coefficients must be finite");
  DIAG_REQ(Ainv || a[0] == 0.0, "a0 != 0 needs Ainv");
  DIAG_REQ(v || a[2] == 0.0, "a2 != 0 needs v");
  DIAG_REQ(Mx || a[3] == 0.0, "a3 != 0 needs Mx");
  if (int rc = bind(ctx)) return rc;
  hipStream_t s = ctx->stream;
  auto even = [](int64_t x) { return (x + 1) & ~(int64_t)1; };
  // every array reaches to the end of the last 64-row tile, NaN past its real rows; an absent
  // operand is a live buffer of NaN (the production call always passes a pointer)
  const int64_t nt64 = (n + 63) / 64 * 64;
  const int64_t nx = even(nt64 * d), nv = even(nt64), nm = nt64 * ld;
  const int passes = grad_contract_passes(d);
  const int64_t slab = grad_contract_slab_doubles((int)n, d);
  HIPCHK(ensure(ctx, ctx->t0, (size_t)(nx + 2 * nv) * 8));
  HIPCHK(ensure(ctx, ctx->t1, (size_t)nm * 8));
  HIPCHK(ensure(ctx, ctx->t2, (size_t)nm * 8));
  HIPCHK(ensure(ctx, ctx->gslab, (size_t)slab * 8));
  HIPCHK(ensure(ctx, ctx->gout, (size_t)passes * 18 * 8));
  double* dX = ctx->t0.d();
  double* dal = dX + nx;
  double* dv = dal + nv;
  HIPCHK(hipMemsetAsync(ctx->t0.d(), 0xFF, (size_t)(nx + 2 * nv) * 8, s));
  HIPCHK(hipMemsetAsync(ctx->t1.d(), 0xFF, (size_t)nm * 8, s));
  HIPCHK(hipMemsetAsync(ctx->t2.d(), 0xFF, (size_t)nm * 8, s));
  auto put = [&](double* dst, const double* src, int64_t cnt) {
    return src ? hipMemcpyAsync(dst, src, (size_t)cnt * 8, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  HIPCHK(put(dX, X, n * d));
  HIPCHK(put(dal, alpha, n));
  HIPCHK(put(dv, v, n));
  HIPCHK(put(ctx->t1.d(), Ainv, n * ld));
  HIPCHK(put(ctx->t2.d(), Mx, n * ld));
  HIPCHK(hipMemsetAsync(ctx->gslab.d(), 0xFF, (size_t)slab * 8, s));
  HIPCHK(hipMemsetAsync(ctx->gout.d(), 0xFF, (size_t)passes * 18 * 8, s));
  GradParams g{};
  g.x = dX; g.n = (int)n; g.d = d; g.sf2 = sf2;
  for (int k = 0; k < d; ++k) g.inv_ell[k] = inv_ell[k];
  g.Ainv = ctx->t1.d(); g.Mx = ctx->t2.d(); g.ldm = ld;
  g.alpha = dal; g.v = dv;
  g.a0 = a[0]; g.a1 = a[1]; g.a2 = a[2]; g.a3 = a[3];
  g.slab = ctx->gslab.d();
  HIPCHK(launch_grad_contract(g, ctx->gout.d(), s));
  HIPCHK(hipMemcpyAsync(out, ctx->gout.d(), (size_t)passes * 18 * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int gps_fitc_contract_diag(gps_ctx* ctx, int64_t nr, int64_t nc, int64_t nc_pad, int d,
                           const double* xr, const double* xc, const double* inv_ell, double sf2,
                           int nt, const double* const* R, const int64_t* ldr, const double* coef,
                           const double* const* rs, const double* pc, const double* const* pv,
                           const double* const* qv, double* out, double* zout) {
  static const char kWho[] = "gps_fitc_contract_diag: ";
  DIAG_REQ(xr && xc && inv_ell && pc && out && zout, "NULL argument");
  DIAG_REQ(d >= 1 && d <= GPS_MAX_D, "d must be in 1..64");
  DIAG_REQ(nr >= 1 && nr <= (1 << 20), "nr must be in 1..2^20");
  DIAG_REQ(nc >= 1 && nc <= 16384, "nc must be in 1..16384");
  DIAG_REQ(nc_pad >= nc && nc_pad <= nc + 128, "nc_pad must be in nc..nc+128");
  DIAG_REQ(nt >= 0 && nt <= 4, "nt must be in 0..4");
  DIAG_REQ(nt == 0 || (R && ldr && coef), "matrix terms need R, ldr and coef");
  DIAG_REQ(std::isfinite(sf2) && std::isfinite(pc[0]) && std::isfinite(pc[1]),
           "sf2 and the coefficients must be finite");
  int64_t rtot = 0;
  for (int t = 0; t < nt; ++t) {
    DIAG_REQ(R[t], "NULL matrix term");
    DIAG_REQ(ldr[t] >= nc && ldr[t] <= 32768, "ldr must be in nc..32768");
    DIAG_REQ(std::isfinite(coef[t]), "sf2 and the coefficients must be finite");
    rtot += (nr + 16) * ldr[t];
  }
  DIAG_REQ(rtot <= ((int64_t)1 << 26), "the matrix terms exceed 2^26 doubles");
  for (int q = 0; q < 2; ++q)
    DIAG_REQ(pc[q] == 0.0 || (pv && qv && pv[q] && qv[q]), "a rank-one term needs pv and qv");
  if (int rc = bind(ctx)) return rc;
  hipStream_t s = ctx->stream;
  // every array gets a tail past its real extent (16 rows: one batch of the row loop; 64 columns:
  // one column block), and everything not uploaded is NaN
  const int64_t nrt = nr + 16, nct = nc_pad + 64;
  const int64_t vec = nrt * d + nct * d + 6 * nrt + 2 * nct;
  const int passes = fitc_contract_passes(d);
  const int64_t slab = fitc_contract_slab_doubles((int)nr, (int)nc_pad, d);
  const int64_t nout = passes * 17 + nc * d;
  HIPCHK(ensure(ctx, ctx->t0, (size_t)vec * 8));
  HIPCHK(ensure(ctx, ctx->t1, (size_t)std::max<int64_t>(rtot, 2) * 8));
  HIPCHK(ensure(ctx, ctx->gslab, (size_t)slab * 8));
  HIPCHK(ensure(ctx, ctx->gout, (size_t)nout * 8));
  HIPCHK(hipMemsetAsync(ctx->t0.d(), 0xFF, (size_t)vec * 8, s));
  HIPCHK(hipMemsetAsync(ctx->t1.d(), 0xFF, (size_t)std::max<int64_t>(rtot, 2) * 8, s));
  HIPCHK(hipMemsetAsync(ctx->gslab.d(), 0xFF, (size_t)slab * 8, s));
  HIPCHK(hipMemsetAsync(ctx->gout.d(), 0xFF, (size_t)nout * 8, s));
  auto up = [&](double* dst, const double* src, int64_t cnt) {
    return hipMemcpyAsync(dst, src, (size_t)cnt * 8, hipMemcpyHostToDevice, s);
  };
  FitcContractParams p{};
  double* w = ctx->t0.d();
  HIPCHK(up(w, xr, nr * d)); p.xr = w; w += nrt * d;
  HIPCHK(up(w, xc, nc * d)); p.xc = w; w += nct * d;
  p.nr = (int)nr; p.nc = (int)nc; p.nc_pad = (int)nc_pad; p.d = d; p.sf2 = sf2;
  for (int k = 0; k < d; ++k) p.inv_ell[k] = inv_ell[k];
  p.nt = nt;
  double* m = ctx->t1.d();
  for (int t = 0; t < 4; ++t) {
    if (t < nt) {
      HIPCHK(up(m, R[t], nr * ldr[t]));
      p.R[t] = m; p.ldr[t] = ldr[t]; p.coef[t] = coef[t];
      m += nrt * ldr[t];
      if (rs && rs[t]) {
        HIPCHK(up(w, rs[t], nr));
        p.rs[t] = w;
      }
    }
    w += nrt;
  }
  for (int q = 0; q < 2; ++q) {
    p.pc[q] = pc[q];
    // a rank-one term that is off still gets live (NaN) vectors, as the production call has
    p.pv[q] = w;
    if (pc[q] != 0.0) HIPCHK(up(w, pv[q], nr));
    w += nrt;
    p.qv[q] = w;
    if (pc[q] != 0.0) HIPCHK(up(w, qv[q], nc));
    w += nct;
  }
  p.slab = ctx->gslab.d();
  HIPCHK(launch_fitc_grad_contract(p, ctx->gout.d(), ctx->gout.d() + passes * 17, s));
  HIPCHK(hipMemcpyAsync(out, ctx->gout.d(), (size_t)passes * 17 * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(zout, ctx->gout.d() + passes * 17, (size_t)nc * d * 8,
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

// ---- the vector layer's launches on host arrays (kernels_vec.hip; tests/test_gpu_vec.py,
// DESIGN §30).  One call: judge, bind, carve device space from the compat scratch (t0: inputs,
// t1: outputs, slabs and partials — both NaN throughout before anything is uploaded, with a NaN
// gap after every array), upload, poison the strict-upper 128-tiles of the lower modes, call the
// production launch_*, copy back.  No context member is added.
int gps_vec_diag(gps_ctx* ctx, int which, const int64_t* dims, const double* scal,
                 const double* const* in, double* const* out) {
  static const char kWho[] = "gps_vec_diag: ";
  DIAG_REQ(dims && scal && in && out, "NULL argument");
  DIAG_REQ(which >= 0 && which <= 13, "which must be 0..13");
  constexpr int64_t kCap = (int64_t)1 << 26;  // doubles per scratch buffer
  constexpr int64_t kGap = 16;                // NaN doubles after every array
  auto even = [](int64_t v) { return (v + 1) & ~(int64_t)1; };
  auto tile = [](int64_t v) { return v >= GPS_TILE && v % GPS_TILE == 0; };
  const int64_t d0 = dims[0], d1 = dims[1], d2 = dims[2], d3 = dims[3], d4 = dims[4], d5 = dims[5],
                d6 = dims[6], d7 = dims[7];
  int64_t need0 = 0, need1 = 0;  // doubles of t0 / t1, gaps not counted (added per array below)
  int n_in = 0, n_out = 0;       // pointer slots looked at
  bool in_opt[8] = {false}, out_opt[8] = {false};
  switch (which) {
    case 0: {  // {mode 0 full / 1 lower / 2 trmv_lower, rows, cols, ldm, trans}; {M, x}; {y}
      DIAG_REQ(d0 >= 0 && d0 <= 2, "gemv: mode must be 0 (full), 1 (lower) or 2 (trmv_lower)");
      DIAG_REQ(d1 >= 1 && d1 <= 16384 && d2 >= 1 && d2 <= 16384, "gemv: rows and cols must be in 1..16384");
      DIAG_REQ(!(d2 & 1), "gemv: cols must be even");
      DIAG_REQ(!(d3 & 1) && d3 >= d2 && d3 <= 32768, "gemv: ldm must be even, in cols..32768");
      DIAG_REQ(d0 == 0 || (d1 == d2 && tile(d1)), "gemv: the lower form is square, a multiple of 128");
      DIAG_REQ(d0 != 2 || d4 == 0, "launch_trmv_lower has no transposed form (launch_colred is)");
      n_in = 2; n_out = 1;
      need0 = d1 * d3 + d2; need1 = d1;
      break;
    }
    case 1:    // {rows, cols, ldm, lower, crows}; {M, w or NULL, rowscale or NULL}; {s1, s2} (either)
    case 2: {  // {rows, cols, ldm, lower}; {M, w}; {slab [2·nchunk·cols], count[1]}
      const char* k = which == 1 ? "colred: " : "colred_partials: ";
      const int64_t crows = which == 1 ? d4 : 256;
      DIAG_REQ(d0 >= 1 && d0 <= 16384 && d1 >= 1 && d1 <= 16384, std::string(k) + "rows and cols must be in 1..16384");
      DIAG_REQ(!(d1 & 1), std::string(k) + "cols must be even");
      DIAG_REQ(!(d2 & 1), std::string(k) + "ldm must be even");
      DIAG_REQ(d2 >= d1 && d2 <= 32768, std::string(k) + "ldm must be in cols..32768");
      DIAG_REQ(crows >= 1, std::string(k) + "crows must be at least 1");
      DIAG_REQ(d3 == 0 || d3 == 1, std::string(k) + "lower is a flag");
      DIAG_REQ(!d3 || (d0 == d1 && tile(d0)), std::string(k) + "the lower form is square, a multiple of 128");
      const int64_t nchunk = (d0 + crows - 1) / crows;
      DIAG_REQ(2 * nchunk * d1 <= kCap / 2, std::string(k) + "the chunk slabs exceed 2^25 doubles");
      if (which == 1) {
        n_in = 3; n_out = 2;
        in_opt[1] = in_opt[2] = out_opt[0] = out_opt[1] = true;
        DIAG_REQ(out[0] || out[1], "colred: neither s1 nor s2");
        DIAG_REQ(!out[0] || in[1], "colred: s1 needs w");
      } else {
        n_in = 2; n_out = 2;
      }
      need0 = d0 * d2 + 2 * d0; need1 = 2 * nchunk * d1 + 2 * d1 + 2;
      break;
    }
    case 3: {  // {nslab, len, ld}; {slab [nslab][len], init or NULL}; {out [len]}
      DIAG_REQ(d0 >= 1 && d0 <= 4096, "slab_sum: nslab must be in 1..4096");
      DIAG_REQ(d1 >= 1 && d1 <= (1 << 20), "slab_sum: len must be in 1..2^20");
      DIAG_REQ(d2 >= d1 && d2 <= (1 << 21), "slab_sum: ld must be in len..2^21");
      DIAG_REQ((d0 + 1) * d2 <= kCap / 2, "slab_sum: the slabs exceed 2^25 doubles");
      n_in = 2; n_out = 1; in_opt[1] = true;
      need0 = (d0 + 1) * d2 + d1; need1 = d1;
      break;
    }
    case 4:    // {nslab, M, stride}; {slab [nslab][M·M], base or NULL}; {dst [M·M]}
    case 5: {  // {nslab, M, stride, m, r0, r1, unpack, full}; same in; {packed (in/out), dst}
      const char* k = which == 4 ? "sym_slab_sum: " : "sym_pack: ";
      DIAG_REQ(d0 >= 1 && d0 <= 64, std::string(k) + "nslab must be in 1..64");
      DIAG_REQ(tile(d1) && d1 <= 4096, std::string(k) + "M must be a multiple of 128, at most 4096");
      DIAG_REQ(d2 >= d1 * d1 && d2 <= kCap, std::string(k) + "stride must be at least M*M");
      DIAG_REQ((d0 + 1) * d2 <= kCap / 2, std::string(k) + "the slabs exceed 2^25 doubles");
      n_in = 2; in_opt[1] = true;
      need0 = (d0 + 1) * d2 + d1 * d1;
      if (which == 4) {
        n_out = 1;
        need1 = d1 * d1;
      } else {
        DIAG_REQ(d3 >= 1 && d3 <= d1, "sym_pack: m must be in 1..M");
        DIAG_REQ(d4 >= 0 && d4 <= d5 && d5 <= d3, "sym_pack: the rows must satisfy 0 <= r0 <= r1 <= m");
        DIAG_REQ((d6 == 0 || d6 == 1) && (d7 == 0 || d7 == 1), "sym_pack: unpack and full are flags");
        n_out = 2; out_opt[1] = !d6;
        need1 = d3 * (d3 + 1) / 2 + d1 * d1;
      }
      break;
    }
    case 6: {  // {n, nslab, ld}; {y [n], slab1, slab2 [nslab][n_pad], beta, logdiag [n_pad]};
               // {alpha, dinv, mu_loo, var_loo [n_pad], obj [5], sums [4]}
      DIAG_REQ(d0 >= 1 && d0 <= (1 << 20), "full_loo: n must be in 1..2^20");
      DIAG_REQ(d1 >= 1 && d1 <= 64, "full_loo: nslab must be in 1..64");
      DIAG_REQ(d2 >= gps::pad_to(d0) && d2 <= (1 << 21), "full_loo: ld must be in n_pad..2^21");
      DIAG_REQ((2 * d1 + 1) * d2 <= kCap / 2, "full_loo: the slabs exceed 2^25 doubles");
      n_in = 5; n_out = 6;
      need0 = (2 * d1 + 1) * d2 + 3 * gps::pad_to(d0);
      need1 = 4 * gps::pad_to(d0) + 16 + 4 * (gps::pad_to(d0) / 256 + 1);
      break;
    }
    case 7:    // {n, n_pad, nslab, ld}; scal {sf2, sn2}; {slab [nslab][n_pad], y [n]};
               // {q, lam, inv_lam, ys [n_pad], sums [2]}
    case 8: {  // {n, n_pad, nslab, ld}; {y, lam [n], slab [nslab][n_pad], g [n]};
               // {r, mu_loo, var_loo [n_pad], sums [2]}
      const char* k = which == 7 ? "fitc_lambda: " : "fitc_loo: ";
      DIAG_REQ(d0 >= 1 && d0 <= (1 << 20), std::string(k) + "n must be in 1..2^20");
      DIAG_REQ(d1 >= d0 && d1 <= (1 << 20), std::string(k) + "n_pad must be in n..2^20");
      DIAG_REQ(d2 >= 1 && d2 <= 64, std::string(k) + "nslab must be in 1..64");
      DIAG_REQ(d3 >= d1 && d3 <= (1 << 21), std::string(k) + "ld must be in n_pad..2^21");
      DIAG_REQ((d2 + 1) * d3 <= kCap / 2, std::string(k) + "the slabs exceed 2^25 doubles");
      if (which == 7) DIAG_REQ(std::isfinite(scal[0]) && std::isfinite(scal[1]), "fitc_lambda: sf2 and sn2 must be finite");
      n_in = which == 7 ? 2 : 4; n_out = which == 7 ? 5 : 4;
      need0 = (d2 + 1) * d3 + 3 * d1;
      need1 = 4 * d1 + 2 + 2 * (d1 / 256 + 1);
      break;
    }
    case 9: {  // {nt, fitc}; scal {base_var}; {s1 | qm, s2 | qb [nt]}; {mu (full GP only), var [nt]}
      DIAG_REQ(d0 >= 1 && d0 <= (1 << 20), "pred_finalize: nt must be in 1..2^20");
      DIAG_REQ(d1 == 0 || d1 == 1, "pred_finalize: fitc is a flag");
      DIAG_REQ(std::isfinite(scal[0]), "pred_finalize: base_var must be finite");
      n_in = 2; n_out = 2; out_opt[0] = d1 != 0;
      need0 = 2 * d0; need1 = 2 * d0;
      break;
    }
    case 10: {  // {n, add_noise}; scal {s2}; {y, alpha, dinv [n]}; {sums [2]}
      DIAG_REQ(d0 >= 1 && d0 <= (1 << 20), "surface_point: n must be in 1..2^20");
      DIAG_REQ(d1 == 0 || d1 == 1, "surface_point: add_noise is a flag");
      DIAG_REQ(std::isfinite(scal[0]), "surface_point: s2 must be finite");
      n_in = 3; n_out = 1;
      need0 = 3 * d0; need1 = 2 + 2 * (d0 / 256 + 1);
      break;
    }
    case 11: {  // {n}; {a, b or NULL [n]}; {out [1]}
      DIAG_REQ(d0 >= 1 && d0 <= (1 << 20), "dot: n must be in 1..2^20");
      n_in = 2; n_out = 1; in_opt[1] = true;
      need0 = 2 * d0; need1 = 1;
      break;
    }
    case 12: {  // {rows, cols, lds, rows_pad, cols_pad, ldd, pad_identity}; {src [rows][cols]};
                // {dst [rows_pad][ldd]}; on the device src has row stride lds, NaN between the rows
      DIAG_REQ(d0 >= 1 && d1 >= 1 && d3 >= d0 && d4 >= d1 && d3 <= 8192 && d4 <= 8192,
               "pad_copy: 1 <= rows <= rows_pad <= 8192 and 1 <= cols <= cols_pad <= 8192");
      DIAG_REQ(d2 >= d1 && d2 <= 16384, "pad_copy: lds must be in cols..16384");
      DIAG_REQ(d5 >= d4 && d5 <= 16384, "pad_copy: ldd must be in cols_pad..16384");
      DIAG_REQ(d6 == 0 || d6 == 1, "pad_copy: pad_identity is a flag");
      n_in = 1; n_out = 1;
      need0 = d0 * d2; need1 = d3 * d5;
      DIAG_REQ(need0 <= kCap / 2 && need1 <= kCap / 2, "pad_copy: the matrices exceed 2^25 doubles");
      break;
    }
    default: {  // 13: {n, count}; {src [n][count]}; {out [count]}
      DIAG_REQ(d0 >= 1 && d0 <= gps::kLocalSumMax, "local_sum: n must be in 1..64");
      DIAG_REQ(d1 >= 1 && d1 <= (1 << 18), "local_sum: count must be in 1..2^18");
      n_in = 1; n_out = 1;
      need0 = d0 * d1; need1 = d1;
      break;
    }
  }
  for (int q = 0; q < n_in; ++q) DIAG_REQ(in[q] || in_opt[q], "NULL input array");
  for (int q = 0; q < n_out; ++q) DIAG_REQ(out[q] || out_opt[q], "NULL output array");
  if (int rc = bind(ctx)) return rc;
  hipStream_t s = ctx->stream;
  const int64_t cap0 = need0 + 80 * kGap + 256, cap1 = need1 + 80 * kGap + 256;
  HIPCHK(ensure(ctx, ctx->t0, (size_t)cap0 * 8));
  HIPCHK(ensure(ctx, ctx->t1, (size_t)cap1 * 8));
  HIPCHK(hipMemsetAsync(ctx->t0.d(), 0xFF, (size_t)cap0 * 8, s));
  HIPCHK(hipMemsetAsync(ctx->t1.d(), 0xFF, (size_t)cap1 * 8, s));
  int64_t used0 = 0, used1 = 0;
  bool over = false;
  auto take = [&](int buf, int64_t cnt) -> double* {
    int64_t& used = buf ? used1 : used0;
    double* p = (buf ? ctx->t1.d() : ctx->t0.d()) + used;
    used += even(cnt) + kGap;
    if (used > (buf ? cap1 : cap0)) over = true;
    return p;
  };
#define VD_FITS() \
  if (over) return fail(ctx, -2, std::string(kWho) + "internal: the scratch carving overran")
  auto up = [&](double* dst, const double* src, int64_t cnt) {
    return hipMemcpyAsync(dst, src, (size_t)cnt * 8, hipMemcpyHostToDevice, s);
  };
  auto up2d = [&](double* dst, int64_t ldd, const double* src, int64_t rows, int64_t cols) {
    return hipMemcpy2DAsync(dst, (size_t)ldd * 8, src, (size_t)cols * 8, (size_t)cols * 8,
                            (size_t)rows, hipMemcpyHostToDevice, s);
  };
  auto down = [&](double* dst, const double* src, int64_t cnt) {
    return hipMemcpyAsync(dst, src, (size_t)cnt * 8, hipMemcpyDeviceToHost, s);
  };
  // NaN over the strict-upper 128-tiles of a square np × np matrix
  auto poison_upper = [&](double* p, int64_t ld, int64_t np) {
    for (int64_t t = 0; (t + 1) * GPS_TILE < np; ++t) {
      hipError_t e = hipMemset2DAsync(p + t * GPS_TILE * ld + (t + 1) * GPS_TILE, (size_t)ld * 8, 0xFF,
                                      (size_t)(np - (t + 1) * GPS_TILE) * 8, GPS_TILE, s);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  switch (which) {
    case 0: {
      double* M = take(0, d1 * d3);
      double* x = take(0, d2);
      double* y = take(1, d1);
      VD_FITS();
      HIPCHK(up2d(M, d3, in[0], d1, d2));
      if (d0) HIPCHK(poison_upper(M, d3, d1));
      HIPCHK(up(x, in[1], d2));
      if (d0 == 0) HIPCHK(launch_gemv_full(M, d3, x, y, (int)d1, (int)d2, s));
      else if (d0 == 1) HIPCHK(launch_gemv_lower(M, d3, x, y, (int)d1, s));
      else HIPCHK(launch_trmv_lower(M, d3, x, y, (int)d1, (int)d4, s));
      HIPCHK(down(out[0], y, d1));
      break;
    }
    case 1:
    case 2: {
      const int64_t crows = which == 1 ? d4 : 256, nchunk = (d0 + crows - 1) / crows;
      double* M = take(0, d0 * d2);
      double* w = in[1] ? take(0, d0) : nullptr;
      double* rs = which == 1 && in[2] ? take(0, d0) : nullptr;
      double* slab = take(1, 2 * nchunk * d1);
      double* s1 = take(1, d1);
      double* s2 = take(1, d1);
      VD_FITS();
      HIPCHK(up2d(M, d2, in[0], d0, d1));
      if (d3) HIPCHK(poison_upper(M, d2, d0));
      if (w) HIPCHK(up(w, in[1], d0));
      if (rs) HIPCHK(up(rs, in[2], d0));
      if (which == 1) {
        HIPCHK(launch_colred(M, d2, (int)d0, (int)d1, (int)d3, w, rs, out[0] ? s1 : nullptr,
                             out[1] ? s2 : nullptr, slab, s, (int)crows));
        if (out[0]) HIPCHK(down(out[0], s1, d1));
        if (out[1]) HIPCHK(down(out[1], s2, d1));
      } else {
        const int got = launch_colred_partials(M, d2, (int)d0, (int)d1, (int)d3, w, slab, s);
        if (got < 0) return fail(ctx, -2, std::string(kWho) + "launch_colred_partials failed");
        HIPCHK(down(out[0], slab, 2 * nchunk * d1));
        out[1][0] = (double)got;
      }
      break;
    }
    case 3: {
      double* slab = take(0, (d0 + 1) * d2);
      double* init = in[1] ? take(0, d1) : nullptr;
      double* o = take(1, d1);
      VD_FITS();
      HIPCHK(up2d(slab, d2, in[0], d0, d1));
      if (init) HIPCHK(up(init, in[1], d1));
      HIPCHK(launch_slab_sum(slab, d2, (int)d0, d1, init, o, s));
      HIPCHK(down(out[0], o, d1));
      break;
    }
    case 4:
    case 5: {
      const int64_t mm = d1 * d1, plen = which == 5 ? d3 * (d3 + 1) / 2 : 0;
      const bool unpack = which == 5 && d6;
      double* slab = take(0, (d0 + 1) * d2);
      double* base = in[1] ? take(0, mm) : nullptr;
      double* packed = which == 5 ? take(1, plen) : nullptr;
      double* dst = take(1, mm);
      VD_FITS();
      for (int64_t q = 0; q < d0; ++q) {
        HIPCHK(up(slab + q * d2, in[0] + q * mm, mm));
        HIPCHK(poison_upper(slab + q * d2, d1, d1));
      }
      if (base) {
        HIPCHK(up(base, in[1], mm));
        if (which == 4 || !d7) HIPCHK(poison_upper(base, d1, d1));
      }
      if (which == 4) {
        HIPCHK(launch_sym_slab_sum(slab, d2, (int)d0, (int)d1, base, dst, s));
      } else {
        HIPCHK(up(packed, out[0], plen));
        HIPCHK(launch_sym_pack(slab, d2, (int)d0, (int)d4, (int)d5, (int)d1, packed, s));
        if (unpack) HIPCHK(launch_sym_unpack(packed, (int)d3, (int)d1, base, (int)d7, dst, s));
        HIPCHK(down(out[0], packed, plen));
      }
      if (which == 4 || unpack) HIPCHK(down(out[which == 4 ? 0 : 1], dst, mm));
      break;
    }
    case 6: {
      const int64_t np = gps::pad_to(d0), nblk = np / 256 + (np % 256 ? 1 : 0);
      double* y = take(0, np);
      double* slab = take(0, (2 * d1 + 1) * d2);
      double* beta = take(0, np);
      double* logdiag = take(0, np);
      double* o[4];
      for (auto& p : o) p = take(1, np);
      double* obj = take(1, 16);
      double* part = take(1, nblk * 4);
      VD_FITS();
      HIPCHK(up(y, in[0], d0));
      HIPCHK(up2d(slab, d2, in[1], d1, np));
      HIPCHK(up2d(slab + d1 * d2, d2, in[2], d1, np));
      HIPCHK(up(beta, in[3], np));
      HIPCHK(up(logdiag, in[4], np));
      HIPCHK(launch_full_loo(y, slab, (int)d1, d2, beta, logdiag, (int)d0, o[0], o[1], o[2], o[3], obj,
                             part, s));
      for (int q = 0; q < 4; ++q) HIPCHK(down(out[q], o[q], np));
      HIPCHK(down(out[4], obj, 5));
      HIPCHK(down(out[5], obj + 8, 4));
      break;
    }
    case 7:
    case 8: {
      const int64_t nblk = std::max<int64_t>(1, (d1 + 255) / 256);
      const int nv = which == 7 ? 4 : 3;
      double* slab = take(0, (d2 + 1) * d3);
      double* v[3];
      for (auto& p : v) p = take(0, d1);
      double* o[4];
      for (auto& p : o) p = take(1, d1);
      double* sums = take(1, 2);
      double* part = take(1, nblk * 2);
      VD_FITS();
      HIPCHK(up2d(slab, d3, in[which == 7 ? 0 : 2], d2, d1));
      if (which == 7) {
        HIPCHK(up(v[0], in[1], d0));
        HIPCHK(launch_fitc_lambda(slab, d3, (int)d2, v[0], (int)d0, (int)d1, scal[0], scal[1], o[0], o[1],
                                  o[2], o[3], sums, part, s));
      } else {
        HIPCHK(up(v[0], in[0], d0));
        HIPCHK(up(v[1], in[1], d0));
        HIPCHK(up(v[2], in[3], d0));
        HIPCHK(launch_fitc_loo(v[0], v[1], slab, d3, (int)d2, v[2], (int)d0, (int)d1, o[0], o[1], o[2],
                               sums, part, s));
      }
      for (int q = 0; q < nv; ++q) HIPCHK(down(out[q], o[q], d1));
      HIPCHK(down(out[nv], sums, 2));
      break;
    }
    case 9: {
      double* a = take(0, d0);
      double* b = take(0, d0);
      double* mu = take(1, d0);
      double* var = take(1, d0);
      VD_FITS();
      HIPCHK(up(a, in[0], d0));
      HIPCHK(up(b, in[1], d0));
      if (d1) HIPCHK(launch_fitc_pred_finalize(a, b, (int)d0, scal[0], var, s));
      else HIPCHK(launch_pred_finalize(a, b, (int)d0, scal[0], mu, var, s));
      if (!d1) HIPCHK(down(out[0], mu, d0));
      HIPCHK(down(out[1], var, d0));
      break;
    }
    case 10: {
      const int64_t nblk = std::max<int64_t>(1, (d0 + 255) / 256);
      double* v[3];
      for (auto& p : v) p = take(0, d0);
      double* sums = take(1, 2);
      double* part = take(1, nblk * 2);
      VD_FITS();
      for (int q = 0; q < 3; ++q) HIPCHK(up(v[q], in[q], d0));
      HIPCHK(launch_surface_point_sums(v[0], v[1], v[2], (int)d0, scal[0], (int)d1, sums, part, s));
      HIPCHK(down(out[0], sums, 2));
      break;
    }
    case 11: {
      double* a = take(0, d0);
      double* b = in[1] ? take(0, d0) : nullptr;
      double* o = take(1, 1);
      VD_FITS();
      HIPCHK(up(a, in[0], d0));
      if (b) HIPCHK(up(b, in[1], d0));
      HIPCHK(launch_dot(a, b, (int)d0, o, s));
      HIPCHK(down(out[0], o, 1));
      break;
    }
    case 12: {
      double* src = take(0, d0 * d2);
      double* dst = take(1, d3 * d5);
      VD_FITS();
      HIPCHK(up2d(src, d2, in[0], d0, d1));
      HIPCHK(launch_pad_copy(src, d2, dst, d5, (int)d0, (int)d1, (int)d3, (int)d4, (int)d6, s));
      HIPCHK(down(out[0], dst, d3 * d5));
      break;
    }
    default: {
      LocalSumPtrs sp{};
      for (int64_t q = 0; q < d0; ++q) sp.p[q] = take(0, d1);
      double* o = take(1, d1);
      VD_FITS();
      for (int64_t q = 0; q < d0; ++q) HIPCHK(up(const_cast<double*>(sp.p[q]), in[0] + q * d1, d1));
      HIPCHK(launch_local_sum(sp, (int)d0, d1, o, s));
      HIPCHK(down(out[0], o, d1));
      break;
    }
  }
#undef VD_FITS
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

// ---- the block-LOO, energy-score and joint kernels' launches on host arrays (kernels_block.hip,
// kernels_joint.hip, fitc_grad_v / fitc_grad_y of kernels_fitc_grad.hip; tests/test_gpu_block.py,
// DESIGN §39).  As gps_vec_diag: judge, bind, carve t0 (inputs) and t1 (outputs and in/out arrays),
// both NaN throughout beforehand with a 16-double NaN gap after every array, upload, call the
// production launch_*, copy back.  An input is dense [rows][cols] on the host and has its row
// stride on the device; an output comes back as its device image, [rows][ld] and the gap after it,
// so the caller sees what the kernel left alone.  No context member is added.
int gps_block_diag(gps_ctx* ctx, int which, const int64_t* dims, const double* scal,
                   const double* const* in, double* const* out) {
  static const char kWho[] = "gps_block_diag: ";
  DIAG_REQ(dims && scal && in && out, "NULL argument");
  DIAG_REQ(which >= 0 && which <= 23, "which must be 0..23");
  constexpr int64_t kGap = 16, kMax = 4096, kLen = (int64_t)1 << 20;
  const int64_t d0 = dims[0], d1 = dims[1], d2 = dims[2], d3 = dims[3], d4 = dims[4], d5 = dims[5],
                d6 = dims[6], d7 = dims[7];
  for (int q = 0; q < 8; ++q) DIAG_REQ(std::isfinite(scal[q]), "the scalars must be finite");
  struct Arr {
    int64_t rows, cols, ld;
    bool opt, io;        // may be NULL; (outputs) uploaded first, the kernel reads it
    int64_t extra;       // doubles carved past rows·ld and left NaN
    double* d;
  };
  Arr ai[12] = {}, ao[4] = {};
  int n_in = 0, n_out = 0;
  auto I = [&](int64_t rows, int64_t cols, int64_t ld, bool opt = false) {
    ai[n_in++] = Arr{rows, cols, ld, opt, false, 0, nullptr};
  };
  auto O = [&](int64_t rows, int64_t cols, int64_t ld, bool opt = false, bool io = false) {
    ao[n_out++] = Arr{rows, cols, ld, opt, io, 0, nullptr};
  };
  auto V = [&](int64_t len, bool opt = false) { I(1, len, len, opt); };
  auto in_range = [](int64_t v, int64_t lo, int64_t hi) { return v >= lo && v <= hi; };
  auto flag = [](int64_t v) { return v == 0 || v == 1; };
  switch (which) {
    case 0: {  // fold_grad {b, ldp, ldh, ldg}; scal {c0, c1, c2, c3, gr, gw}
      DIAG_REQ(in_range(d0, 1, kMax), "fold_grad: b must be in 1..4096");
      DIAG_REQ(in_range(d1, d0, 2 * kMax), "fold_grad: ldp must be in b..8192");
      DIAG_REQ(!in[1] || in_range(d2, d0, 2 * kMax), "fold_grad: ldh must be in b..8192");
      DIAG_REQ(in_range(d3, d0, 2 * kMax), "fold_grad: ldg must be in b..8192");
      DIAG_REQ(in[1] || scal[3] == 0.0, "fold_grad: c3 needs H");
      DIAG_REQ(in[3] || (scal[2] == 0.0 && scal[5] == 0.0), "fold_grad: c2 and gw need w");
      I(d0, d0, d1); I(d0, d0, in[1] ? d2 : d0, true); V(d0); V(d0, true);
      O(d0, d0, d3); O(1, d0, d0);
      break;
    }
    case 1: {  // row_dots {rows, cols, lda, ldb, same}
      const bool hasb = d4 == 1 || in[1];
      DIAG_REQ(in_range(d0, 1, kMax) && in_range(d1, 1, kMax), "row_dots: rows and cols must be in 1..4096");
      DIAG_REQ(!(d1 & 1), "row_dots: cols must be even");
      DIAG_REQ(!(d2 & 1), "row_dots: lda must be even");
      DIAG_REQ(in_range(d2, d1, 2 * kMax), "row_dots: lda must be in cols..8192");
      DIAG_REQ(flag(d4), "row_dots: same is a flag");
      DIAG_REQ(!(d4 && in[1]), "row_dots: same takes B from A, in[1] must be NULL");
      DIAG_REQ(!hasb || !(d3 & 1), "row_dots: ldb must be even");
      DIAG_REQ(!hasb || (d4 ? d3 == d2 : in_range(d3, d1, 2 * kMax)), "row_dots: ldb must be in cols..8192 (lda with same)");
      DIAG_REQ(in[2] || hasb, "row_dots: neither t nor B");
      DIAG_REQ((in[2] != nullptr) == (out[0] != nullptr), "row_dots: at goes with t");
      DIAG_REQ(hasb == (out[1] != nullptr), "row_dots: ab goes with B");
      I(d0, d1, d2); I(d0, d1, hasb ? d3 : d1, true); V(d1, true);
      O(1, d0, d0, true); O(1, d0, d0, true);
      break;
    }
    case 2: {  // lr_fold_vec {mode, b, bp}; in {lam, x, at, ab, r, c, w, gc, q}
      DIAG_REQ(in_range(d0, 0, 3), "lr_fold_vec: mode must be 0..3");
      DIAG_REQ(d1 >= 1 && d2 >= d1 && d2 <= kLen, "lr_fold_vec: 1 <= b <= bp <= 2^20");
      static const int need[4] = {0x00f, 0x007, 0x1f1, 0x031};
      for (int q = 0; q < 9; ++q) V(d1, !((need[d0] >> q) & 1));
      O(1, d2, d2); O(1, d2, d2, d0 == 1);
      break;
    }
    case 3: {  // lr_combine {rows, rows_pad, cols, ldx, ldy, ldo}; scal {c0, c1, c2}
      DIAG_REQ(d0 >= 1 && d1 >= d0 && d1 <= kMax, "lr_combine: 1 <= rows <= rows_pad <= 4096");
      DIAG_REQ(in_range(d2, 1, kMax), "lr_combine: cols must be in 1..4096");
      DIAG_REQ(in_range(d3, d2, 2 * kMax), "lr_combine: ldx must be in cols..8192");
      DIAG_REQ(in_range(d4, d2, 2 * kMax), "lr_combine: ldy must be in cols..8192");
      DIAG_REQ(in_range(d5, d2, 2 * kMax), "lr_combine: ldo must be in cols..8192");
      DIAG_REQ((in[4] != nullptr) == (in[5] != nullptr), "lr_combine: u1 goes with v1");
      DIAG_REQ((in[6] != nullptr) == (in[7] != nullptr), "lr_combine: u2 goes with v2");
      I(d0, d2, d3); I(d0, d2, d4); V(d0); V(d0, true);
      V(d0, true); V(d2, true); V(d0, true); V(d2, true);
      O(d1, d2, d5);
      break;
    }
    case 4: {  // fold_sum {nslab, skip, len, stride, inplace}; scal {sgn}
      DIAG_REQ(in_range(d0, 1, 64), "fold_sum: nslab must be in 1..64");
      DIAG_REQ(in_range(d1, -1, d0 - 1), "fold_sum: skip must be in -1..nslab-1");
      DIAG_REQ(in_range(d2, 1, kLen), "fold_sum: len must be in 1..2^20");
      DIAG_REQ(in_range(d3, d2, 2 * kLen), "fold_sum: stride must be in len..2^21");
      DIAG_REQ((d0 + 1) * d3 <= ((int64_t)1 << 24), "fold_sum: the slabs exceed 2^24 doubles");
      DIAG_REQ(flag(d4), "fold_sum: inplace is a flag");
      DIAG_REQ(!(d4 && in[1]), "fold_sum: in place the base comes through out[0]");
      I(d0, d2, d3); ai[0].extra = d3;   // one NaN slab past the real ones
      V(d2, true); V(d2, true);
      O(1, d2, d2, false, d4 != 0);
      break;
    }
    case 5: {  // fold_logdet {m, b}
      DIAG_REQ(in_range(d0, 1, kLen), "fold_logdet: m must be in 1..2^20");
      DIAG_REQ(in_range(d1, 1, kLen), "fold_logdet: b must be in 1..2^20");
      V(d0); V(d0); V(d1); O(1, 1, 1);
      break;
    }
    case 6:     // row_scale {rows, cols, ld}; in {scale}; out {M (in/out)}
    case 21: {  // row_add   {rows, cols, ld}; in {mu [cols]}; out {M (in/out)}
      const char* k = which == 6 ? "row_scale: " : "row_add: ";
      DIAG_REQ(in_range(d0, 1, kMax) && in_range(d1, 1, kMax), std::string(k) + "rows and cols must be in 1..4096");
      if (which == 6) DIAG_REQ(!(d1 & 1), "row_scale: cols must be even");
      if (which == 6) DIAG_REQ(!(d2 & 1), "row_scale: ld must be even");
      DIAG_REQ(in_range(d2, d1, 2 * kMax), std::string(k) + "ld must be in cols..8192");
      V(which == 6 ? d0 : d1); O(d0, d1, d2, false, true);
      break;
    }
    case 7: {  // vec_mul {n}
      DIAG_REQ(in_range(d0, 1, kLen), "vec_mul: n must be in 1..2^20");
      V(d0); V(d0); O(1, d0, d0);
      break;
    }
    case 8: {  // blk_mdiag {n, n_pad, m_pad, ldf, ldus, ldu, ldy, alias}
      DIAG_REQ(d0 >= 1 && d1 >= d0 && d1 <= kMax, "blk_mdiag: 1 <= n <= n_pad <= 4096");
      DIAG_REQ(in_range(d2, 1, kMax), "blk_mdiag: m_pad must be in 1..4096");
      DIAG_REQ(!(d2 & 1), "blk_mdiag: m_pad must be even");
      DIAG_REQ(!(d3 & 1), "blk_mdiag: ldf must be even");
      DIAG_REQ(!(d4 & 1), "blk_mdiag: ldus must be even");
      DIAG_REQ(!(d5 & 1), "blk_mdiag: ldu must be even");
      DIAG_REQ(!(d6 & 1), "blk_mdiag: ldy must be even");
      DIAG_REQ(in_range(d3, d2, 2 * kMax) && in_range(d4, d2, 2 * kMax) && in_range(d5, d2, 2 * kMax) &&
               in_range(d6, d2, 2 * kMax), "blk_mdiag: every ld must be in m_pad..8192");
      DIAG_REQ(flag(d7), "blk_mdiag: alias is a flag");
      DIAG_REQ(!d7 || d6 == d4, "blk_mdiag: Y over US needs ldy == ldus");
      DIAG_REQ(!(d7 && in[1]), "blk_mdiag: aliased, US comes through out[2]");
      I(d0, d2, d3); I(d0, d2, d4, d7 != 0); I(d0, d2, d5); V(d0); V(d0); V(d0); V(d0);
      O(1, d1, d1); O(1, d1, d1); O(d1, d2, d6, false, d7 != 0);
      break;
    }
    case 9: {  // ns_init {b, bp, ldc}; scal {scale, pad}; in {C or NULL}
      DIAG_REQ(d0 >= 1 && d1 >= d0 && d1 <= kMax, "ns_init: 1 <= b <= bp <= 4096");
      DIAG_REQ(!in[0] || in_range(d2, d0, 2 * kMax), "ns_init: ldc must be in b..8192");
      I(d0, d0, in[0] ? d2 : d0, true); O(d1, d1, d1);
      break;
    }
    case 10:    // diag_add_const {n, ld}; scal {c}; out {M (in/out)}
    case 11: {  // sym_avg {n, ld}; out {M (in/out)}
      const char* k = which == 10 ? "diag_add_const: " : "sym_avg: ";
      DIAG_REQ(in_range(d0, 1, kMax), std::string(k) + "n must be in 1..4096");
      DIAG_REQ(in_range(d1, d0, 2 * kMax), std::string(k) + "ld must be in n..8192");
      O(d0, d0, d1, false, true);
      break;
    }
    case 12:    // scaled_row {b, bp}; scal {scale}; in {src [b]}; out {dst [bp]}
    case 18: {  // joint_resid {b, bp}; in {y, mu [b]}; out {r [bp]}
      const char* k = which == 12 ? "scaled_row: " : "joint_resid: ";
      DIAG_REQ(d0 >= 1 && d1 >= d0 && d1 <= kLen, std::string(k) + "1 <= b <= bp <= 2^20");
      V(d0); if (which == 18) V(d0);
      O(1, d1, d1);
      break;
    }
    case 13: {  // row_axpy {rows, cols, ldc, ldz}; in {Z, sv [rows]}; out {C (in/out)}
      DIAG_REQ(in_range(d0, 1, kMax) && in_range(d1, 1, kMax), "row_axpy: rows and cols must be in 1..4096");
      DIAG_REQ(in_range(d2, d1, 2 * kMax), "row_axpy: ldc must be in cols..8192");
      DIAG_REQ(in_range(d3, d1, 2 * kMax), "row_axpy: ldz must be in cols..8192");
      I(d0, d1, d3); V(d0); O(d0, d1, d2, false, true);
      break;
    }
    case 14: {  // ns_resid {n, ld}
      DIAG_REQ(in_range(d0, 1, kMax), "ns_resid: n must be in 1..4096");
      DIAG_REQ(in_range(d1, d0, 2 * kMax), "ns_resid: ld must be in n..8192");
      I(d0, d0, d1); O(1, 1, 1);
      break;
    }
    case 15: {  // es_dist {S, bp, ldd}; in {Z [S][bp], Zh [S+1][bp]}; out {D [ldd][ldd]}
      DIAG_REQ(in_range(d0, 1, kMax - 1), "es_dist: S must be in 1..4095");
      DIAG_REQ(d1 % 64 == 0, "es_dist: bp must be a multiple of 64");
      DIAG_REQ(in_range(d1, 64, kMax), "es_dist: bp must be in 64..4096");
      DIAG_REQ(in_range(d2, d0 + 1, kMax), "es_dist: ldd must be in S + 1..4096");
      I(d0, d1, d1); I(d0 + 1, d1, d1); O(d2, d2, d2);
      break;
    }
    case 16: {  // es_reduce {S, Sp, ldd, grad}; scal {beta}; out {D (in/out), rs, cs, out}
      DIAG_REQ(d0 >= 2, "es_reduce: S must be at least 2");
      DIAG_REQ(d1 >= d0 + 1, "es_reduce: Sp must be at least S + 1");
      DIAG_REQ(d1 <= kMax, "es_reduce: Sp must be at most 4096");
      DIAG_REQ(in_range(d2, d1, kMax), "es_reduce: ldd must be in Sp..4096");
      DIAG_REQ(flag(d3), "es_reduce: grad is a flag");
      DIAG_REQ(scal[0] > 0.0, "es_reduce: beta must be positive");
      O(d1, d1, d2, false, true); O(1, d1, d1, !d3); O(1, d1, d1, !d3); O(1, 1, 1);
      break;
    }
    case 17: {  // joint_cov {b, bp, d, ks, stride}; scal {sf2, sn2}; in {x [b][d], inv_ell [d], slab}
      DIAG_REQ(d1 % GPS_TILE == 0, "joint_cov: bp must be a multiple of 128");
      DIAG_REQ(in_range(d1, GPS_TILE, 1024), "joint_cov: bp must be in 128..1024");
      DIAG_REQ(in_range(d0, 1, d1), "joint_cov: b must be in 1..bp");
      DIAG_REQ(in_range(d2, 1, GPS_MAX_D), "joint_cov: d must be in 1..GPS_MAX_D");
      DIAG_REQ(d3 >= 1, "joint_cov: ks must be at least 1");
      DIAG_REQ(d3 <= 8, "joint_cov: ks must be at most 8");
      DIAG_REQ(in_range(d4, d1 * d1, 2 * d1 * d1), "joint_cov: stride must be in bp*bp..2*bp*bp");
      I(d0, d2, d2); V(d2); I(d3, d1 * d1, d4); O(d1, d1, d1);
      break;
    }
    case 19: {  // joint_dss {b}; in {logdiag, t}
      DIAG_REQ(in_range(d0, 1, kLen), "joint_dss: b must be in 1..2^20");
      V(d0); V(d0); O(1, 1, 1);
      break;
    }
    case 20: {  // sign_fill {npos, n}
      DIAG_REQ(in_range(d1, 1, kLen), "sign_fill: n must be in 1..2^20");
      DIAG_REQ(in_range(d0, 0, d1), "sign_fill: npos must be in 0..n");
      O(1, d1, d1);
      break;
    }
    case 22: {  // fitc_grad_v {n}; in {ulam, z, lam or NULL}
      DIAG_REQ(in_range(d0, 1, kLen), "fitc_grad_v: n must be in 1..2^20");
      V(d0); V(d0); V(d0, true); O(1, d0, d0);
      break;
    }
    default: {  // 23: fitc_grad_y {rows, cols, ld, alias}; in {U, UP or NULL, s1, s2}; out {Y}
      DIAG_REQ(in_range(d0, 1, kMax) && in_range(d1, 1, kMax), "fitc_grad_y: rows and cols must be in 1..4096");
      DIAG_REQ(!(d1 & 1), "fitc_grad_y: cols must be even");
      DIAG_REQ(!(d2 & 1), "fitc_grad_y: ld must be even");
      DIAG_REQ(in_range(d2, d1, 2 * kMax), "fitc_grad_y: ld must be in cols..8192");
      DIAG_REQ(flag(d3), "fitc_grad_y: alias is a flag");
      DIAG_REQ(!(d3 && in[1]), "fitc_grad_y: aliased, UP comes through out[0]");
      DIAG_REQ((in[1] || d3) == (in[3] != nullptr), "fitc_grad_y: s2 goes with UP");
      I(d0, d1, d2); I(d0, d1, d2, true); V(d0); V(d0, true); O(d0, d1, d2, false, d3 != 0);
      break;
    }
  }
  for (int q = 0; q < n_in; ++q) DIAG_REQ(in[q] || ai[q].opt, "NULL input array");
  for (int q = 0; q < n_out; ++q) DIAG_REQ(out[q] || ao[q].opt, "NULL output array");
  if (int rc = bind(ctx)) return rc;
  hipStream_t s = ctx->stream;
  auto span = [&](const Arr& a) { return ((a.rows * a.ld + a.extra + 1) & ~(int64_t)1) + kGap; };
  int64_t cap0 = 256, cap1 = 256;
  for (int q = 0; q < n_in; ++q) cap0 += span(ai[q]);
  for (int q = 0; q < n_out; ++q) cap1 += span(ao[q]);
  HIPCHK(ensure(ctx, ctx->t0, (size_t)cap0 * 8));
  HIPCHK(ensure(ctx, ctx->t1, (size_t)cap1 * 8));
  HIPCHK(hipMemsetAsync(ctx->t0.d(), 0xFF, (size_t)cap0 * 8, s));
  HIPCHK(hipMemsetAsync(ctx->t1.d(), 0xFF, (size_t)cap1 * 8, s));
  int64_t used0 = 0, used1 = 0;
  for (int q = 0; q < n_in; ++q) {
    if (!in[q]) continue;
    Arr& a = ai[q];
    a.d = ctx->t0.d() + used0;
    used0 += span(a);
    HIPCHK(hipMemcpy2DAsync(a.d, (size_t)a.ld * 8, in[q], (size_t)a.cols * 8, (size_t)a.cols * 8,
                            (size_t)a.rows, hipMemcpyHostToDevice, s));
  }
  for (int q = 0; q < n_out; ++q) {
    if (!out[q]) continue;
    Arr& a = ao[q];
    a.d = ctx->t1.d() + used1;
    used1 += span(a);
    if (a.io)  // the host image has the device's row stride; the row gaps stay NaN
      HIPCHK(hipMemcpy2DAsync(a.d, (size_t)a.ld * 8, out[q], (size_t)a.ld * 8, (size_t)a.cols * 8,
                              (size_t)a.rows, hipMemcpyHostToDevice, s));
  }
  if (used0 > cap0 || used1 > cap1) return fail(ctx, -2, std::string(kWho) + "internal: the scratch carving overran");
  auto nan2d = [&](double* p, int64_t ld, int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    return hipMemset2DAsync(p, (size_t)ld * 8, 0xFF, (size_t)cols * 8, (size_t)rows, s);
  };
  const double *i0 = ai[0].d, *i1 = ai[1].d, *i2 = ai[2].d, *i3 = ai[3].d, *i4 = ai[4].d, *i5 = ai[5].d,
               *i6 = ai[6].d, *i7 = ai[7].d, *i8 = ai[8].d;
  double *o0 = ao[0].d, *o1 = ao[1].d, *o2 = ao[2].d, *o3 = ao[3].d;
  switch (which) {
    case 0:
      HIPCHK(launch_fold_grad(i0, d1, i1, i1 ? d2 : 0, i2, i3, (int)d0, scal[0], scal[1], scal[2], scal[3],
                              scal[4], scal[5], o0, d3, o1, s));
      break;
    case 1:
      HIPCHK(launch_row_dots(i0, d2, d4 ? i0 : i1, (d4 || i1) ? d3 : 0, i2, (int)d0, (int)d1, o0, o1, s));
      break;
    case 2:
      HIPCHK(launch_lr_fold_vec((int)d0, (int)d1, (int)d2, i0, i1, i2, i3, i4, i5, i6, i7, i8, o0, o1, s));
      break;
    case 3:
      HIPCHK(launch_lr_combine(i0, d3, i1, d4, i2, i3, scal[0], i4, i5, scal[1], i6, i7, scal[2], (int)d0,
                               (int)d1, (int)d2, o0, d5, s));
      break;
    case 4:
      HIPCHK(launch_fold_sum(i0, d3, (int)d0, (int)d1, d4 ? o0 : i1, i2, scal[0], o0, d2, s));
      break;
    case 5: HIPCHK(launch_fold_logdet(i0, i1, (int)d0, i2, (int)d1, o0, s)); break;
    case 6: HIPCHK(launch_row_scale(o0, d2, (int)d0, (int)d1, i0, s)); break;
    case 7: HIPCHK(launch_vec_mul(i0, i1, (int)d0, o0, s)); break;
    case 8:
      HIPCHK(launch_blk_mdiag(i0, d3, d7 ? o2 : i1, d4, i2, d5, (int)d2, i3, i4, i5, i6, (int)d0, (int)d1,
                              o0, o1, o2, d6, s));
      break;
    case 9: HIPCHK(launch_ns_init(i0, i0 ? d2 : 0, (int)d0, (int)d1, scal[0], scal[1], o0, s)); break;
    case 10: HIPCHK(launch_diag_add_const(o0, d1, (int)d0, scal[0], s)); break;
    case 11: HIPCHK(launch_sym_avg(o0, d1, (int)d0, s)); break;
    case 12: HIPCHK(launch_scaled_row(i0, (int)d0, (int)d1, scal[0], o0, s)); break;
    case 13: HIPCHK(launch_row_axpy(o0, d2, i0, d3, i1, (int)d0, (int)d1, s)); break;
    case 14: HIPCHK(launch_ns_resid(i0, d1, (int)d0, o0, s)); break;
    case 15: HIPCHK(launch_es_dist(i0, i1, d1, (int)d0, (int)d1, o0, d2, s)); break;
    case 16:
      // what W must zero: the rows >= S and, in the rows above, the columns > S
      HIPCHK(nan2d(o0 + d0 * d2, d2, d1 - d0, d1));
      HIPCHK(nan2d(o0 + d0 + 1, d2, d0, d1 - d0 - 1));
      HIPCHK(launch_es_reduce(o0, d2, (int)d0, (int)d1, scal[0], (int)d3, o1, o2, o3, s));
      break;
    case 17: {
      JointCovParams p{};
      p.x = i0; p.b = (int)d0; p.bp = (int)d1; p.d = (int)d2;
      p.sf2 = scal[0]; p.sn2 = scal[1];
      for (int k = 0; k < (int)d2; ++k) p.inv_ell[k] = in[1][k];
      p.slab = i2; p.stride = d4; p.ks = (int)d3; p.out = o0;
      for (int64_t q = 0; q < d3; ++q) {  // NaN where the kernel must override or not read
        double* sl = const_cast<double*>(i2) + q * d4;
        HIPCHK(nan2d(sl + d0 * d1, d1, d1 - d0, d1));
        HIPCHK(nan2d(sl + d0, d1, d0, d1 - d0));
        for (int64_t t = 0; (t + 1) * 32 < d1; ++t)
          HIPCHK(nan2d(sl + t * 32 * d1 + (t + 1) * 32, d1, 32, d1 - (t + 1) * 32));
      }
      HIPCHK(launch_joint_cov(p, s));
      break;
    }
    case 18: HIPCHK(launch_joint_resid(i0, i1, (int)d0, (int)d1, o0, s)); break;
    case 19: HIPCHK(launch_joint_dss(i0, i1, (int)d0, o0, s)); break;
    case 20: HIPCHK(launch_sign_fill(o0, (int)d0, (int)d1, s)); break;
    case 21: HIPCHK(launch_row_add(o0, d2, i0, (int)d0, (int)d1, s)); break;
    case 22: HIPCHK(launch_fitc_grad_v(i0, i1, i2, (int)d0, o0, s)); break;
    default:
      HIPCHK(launch_fitc_grad_y(i0, d3 ? o0 : i1, d2, i2, i3, (int)d0, (int)d1, o0, s));
      break;
  }
  for (int q = 0; q < n_out; ++q)
    if (out[q])
      HIPCHK(hipMemcpyAsync(out[q], ao[q].d, (size_t)(ao[q].rows * ao[q].ld + kGap) * 8,
                            hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}
#undef DIAG_REQ

int64_t gps_gemm_schedule(const gps_gemm_desc* d, const int32_t* kr, int have_kscale, int slots,
                          int32_t* plan, int32_t* items, int64_t cap) {
  if (!d || !plan || cap < 0 || (cap > 0 && !items) || slots < 0 || slots > 4096)
    return fail(nullptr, -1, "gps_gemm_schedule: bad argument");
  DiagExtents x;
  std::string why;
  if (!diag_check(*d, true, have_kscale != 0, true, kr, true, true, x, why))
    return fail(nullptr, -1, "gps_gemm_schedule: " + why);
  // the arrays are never touched (nothing is launched); what gemm() would hand the launch on the
  // main stream is marked present: the stream's workspace and, with it, the stream-K tickets
  static double mark[2];
  GemmParams p = desc_params(*d);
  p.A = p.B = mark; p.C = p.out0 = p.out1 = mark; p.w = mark;
  p.kscale = have_kscale ? mark : nullptr;
  p.kr = d->tri == TRI_KR_J ? kr : nullptr;
  if (own_slabs(*d) || (d->epi == EPI_STORE && (p.ksplit == 1 || p.tile == 64))) {
    p.ws = mark;
    p.ws_cap = kSplitWsDoubles;
    if (!own_slabs(*d) && slots > 0) {
      p.sk_cnt = reinterpret_cast<int*>(mark);
      p.sk_slots = slots;
    }
  }
  GemmLaunchInfo info{};
  const int64_t n = gemm_schedule(d->lay_a, d->lay_b, d->epi, p, info, items, cap);
  if (n < 0) return fail(nullptr, -1, "gps_gemm_schedule: launch_gemm refuses the launch");
  const int v[GPS_N_GEMM_PLAN] = {info.tile, info.ksplit, info.map_mode, info.sk_dp,
                                  info.sk_wgs, info.slab_xcd, info.grid_x, info.grid_y};
  for (int i = 0; i < GPS_N_GEMM_PLAN; ++i) plan[i] = v[i];
  return n;
}

int gps_gemm_pipe_resolved(const gps_gemm_desc* d, const int32_t* kr, int have_kscale, int pipe) {
  if (!d) return fail(nullptr, -1, "gps_gemm_pipe_resolved: bad argument");
  DiagExtents x;
  std::string why;
  if (!diag_check(*d, true, have_kscale != 0, true, kr, true, true, x, why))
    return fail(nullptr, -1, "gps_gemm_pipe_resolved: " + why);
  static double mark[2];  // (as gps_gemm_schedule: nothing is launched, no array is touched)
  GemmParams p = desc_params(*d);
  p.A = p.B = mark; p.C = p.out0 = p.out1 = mark; p.w = mark;
  p.kscale = have_kscale ? mark : nullptr;
  p.kr = d->tri == TRI_KR_J ? kr : nullptr;
  if (own_slabs(*d) || (d->epi == EPI_STORE && (p.ksplit == 1 || p.tile == 64))) {
    p.ws = mark;
    p.ws_cap = kSplitWsDoubles;
  }
  p.pipe = pipe;  // (what gemm() copies from the context's option)
  GemmLaunchInfo info{};
  GemmParams q;
  if (launch_gemm(d->lay_a, d->lay_b, d->epi, p, nullptr, &info, &q) != hipSuccess)
    return fail(nullptr, -1, "gps_gemm_pipe_resolved: launch_gemm refuses the launch");
  return q.pipe;
}

}  // extern "C"
