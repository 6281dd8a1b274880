// Batches of full GPs of up to GPS_BATCH_FULL_TALL_MAX_N = 512 training rows, one workgroup of 256
// threads per problem, on the pointwise objectives (NLML, LOO-CRPS, LOO-LogS).  DESIGN §24.  The
// kernel's text — the tile product, the factorisation, forward(), gradient() and the body with the
// SGD loop and the final pass — is in batch_full_tall_shared.h, which the block-LOO kernel
// (kernels_batch_full_tall_block.hip) includes too; this file is the kernel's entry,
// its sizes and its launcher.
#include "batch_full_tall_shared.h"

namespace gps {

namespace {

__global__ __launch_bounds__(BT) void batch_full_tall_kernel(BatchFullTallParams tp) {
  tall_body<false>(tp.b, tp.ws, tp.ws_stride, 0, 0, nullptr, nullptr);
}

// the same fit with the validation rows scored at the checkpoints
__global__ __launch_bounds__(BT) void batch_full_tall_va_kernel(BatchFullTallParams tp) {
  tall_body<false, true>(tp.b, tp.ws, tp.ws_stride, 0, 0, nullptr, nullptr);
}

}  // namespace

size_t batch_full_tall_lds_bytes(int n) {
  return (size_t)(T * TL + kPan + 8 * padded(n) + 2 * T + BG * 16 + kThDoubles) * sizeof(double);
}

int64_t batch_full_tall_ws_doubles(int64_t n) {
  const int64_t np = padded(n);
  return 2 * np * np;
}

int batch_full_tall_steps(int64_t n) {
  const int64_t nb = padded(n) / T;
  const int64_t s = 1024 / (nb * nb * nb);
  return (int)(s < 1 ? 1 : s > kBatchStepsPerLaunch ? kBatchStepsPerLaunch : s);
}

hipError_t launch_batch_full_tall(const BatchFullTallParams& tp, hipStream_t s) {
  const BatchParams& p = tp.b;
  if (!full_tall_args_ok(p, batch_full_tall_steps, tp.ws, tp.ws_stride,
                         batch_full_tall_ws_doubles(p.n)))
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds((const void*)batch_full_tall_kernel,
                                         batch_full_tall_lds_bytes(GPS_BATCH_FULL_TALL_MAX_N));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_full_tall_kernel, dim3((unsigned)p.nprob), dim3(BT),
                     batch_full_tall_lds_bytes(p.n), s, tp);
  return hipGetLastError();
}

hipError_t launch_batch_full_tall_va(const BatchFullTallParams& tp, hipStream_t s) {
  const BatchParams& p = tp.b;
  if (!full_tall_va_args_ok(p) ||
      !full_tall_args_ok(p, batch_full_tall_steps, tp.ws, tp.ws_stride,
                         batch_full_tall_ws_doubles(p.n)))
    return hipErrorInvalidValue;
  const hipError_t e = raise_dynamic_lds((const void*)batch_full_tall_va_kernel,
                                         batch_full_tall_lds_bytes(GPS_BATCH_FULL_TALL_MAX_N));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_full_tall_va_kernel, dim3((unsigned)p.nprob), dim3(BT),
                     batch_full_tall_lds_bytes(p.n), s, tp);  // LDS and workspace as without
  return hipGetLastError();
}

}  // namespace gps
