// Device helpers shared by the two tall FITC batch kernels, one workgroup of 256 threads per
// problem: kernels_batch_fitc_tall.hip (the pointwise objectives) and
// kernels_batch_fitc_tall_block.hip (the block-LOO objectives).  What is here is what
// moves a chunk of kBatchFitcTallChunk rows between the per-problem workspace and LDS and what
// accumulates a chunk's m-vectors and m×m blocks in a fixed order; each kernel keeps its own LDS
// and workspace layout, its own passes and its own copy of the step driver (§27 says why).
// Included once per kernel file; everything sits in that file's anonymous namespace.
#pragma once
#include "batch_fitc_shared.h"
#include "gps_internal.h"
#include "gpscore.h"

namespace gps {

namespace {

constexpr int CH = kBatchFitcTallChunk;  // rows of a chunk

__host__ __device__ constexpr int chunk_rows(int n) { return n < CH ? n : CH; }

// cnt contiguous doubles, kCopyUn loads in flight per thread before the first store: with one wave
// per SIMD nothing else hides a memory round trip, so a chunk's copy is one or two of them (one
// up to m = 24), not one per element
constexpr int kCopyUn = 12;
__device__ __forceinline__ void copy_flat(double* __restrict__ dst, const double* __restrict__ src,
                                          int cnt) {
  for (int e0 = threadIdx.x; e0 < cnt; e0 += FT * kCopyUn) {
    double r[kCopyUn];
#pragma unroll
    for (int u = 0; u < kCopyUn; ++u) r[u] = e0 + u * FT < cnt ? src[e0 + u * FT] : 0.0;
#pragma unroll
    for (int u = 0; u < kCopyUn; ++u)
      if (e0 + u * FT < cnt) dst[e0 + u * FT] = r[u];
  }
}
// two copies of one length whose loads share the round trips
__device__ __forceinline__ void copy_flat2(double* __restrict__ d1, const double* __restrict__ s1,
                                           double* __restrict__ d2, const double* __restrict__ s2,
                                           int cnt) {
  for (int e0 = threadIdx.x; e0 < cnt; e0 += FT * kCopyUn) {
    double r1[kCopyUn], r2[kCopyUn];
#pragma unroll
    for (int u = 0; u < kCopyUn; ++u) {
      const bool on = e0 + u * FT < cnt;
      r1[u] = on ? s1[e0 + u * FT] : 0.0;
      r2[u] = on ? s2[e0 + u * FT] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kCopyUn; ++u)
      if (e0 + u * FT < cnt) {
        d1[e0 + u * FT] = r1[u];
        d2[e0 + u * FT] = r2[u];
      }
  }
}

// rows [c0, c0 + rows) of a workspace matrix ↔ the chunk array: both have row stride ld, so a chunk
// is one contiguous block (the pad column of an even m travels along and is never read)
__device__ __forceinline__ void load_rows(double* dst, const double* src, int c0, int rows,
                                          int ld) {
  copy_flat(dst, src + (int64_t)c0 * ld, rows * ld);
}
__device__ __forceinline__ void store_rows(double* dst, const double* src, int c0, int rows,
                                           int ld) {
  copy_flat(dst + (int64_t)c0 * ld, src, rows * ld);
}

// out[j] (+)= Σ_i A[i][j]·w[i] over the chunk's rows (j < m): group j of C lanes, lane c takes rows
// c, c + C, ...; the group's first lane owns out[j] in every chunk
__device__ __forceinline__ void tmatvec_acc(const double* A, int lda, const double* w, int rows,
                                            int m, double* out, bool first) {
  const int C = group_lanes(m), j = threadIdx.x / C, c = threadIdx.x - j * C;
  double a = 0.0;
  if (j < m)
#pragma unroll 8
    for (int i = c; i < rows; i += C) a = fma(A[i * lda + j], w[i], a);
  a = group_sum(a, C);
  if (j < m && c == 0) out[j] = first ? a : out[j] + a;
}

// out[j][l] (+)= Σ_i A[i][j]·A[i][l]·w[i] over the chunk's rows for all m×m entries (the product
// A_ij·A_il is formed first, so the result is bitwise symmetric); the first chunk starts from
// base[j][l] (or 0).  Up to 128 entries share the workgroup as tmatvec_acc's columns do; more take
// one thread each, 256 at a time.  The lane that writes an entry is the same in every chunk.
__device__ __forceinline__ void wgram_acc(const double* A, int lda, const double* w, int rows,
                                          int m, const double* base, double* out, int ldm,
                                          bool first) {
  const int ne = m * m;
  const int C = ne <= FT / 2 ? group_lanes(ne) : 1, G = FT / C;
  const int g = threadIdx.x / C, c = threadIdx.x - g * C;
  for (int e0 = 0; e0 < ne; e0 += G) {
    const int e = e0 + g;
    const bool on = e < ne;
    const int j = on ? e / m : 0, l = on ? e - j * m : 0;
    double a = 0.0;
    if (on)
#pragma unroll 8
      for (int i = c; i < rows; i += C) a = fma(A[i * lda + j] * A[i * lda + l], w[i], a);
    a = group_sum(a, C);
    if (on && c == 0) {
      const double b0 = first ? (base ? base[j * ldm + l] : 0.0) : out[j * ldm + l];
      out[j * ldm + l] = b0 + a;
    }
  }
}

}  // namespace

}  // namespace gps
