// The integer schedule of the FP64 GEMM kernels (kernels_gemm.hip): which output tile, K range,
// K slice and workspace slot a workgroup runs.  Host and device share these functions — the
// kernels call them, and gemm_schedule() (the device-less diagnostic behind gps_gemm_schedule)
// enumerates a launch's work items with them, so tests/test_gemm_schedule.py checks on the CPU
// the very code the kernels run: every tile exactly once, K slices that partition their range,
// stream-K runs that partition the tail with distinct workspace slots and matching ticket counts.
#pragma once
#include "gps_internal.h"

#define GPS_HD __host__ __device__ __forceinline__

namespace gps {

constexpr int BK = 16;
constexpr int GROUP_M = 8;

GPS_HD int sched_min(int a, int b) { return a < b ? a : b; }

// logical tile id -> (ti, tj).  Lower-triangular enumeration for SYRK outputs
// (uniform work per tile); otherwise a grouped raster (GROUP_M tile rows at a
// time, column-major inside the group) so the tiles resident together share A
// and B panels in L2.
//
// Triangular operands (work per tile grows linearly along one tile index) are
// issued heaviest-first and WITHOUT the XCD-contiguous remap.  Measured on
// MI355X (tools/gemm_bench.cpp, 20096×5120×20096 TRMM): remap + any order
// 35-45 TF/s, plain grouped order 64.6, heaviest-first 68.9.  Workgroups are
// dealt to XCDs in block order, so an XCD whose slots are all held by long tiles
// stalls the dispatch of every later block; equal-work neighbours in block order
// (which land on different XCDs) avoid that.  Map 3 (the default for triangular
// operands since the microbenchmark below) keeps that equal-work-per-XCD property
// but gives each XCD a compact band of tiles: 70.7 TF/s on the same TRMM.
GPS_HD bool tile_of(const GemmParams& p, int t, int& ti, int& tj) {
  if (p.lower_out) {
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    while (r * (r + 1) / 2 > t) --r;
    ti = r;
    tj = t - r * (r + 1) / 2;
    return true;
  }
  if (p.map_mode == 3) {
    // XCD-banded heaviest-first (triangular operands): block b runs on XCD b % 8;
    // XCD x owns a contiguous band of the index that does NOT carry the triangular
    // work and walks the other index heaviest-first, so every XCD gets the same work
    // profile (balanced under in-order dispatch) while its ~64 resident tiles form a
    // compact 2-D patch (both operand panels reused from its own L2).  Positions past
    // the matrix edge are holes (the workgroup exits at once).
    const int x = t & 7, i = t >> 3;
    if (p.tri == TRI_K_LE_I || p.tri == TRI_K_GE_I) {  // work grows/shrinks with ti
      const int bw = (p.tiles_n + 7) >> 3;
      const int ri = i / bw;
      tj = x * bw + i % bw;
      ti = p.tri == TRI_K_LE_I ? p.tiles_m - 1 - ri : ri;
      return tj < p.tiles_n && ri < p.tiles_m;
    }
    const int bh = (p.tiles_m + 7) >> 3;  // TRI_K_LE_J / TRI_K_GE_J: work follows tj
    const int cj = i / bh;
    ti = x * bh + i % bh;
    tj = p.tri == TRI_K_LE_J ? p.tiles_n - 1 - cj : cj;
    return ti < p.tiles_m && cj < p.tiles_n;
  }
  if (p.map_mode == 5) {
    // XCD-banded 8×8 patches (the automatic order of the FITC row norms): as map 3, XCD x owns
    // a band of the index that does not carry the triangular work, but its resident tiles form 8 (band) × 8
    // (work index) patches, the work index walked heaviest-first patch by patch, so an 8×8
    // group of tiles with neighbouring K ranges shares both operand panels in its L2.
    const int x = t & 7, i = t >> 3;
    const bool wi = p.tri == TRI_K_LE_I || p.tri == TRI_K_GE_I;  // work follows ti
    const int nb = wi ? p.tiles_n : p.tiles_m, nw = wi ? p.tiles_m : p.tiles_n;
    const int bb = (nb + 7) >> 3, per = ((bb + 7) >> 3) * 64;
    const int wg = i / per, rem = i - wg * per, w = rem & 63;
    const int bi = x * bb + (rem >> 6) * 8 + (w & 7), wk = wg * 8 + (w >> 3);
    if (bi >= sched_min(nb, x * bb + bb) || wk >= nw) return false;
    const int widx = (p.tri == TRI_K_LE_I || p.tri == TRI_K_LE_J) ? nw - 1 - wk : wk;
    ti = wi ? widx : bi;
    tj = wi ? bi : widx;
    return true;
  }
  const int per_group = GROUP_M * p.tiles_n;
  const int g = t / per_group;
  const int first = g * GROUP_M;
  const int gm = sched_min(GROUP_M, p.tiles_m - first);
  const int tt = t - g * per_group;
  ti = first + tt % gm;
  tj = tt / gm;
  if (p.map_mode != 0) return true;
  if (p.tri == TRI_K_LE_I) ti = p.tiles_m - 1 - ti;       // K grows with ti
  else if (p.tri == TRI_K_LE_J) tj = p.tiles_n - 1 - tj;  // K grows with tj
  // TRI_K_GE_I / TRI_K_GE_J: K shrinks with the index, natural order is heaviest-first
  return true;
}

// bijective XCD-contiguous remap: blocks b, b+8, b+16, ... (one XCD under the
// observed round-robin dispatch) get consecutive logical tile ids.
GPS_HD int xcd_remap(int b, int nblk) {
  const int q = nblk / 8, r = nblk % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// map 6, paired column tiles (row norms over a triangular L⁻¹, work ∝ tj + 1): workgroup (ri, q)
// of a grid of nblk runs column tile qh = T−1−q and then, if q < qh, q, so every workgroup has the
// same K, (T + 1)·TILE — the grid is uniform like a square product's — in a grouped raster over
// XCD-contiguous ids.  Returns whether there is a second tile (false: the middle tile of an odd
// count, which runs alone).
GPS_HD bool pair_of(const GemmParams& p, int b, int nblk, int& ri, int& q, int& qh) {
  const int np = (p.tiles_n + 1) >> 1;
  const int l = xcd_remap(b, nblk);
  const int per_group = GROUP_M * np, g = l / per_group, first = g * GROUP_M;
  const int gm = sched_min(GROUP_M, p.tiles_m - first), tt = l - g * per_group;
  ri = first + tt % gm;
  q = tt / gm;
  qh = p.tiles_n - 1 - q;
  return q < qh;
}

// split-K, slice-major per XCD: the grid's (tile, slice) pairs in slice-major order, each XCD
// a contiguous run of them, so the workgroups resident on an XCD share one K slice's rows of
// both operands in its L2 (the tile-major remap spreads an XCD over every slice).  Block
// (bx, by) of an nt × ny grid -> logical tile id t (for tile_of) and K slice.
GPS_HD void slab_xcd_of(int bx, int by, int nt, int ny, int& t, int& slice) {
  const int l = xcd_remap(bx + by * nt, nt * ny);
  t = l % nt;
  slice = l / nt;
}

// the K range [kb, ke) of the output tile at (row0, col0) with edge `tile` under the triangular
// restriction (before kend and the K split)
GPS_HD void tile_k_range(const GemmParams& p, int row0, int col0, int tile, int& kb, int& ke) {
  kb = 0;
  ke = p.K;
  switch (p.tri) {
    case TRI_K_LE_I: ke = sched_min(ke, p.tri_off + row0 + tile); break;
    case TRI_K_LE_J: ke = sched_min(ke, p.tri_off + col0 + tile); break;
    case TRI_K_GE_J: kb = p.tri_off + col0; break;
    case TRI_K_GE_I: kb = p.tri_off + row0; break;
    case TRI_KR_J:
      kb = p.kr[2 * (col0 / 16)];
      ke = p.kr[2 * ((col0 + tile) / 16 - 1) + 1];
      break;
    default: break;
  }
}

// part s of `parts` of nk 16-deep slices, as even as possible, the longer parts first: [s0, s1)
// (the split-K slices of the LDS kernel, the waves' shares in the small kernel)
GPS_HD void slice_part(int nk, int parts, int s, int& s0, int& s1) {
  const int q = nk / parts, r = nk % parts;
  s0 = s * q + sched_min(s, r);
  s1 = s0 + q + (s < r ? 1 : 0);
}

// the small kernel's block t at edge te (u = 64 / te blocks per 64-tile edge): (ti, tj), false
// past the last block.  lower_out: the blocks (ti, tj) with tj/u <= ti/u, row-major over ti
// (the blocks of the lower 64-tiles, diagonal 64-tiles whole)
template <int TE>
GPS_HD bool small_block_of(const GemmParams& p, int t, int& ti, int& tj) {
  const int tm = p.M / TE, tn = p.N / TE;
  bool valid;
  if (p.lower_out) {
    constexpr int u = 64 / TE;
    auto pre = [](int r) { const int a = r / u, b = r % u; return u * (u * a * (a + 1) / 2 + b * (a + 1)); };
    valid = t < pre(tm);
    if (valid) {
      int lo = 0, hi = tm;
      while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (pre(mid) <= t) lo = mid; else hi = mid; }
      ti = lo;
      tj = t - pre(ti);
    }
  } else {
    valid = t < tm * tn;
    if (valid) { ti = t / tn; tj = t - ti * tn; }
  }
  return valid;
}

// The stream-K tail's partition (gemm_sk_block): the I = tail tiles × nk 16-deep slices are cut
// into S contiguous runs, block s running [bnd(s), bnd(s + 1)); owner(x) is the block whose run
// holds slice x.  A tile u of the tail whose slices lie in more than one run is combined from
// the partials of blocks owner(u·nk) .. owner(u·nk + nk − 1) in workspace slots u + block — which
// needs every one of those blocks to hold a slice of the tile, i.e. no empty run: S <= I
// (launch_gemm).
struct StreamKPart {
  int64_t I, S;
  GPS_HD int64_t bnd(int64_t q) const { return q * I / S; }
  GPS_HD int owner(int64_t x) const {
    int64_t q = x * S / I;
    while (q + 1 < S && bnd(q + 1) <= x) ++q;
    while (q > 0 && bnd(q) > x) --q;
    return (int)q;
  }
};

}  // namespace gps
