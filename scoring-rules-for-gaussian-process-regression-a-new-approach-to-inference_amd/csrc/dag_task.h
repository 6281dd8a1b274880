// The persistent factorisation's task word and counter protocol (dag::potrf_dag_kernel,
// kernels_potrf.hip): THE definition — the list generator
// (dag_schedule.hip), the kernel, gps_dag_task_protocol (and through it tools/ and tests/) all
// use these functions.  Plain C++17 that also compiles under hipcc; no HIP header.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GPS_DAG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GPS_DAG_HD inline
#endif

namespace gps {
namespace dag {
constexpr int NP = 4;        // strips per tile task
constexpr int NPF_TRSM = 8;  // parts of a fine TRSM (16-row strips)
constexpr int NPF_UPD = 16;  // parts of a fine UPD (16 × 64 blocks)
constexpr int U = 16;        // arrivals per finished tile task: 4 per strip, 2 / 1 per fine part

// Word: type | part << 3 | fine << 7 | i << 8 | j << 16 | k << 24, i, j, k in 6 bits each; the K
// batch length − 1 of an UPD / UPDX task (0..7) in bits 14-15 (low) and 22 (high),
// k resp. j its first term — length field 0 is the single-term task of before.  Bit 23: the tile
// form of a batch (one word for the whole tile, part 0).
// type: 0 LEAF(k = i), 1 TRSM(i, k), 2 UPD(i, j, k ..), 3 UPDX(i, k, j ..), 4 FIN(i, k).
struct Task { int type, part, fine, i, j, k, len, tile; };

GPS_DAG_HD uint32_t encode(const Task& t) {
  return (uint32_t)t.type | (uint32_t)t.part << 3 | (uint32_t)t.fine << 7 | (uint32_t)t.i << 8 |
         (uint32_t)((t.len - 1) & 3) << 14 | (uint32_t)t.j << 16 |
         (uint32_t)((t.len - 1) >> 2) << 22 | (uint32_t)t.tile << 23 | (uint32_t)t.k << 24;
}

GPS_DAG_HD Task decode(uint32_t w) {
  Task t;
  t.type = w & 7; t.part = (w >> 3) & 15; t.fine = (w >> 7) & 1; t.i = (w >> 8) & 63;
  t.j = (w >> 16) & 63; t.k = (w >> 24) & 63;
  // K batch of an UPD / UPDX task: terms k .. k + len − 1, resp. j ..
  t.len = 1 + (int)((w >> 14) & 3) + 4 * (int)((w >> 22) & 1);
  t.tile = w >> 23 & 1;
  return t;
}

// The counts a task needs before it may run: up to three (counter, threshold) pairs; a pair the
// task does not use is left as the caller initialised it.  H is the counter handle: `const int*`
// into acnt / xcnt on the device, an integer offset on the host (acnt at 0, xcnt at T·T).
template <class H>
GPS_DAG_HD void poll_rule(int type, int ti, int tj, int tk, int len, int T, H acnt, H xcnt, H& c0,
                          int& v0, H& c1, int& v1, H& c2, int& v2) {
  switch (type) {
    case 0:  // LEAF(k = ti)
      c0 = acnt + ti * T + ti; v0 = U * ti;
      break;
    case 1:  // TRSM(i, k): A_ik final, X_kk from LEAF(k)
      c0 = acnt + ti * T + tk; v0 = U * tk;
      c1 = xcnt + tk * T + tk; v1 = 1;
      break;
    // (a K batch polls its LAST term's operands: L_ik final means TRSM(i, k) ran, which waited
    //  for every UPD(i, k, k') — each of which had polled L_ik' final; X_jk likewise through
    //  FIN(j, k) and the UPDX(j, k, j') — so the last counts imply the others)
    case 2: {  // UPD(i, j, k .. kl)
      const int kl = tk + len - 1;
      c0 = acnt + ti * T + kl; v0 = U * (kl + 1);
      c1 = acnt + tj * T + kl; v1 = U * (kl + 1);
      c2 = acnt + ti * T + tj; v2 = U * tk;
      break;
    }
    case 3: {  // UPDX(i, k, j .. jl): L_ij final, X_jk final, S_ik's earlier terms
      const int jl = tj + len - 1;
      c0 = acnt + ti * T + jl; v0 = U * (jl + 1);
      c1 = xcnt + jl * T + tk; v1 = jl == tk ? 1 : U * (jl - tk + 1);
      c2 = xcnt + ti * T + tk; v2 = U * (tj - tk);
      break;
    }
    case 4:  // FIN(i, k)
      c0 = xcnt + ti * T + tk; v0 = U * (ti - tk);
      c1 = xcnt + ti * T + ti; v1 = 1;
      break;
    default: break;
  }
}

// What a finished task adds: `inc` to out, and (LEAF only) 1 to out2, which is otherwise left as
// the caller initialised it.  The counters mean "U per applied term of the tile": a fine part
// adds U / NPF, a strip len · U / NP, a tile-form task (its four strips' worth) len · U; a LEAF
// adds 1 to both acnt[k][k] and xcnt[k][k].  (potrf_dag_kernel keeps a copy of these values in
// its four branches — calling this there changes its register allocation; change
// both together.)
template <class H>
GPS_DAG_HD void arrival_rule(const Task& t, int T, H acnt, H xcnt, H& out, int& inc, H& out2) {
  if (t.type == 0) {
    out = acnt + t.i * T + t.i;
    out2 = xcnt + t.i * T + t.i;
    inc = 1;
  } else if (t.fine) {  // the chain's TRSM(k+1, k) / UPD(k+1, k+1, k)
    inc = t.type == 1 ? U / NPF_TRSM : U / NPF_UPD;
    out = acnt + t.i * T + (t.type == 1 ? t.k : t.j);
  } else {
    const int per = t.tile ? U : U / NP;
    inc = (t.type == 2 || t.type == 3 ? t.len : 1) * per;
    out = t.type == 1 ? acnt + t.i * T + t.k : t.type == 2 ? acnt + t.i * T + t.j : xcnt + t.i * T + t.k;
  }
}
}  // namespace dag

// Queue order of the tasks of a block of T tiles (dag_schedule.hip).  kb: UPD / UPDX terms of one
// tile in batches of at most kb (1: every term its own task, the list of before); kg: the last kg
// terms of every tile stay single tasks; tf: the batches that run in tile form
// (GPS_OPT_DAG_TILE_FORM's value, 0: none)
std::vector<uint32_t> dag_task_list(int T, int order = 1, bool fine = true, int kb = 1, int kg = 0,
                                    int tf = 0);
// order 1's weights (dag_schedule.hip; tools/dag_bench overrides them for sweeps)
extern double g_dag_weights[8];
// head / exit / done counters (16 ints), acnt and xcnt (T² each), rounded up to 64 ints
inline int64_t dag_cnt_ints(int T) { return (16 + 2 * (int64_t)T * T + 63) / 64 * 64; }
}  // namespace gps
