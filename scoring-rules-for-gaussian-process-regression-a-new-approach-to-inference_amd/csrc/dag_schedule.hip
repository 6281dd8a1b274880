// The persistent factorisation's task list (dag::potrf_dag_kernel, kernels_potrf.hip): host only,
// the task word and the counter protocol from dag_task.h.  Standard headers only, so this file
// also builds as plain C++ (tools/dag_schedule_host.cpp).
#include <algorithm>
#include <queue>
#include <vector>

#include "dag_task.h"

namespace gps {

// Queue order of the persistent factorisation's tasks for a block of T tiles: tile tasks with
// their dependencies, then Kahn's algorithm releasing the ready task of best priority first (so
// the order is topological whatever the priorities), each tile task expanded into its NP strips.
//   order 0: earliest estimated start first (a forward critical-path pass; estimated µs: leaf 36,
//            strip task 4, hand-off 3) — round 3's first build;
//   order 1: largest upward rank first (the longest estimated path from the task to the end of
//            the block, with per-type durations), so the updates that feed the next leaves
//            overtake the bulk of the trailing update (the first leaves waited 20-26 µs behind
//            it), with the durations the round-4 traces measured (below);
//   order 2: the same with round 3's weights (leaf 38, strip 9, fine part 4, hand-off 1).
// fine: the leaf chain's TRSM(k+1,k) and UPD(k+1,k+1,k) as fine parts (8 / 16, see run_fine).
// (Round 4's split chain — the leaf without its inverse, TRSM(k+1,k) by substitution, an INV task
// off the chain — measured slower and was removed: profiles/r4_dag_split_ab.txt,
// profiles/r5_prune_split_chain.diff.)
// The word of each queue slot: dag::encode (dag_task.h).
// order 1's weights, µs: LEAF, fine part, TRSM, UPD, UPDX, FIN strips, hand-off, and the factor
// of a tile-form task over a strip of its batch (tools/dag_bench overrides them for sweeps; the
// library never writes them)
double g_dag_weights[8] = {35.0, 6.0, 9.7, 11.7, 11.2, 9.3, 2.5, 2.0};

std::vector<uint32_t> dag_task_list(int T, int order, bool fine, int kb, int kg, int tf) {
  // len: the K batch of an UPD / UPDX task (terms k .. k + len − 1, resp. j .. j + len − 1)
  struct Task { int type, i, j, k, len; std::vector<int> deps; double est = 0.0, rank = 0.0; int tile = 0; };
  // Tile form (GPS_OPT_DAG_TILE_FORM, tf = minlen | d << 4): a batch of an
  // off-diagonal tile with at least minlen terms whose last term ends at least d tile columns
  // short of where the tile is consumed (UPD(i, j, k0..k1−1): j − k1 ≥ d, the tile feeds
  // TRSM(i, j); UPDX(i, k, j0..j1−1): i − j1 ≥ d, it feeds FIN(i, k)) is ONE queue word, the whole
  // tile on one workgroup — a function of (T, kb, kg, tf, the tile, the batch) alone.
  const int tf_min = tf & 15, tf_d = tf >> 4 & 15;
  auto tile_form = [&](const Task& t) {
    if (!tf_min || (t.type != 2 && t.type != 3) || t.len < tf_min) return false;
    return t.type == 2 ? t.i > t.j && t.j - (t.k + t.len) >= tf_d : t.i - (t.j + t.len) >= tf_d;
  };
  auto is_fine = [&](const Task& t) {
    return fine && ((t.type == 1 && t.i == t.k + 1) || (t.type == 2 && t.i == t.k + 1 && t.j == t.i));
  };
  // K batches: of the nt terms of a tile, numbered in the order they are applied,
  // the first nt − keep go in runs of kb from term 0 (the last run shortened) and the last keep
  // stay single — a function of (kb, kg, the tile) alone, never of the order or the width.
  // [b0, b1): the run of term t.
  auto batch_of = [&](int t, int nt, int keep, int& b0, int& b1) {
    const int nbat = kb > 1 ? std::max(0, nt - keep) : 0;
    if (t >= nbat) { b0 = t; b1 = t + 1; return; }
    b0 = t / kb * kb;
    b1 = std::min(b0 + kb, nbat);
  };
  std::vector<Task> tk;
  std::vector<int> leaf(T), xkk(T), trsm(T * T, -1), fin(T * T, -1);
  std::vector<int> upd_last(T * T, -1), updx_last(T * T, -1);
  auto add = [&](int type, int i, int j, int k, int len, std::vector<int> deps) {
    Task t;
    t.type = type; t.i = i; t.j = j; t.k = k; t.len = len;
    t.tile = tile_form(t);
    for (int d : deps)
      if (d >= 0) t.deps.push_back(d);
    tk.push_back(t);
    return (int)tk.size() - 1;
  };
  // factorisation, right-looking (generation order is topological)
  for (int k = 0; k < T; ++k) {
    leaf[k] = add(0, k, k, k, 1, {upd_last[k * T + k]});
    xkk[k] = leaf[k];  // the task X_kk comes from
    for (int i = k + 1; i < T; ++i) trsm[i * T + k] = add(1, i, k, k, 1, {upd_last[i * T + k], xkk[k]});
    for (int j = k + 1; j < T; ++j)
      for (int i = j; i < T; ++i) {
        // tile (i, j)'s terms k' < j; the chain's UPD(k+1,k+1,k) is a tile's last term and stays
        // a fine task of its own.  A batch is generated with its last term, when every L it reads
        // exists.
        int b0, b1;
        batch_of(k, j, std::max(kg, fine && i == j ? 1 : 0), b0, b1);
        if (k != b1 - 1) continue;
        std::vector<int> deps = {upd_last[i * T + j]};
        for (int q = b0; q < b1; ++q) { deps.push_back(trsm[i * T + q]); deps.push_back(trsm[j * T + q]); }
        if (b1 - b0 == 1) deps = {trsm[i * T + k], trsm[j * T + k], upd_last[i * T + j]};
        upd_last[i * T + j] = add(2, i, j, b0, b1 - b0, deps);
      }
  }
  // inverse: X row j final → its terms pushed into every row i > j
  auto xfinal = [&](int j, int k) { return j == k ? xkk[k] : fin[j * T + k]; };
  for (int j = 0; j < T; ++j) {
    for (int k = 0; k < j; ++k)  // X_jk = −X_jj S_jk once every term j' < j is in
      fin[j * T + k] = add(4, j, k, k, 1, {updx_last[j * T + k], xkk[j]});
    for (int i = j + 1; i < T; ++i)
      for (int k = 0; k <= j; ++k) {
        int b0, b1;  // tile (i, k)'s terms j' in [k, i), numbered from k
        batch_of(j - k, i - k, kg, b0, b1);
        if (j - k != b1 - 1) continue;
        std::vector<int> deps = {updx_last[i * T + k]};
        for (int q = b0 + k; q < b1 + k; ++q) { deps.push_back(trsm[i * T + q]); deps.push_back(xfinal(q, k)); }
        if (b1 - b0 == 1) deps = {trsm[i * T + j], xfinal(j, k), updx_last[i * T + k]};
        updx_last[i * T + k] = add(3, i, b0 + k, k, b1 - b0, deps);
      }
  }
  const int n = (int)tk.size();
  std::vector<std::vector<int>> succ(n);
  std::vector<int> indeg(n, 0);
  for (int t = 0; t < n; ++t)
    for (int d : tk[t].deps) { succ[d].push_back(t); ++indeg[t]; }
  if (order == 0) {
    auto dur = [&](const Task& t) { return t.type == 0 ? 36.0 : 4.0 * t.len * (t.tile ? 2.0 : 1.0); };
    for (int t = 0; t < n; ++t)  // generation order is topological
      for (int d : tk[t].deps) tk[t].est = std::max(tk[t].est, tk[d].est + dur(tk[d]) + 3.0);
  } else if (order == 2) {  // round 3's weights
    auto dur = [&](const Task& t) {
      return t.type == 0 ? 38.0 : is_fine(t) ? 4.0 : 9.0 * t.len * (t.tile ? 2.0 : 1.0);
    };
    for (int t = n - 1; t >= 0; --t) {
      double m = 0.0;
      for (int s2 : succ[t]) m = std::max(m, tk[s2].rank + 1.0);
      tk[t].rank = dur(tk[t]) + m;
      tk[t].est = -tk[t].rank;
    }
  } else {
    // run time per strip task as the round-4 trace measured it (profiles/r4_dag_trace20_*.txt);
    // the fine parts count 6 (they run 8.5 but 8-16 of them in parallel) and each hand-off 2.5
    // (profiles/r4_dag_order_ab.txt: 3.6 % off the block against the round-3 weights)
    const double* w = g_dag_weights;
    auto dur = [&](const Task& t) {
      if (is_fine(t)) return w[1];
      const double tw = t.tile ? w[7] : 1.0;  // (a tile-form task runs its four strips' work)
      switch (t.type) {
        case 0: return w[0];
        case 1: return w[2];
        case 2: return w[3] * t.len * tw;  // (a K batch weighs as its K)
        case 3: return w[4] * t.len * tw;
        default: return w[5];
      }
    };
    for (int t = n - 1; t >= 0; --t) {  // reverse generation order: successors first
      double m = 0.0;
      for (int s2 : succ[t]) m = std::max(m, tk[s2].rank + w[6]);
      tk[t].rank = dur(tk[t]) + m;
      tk[t].est = -tk[t].rank;  // smallest key first
    }
  }
  std::priority_queue<std::pair<double, int>, std::vector<std::pair<double, int>>,
                      std::greater<std::pair<double, int>>> ready;
  for (int t = 0; t < n; ++t)
    if (!indeg[t]) ready.push({tk[t].est, t});
  std::vector<uint32_t> out;
  while (!ready.empty()) {
    const int t = ready.top().second;
    ready.pop();
    const Task& x = tk[t];
    const bool f = is_fine(x);
    const int parts = x.type == 0 || x.tile ? 1 : !f ? dag::NP : x.type == 1 ? dag::NPF_TRSM : dag::NPF_UPD;
    for (int q = 0; q < parts; ++q)
      out.push_back(dag::encode({x.type, q, f, x.i, x.j, x.k, x.len, x.tile}));
    for (int s2 : succ[t])
      if (!--indeg[s2]) ready.push({tk[s2].est, s2});
  }
  return out;
}

}  // namespace gps
