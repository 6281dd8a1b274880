// Persistent factorisation (csrc/kernels_potrf.hip, dag::potrf_dag_kernel) on one diagonal block
// of T 128-tiles, standalone: timing over repeated launches, a sampled correctness check
// (L·Lᵀ = A and L⁻¹·L = I on random entries), and one traced launch whose per-slot timestamps
// go to a CSV for tools/dag_trace.py (critical path, hand-off latencies, per-type durations).
//   dag_bench [T=20] [nwg=256] [trace.csv|-] [reps=20] [group=3] [order=1] [fine=1] [weights|-]
//             [B=1] [g=0] [form=0]
// B, g: the K batches of the UPD / UPDX tasks (GPS_OPT_DAG_KBATCH); form: the batches that run in
// tile form (GPS_OPT_DAG_TILE_FORM's value, minlen | d << 4; its rank factor is an eighth weight).
// A traced launch always runs:
// the bulk strip-task rate printed beside the block time is the flops of the UPD / UPDX strip
// tasks over their fetch-to-done time, summed over the workgroups (what the off-chain tasks
// sustain, waits included), with the mean fetch-to-done and ready-to-done time per strip task;
// the tile-form tasks are reported on a line of their own (count, times, rate while they run).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <vector>
#include "kernels_potrf.hip"
using namespace gps;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  const int T = argc > 1 ? atoi(argv[1]) : 20;
  const int nwg = argc > 2 ? atoi(argv[2]) : 256;
  const char* tpath = argc > 3 && argv[3][0] != '-' ? argv[3] : nullptr;
  const int reps = argc > 4 ? atoi(argv[4]) : 20;
  const int group = argc > 5 ? atoi(argv[5]) : 3;
  const int order = argc > 6 ? atoi(argv[6]) : 1;
  const int fine = argc > 7 ? atoi(argv[7]) : 1;
  const int kb = argc > 9 ? atoi(argv[9]) : 1;
  const int kg = argc > 10 ? atoi(argv[10]) : 0;
  const int tf = argc > 11 ? atoi(argv[11]) : 0;
  if (kb < 1 || kb > 8 || kg < 0 || kg > 3) { fprintf(stderr, "B in 1..8, g in 0..3\n"); return 2; }
  if (tf < 0 || tf > 255 || (tf & 15) > 8 || (tf && !(tf & 15))) { fprintf(stderr, "form: 0 or minlen (1..8) | d << 4\n"); return 2; }
  if (argc > 8 && argv[8][0] != '-') {  // order 1's weights: LEAF,fine,TRSM,UPD,UPDX,FIN,hand-off
    double* w = gps::g_dag_weights;
    if (sscanf(argv[8], "%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf", w, w + 1, w + 2, w + 3, w + 4, w + 5, w + 6, w + 7) < 7) {
      fprintf(stderr, "weights: 7 or 8 comma-separated numbers\n");
      return 2;
    }
  }
  const int n = 128 * T, d = 8;
  // SPD test block: ARD-style Gram of random points + noise (what the recursion hands down)
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd;
  std::vector<double> X((size_t)n * d), h((size_t)n * n);
  for (auto& x : X) x = nd(rng);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0;
      for (int k = 0; k < d; ++k) { const double t = X[i * d + k] - X[j * d + k]; s += t * t; }
      h[(size_t)i * n + j] = exp(-0.25 * s) + (i == j ? 0.05 : 0.0);
    }
  const std::vector<uint32_t> tl = dag_task_list(T, order, fine != 0, kb, kg, tf);
  const int nt = (int)tl.size();
  double *A0, *A, *Li, *ld;
  int *info, *cnt;
  uint32_t* tasks;
  unsigned long long* trace;
  const size_t bytes = (size_t)n * n * 8;
  CK(hipMalloc(&A0, bytes)); CK(hipMalloc(&A, bytes)); CK(hipMalloc(&Li, bytes));
  CK(hipMalloc(&ld, n * 8)); CK(hipMalloc(&info, 8));
  const int64_t ncnt = dag_cnt_ints(T);
  CK(hipMalloc(&cnt, ncnt * 4));
  CK(hipMemset(cnt, 0, ncnt * 4));
  CK(hipMalloc(&tasks, nt * 4));
  CK(hipMalloc(&trace, (size_t)nt * 32));
  CK(hipMemcpy(A0, h.data(), bytes, hipMemcpyHostToDevice));
  CK(hipMemcpy(tasks, tl.data(), nt * 4, hipMemcpyHostToDevice));
  DagParams p;
  p.A = A; p.lda = n; p.Linv = Li; p.ldl = n; p.Lout = nullptr; p.ldlo = 0;
  p.logdiag = ld; p.info = info; p.base = 0; p.nreal = n; p.T = T;
  p.tasks = tasks; p.ntasks = nt; p.cnt = cnt; p.spin_ticks = 200000000ull; p.group = group; p.kbatch = kb;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto launch = [&](bool tr, float* ms) {
    CK(hipMemcpy(A, A0, bytes, hipMemcpyDeviceToDevice));
    CK(hipMemset(Li, 0, bytes));
    CK(hipMemset(info, 0x7f, 8));  // (the counters stay zero between launches: self-reset)
    CK(hipDeviceSynchronize());
    p.trace = tr ? trace : nullptr;
    CK(hipEventRecord(e0, 0));
    CK(launch_potrf_dag(p, nwg, 0));
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(ms, e0, e1));
    int hinfo[2];
    CK(hipMemcpy(hinfo, info, 8, hipMemcpyDeviceToHost));
    if (hinfo[1] != 0x7f7f7f7f) { fprintf(stderr, "dependency wait timed out\n"); exit(2); }
    if (hinfo[0] != 0x7f7f7f7f) { fprintf(stderr, "not PD at %d\n", hinfo[0]); exit(2); }
  };
  std::vector<float> ts;
  for (int r = 0; r < reps + 2; ++r) {
    float ms;
    launch(false, &ms);
    if (r >= 2) ts.push_back(ms);
  }
  std::sort(ts.begin(), ts.end());
  // sampled check on the last untraced launch: L (strict lower in A, diagonal from logdiag)
  std::vector<double> gA((size_t)n * n), gX((size_t)n * n), gld(n);
  CK(hipMemcpy(gA.data(), A, bytes, hipMemcpyDeviceToHost));
  CK(hipMemcpy(gX.data(), Li, bytes, hipMemcpyDeviceToHost));
  CK(hipMemcpy(gld.data(), ld, n * 8, hipMemcpyDeviceToHost));
  // the leaf keeps A's diagonal tiles as input; L's diagonal tiles are X_kk⁻¹ — rebuild L from
  // the off-diagonal tiles (written by TRSM) and the diagonal tiles inverted on the host is
  // costly, so check X·A·Xᵀ = I on sampled entries instead (A from the host copy)
  std::uniform_int_distribution<int> ui(0, n - 1);
  double err = 0.0;
  std::vector<double> v(n);
  for (int s = 0; s < 24; ++s) {
    const int i = ui(rng), j = ui(rng);
    // (X A Xᵀ)_ij = Σ_a X_ia Σ_b A_ab X_jb
    for (int a = 0; a < n; ++a) {
      double t = 0;
      for (int b = 0; b <= j; ++b) t += h[(size_t)a * n + b] * gX[(size_t)j * n + b];
      v[a] = t;
    }
    double r = 0;
    for (int a = 0; a <= i; ++a) r += gX[(size_t)i * n + a] * v[a];
    err = std::max(err, fabs(r - (i == j ? 1.0 : 0.0)));
  }
  double lsum = 0;
  for (double x : gld) lsum += x;
  const double fl = 2.0 * n * (double)n * n / 3.0;
  printf("group=%d order=%d fine=%d w=%s B=%d g=%d form=%d ", group, order, fine, argc > 8 ? argv[8] : "-", kb, kg, tf);
  printf("T=%d n=%d nwg=%d tasks=%d: median %.3f ms (min %.3f, max %.3f) = %.1f us/tile, %.2f TF/s; "
         "max|XAX^T - I| %.2e over 24 samples, sum log L_ii %.6f\n",
         T, n, nwg, nt, ts[ts.size() / 2], ts[0], ts.back(), 1e3 * ts[ts.size() / 2] / T,
         fl / (ts[ts.size() / 2] * 1e-3) / 1e12, err, lsum);
  {
    float ms;
    launch(true, &ms);
    std::vector<unsigned long long> tr((size_t)nt * 4);
    CK(hipMemcpy(tr.data(), trace, (size_t)nt * 32, hipMemcpyDeviceToHost));
    double bflop = 0.0, bticks = 0.0, rticks = 0.0, tflop = 0.0, tticks = 0.0, trticks = 0.0;
    long nb = 0, ntf = 0;
    for (int t = 0; t < nt; ++t) {
      const dag::Task w = dag::decode(tl[t]);
      const int type = w.type, part = w.part, i = w.i, j = w.j, k = w.k, len = w.len;
      if (w.fine || (type != 2 && type != 3)) continue;
      if (w.tile) {  // tile form: four 64×64 blocks, the clipped first UPDX term from 64·(w & 1)
        tflop += 4.0 * 2.0 * 64 * 64 * 128.0 * len - (type == 3 && j == k ? 2.0 * 2.0 * 64 * 64 * 64.0 : 0.0);
        tticks += (double)(tr[4 * t + 2] - tr[4 * t]);
        trticks += (double)(tr[4 * t + 2] - tr[4 * t + 1]);
        ++ntf;
        continue;
      }
      // 32×32 blocks the strip's four waves run: UPD on a diagonal tile the lower ones only; the
      // first UPDX term starts at the wave's own column (X_kk lower)
      double f = 0.0;
      for (int wv = 0; wv < 4; ++wv) {
        if (type == 2 && i == j && wv > part) continue;
        f += 2.0 * 32 * 32 * (128.0 * len - (type == 3 && j == k ? 32.0 * wv : 0.0));
      }
      bflop += f;
      bticks += (double)(tr[4 * t + 2] - tr[4 * t]);
      rticks += (double)(tr[4 * t + 2] - tr[4 * t + 1]);
      ++nb;
    }
    // ticks are 10 ns; the tasks of one workgroup run one after another, nwg of them side by side
    printf("bulk strip tasks (traced launch %.3f ms): %ld UPD/UPDX strips, %.2f us fetch-to-done, %.2f us "
           "ready-to-done, %.1f TF/s over %d workgroups\n", ms, nb, bticks / nb * 1e-2, rticks / nb * 1e-2,
           bflop / (bticks * 1e-8) * nwg / 1e12, nwg);
    if (ntf)
      printf("bulk tile-form tasks: %ld UPD/UPDX tiles, %.2f us fetch-to-done, %.2f us ready-to-done, %.1f TF/s "
             "while running (ready-to-done) and %.1f TF/s fetch-to-done over %d workgroups\n", ntf,
             tticks / ntf * 1e-2, trticks / ntf * 1e-2, tflop / (trticks * 1e-8) * nwg / 1e12,
             tflop / (tticks * 1e-8) * nwg / 1e12, nwg);
    if (!tpath) return err < 1e-8 ? 0 : 3;
    FILE* f = fopen(tpath, "w");
    fprintf(f, "slot,word,fetch,ready,done,wg,xcc\n");
    for (int t = 0; t < nt; ++t)
      fprintf(f, "%d,%u,%llu,%llu,%llu,%llu,%llu\n", t, tl[t], tr[4 * t], tr[4 * t + 1], tr[4 * t + 2],
              tr[4 * t + 3] >> 8, tr[4 * t + 3] & 15);
    fclose(f);
    printf("traced launch %.3f ms -> %s\n", ms, tpath);
  }
  return err < 1e-8 ? 0 : 3;
}
