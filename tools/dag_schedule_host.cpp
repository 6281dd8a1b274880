// The persistent factorisation's list generator and counter protocol (csrc/dag_schedule.hip,
// csrc/dag_task.h) as a plain C++ host program, for a sanitizer build of its own:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I csrc tools/dag_schedule_host.cpp && ./a.out
// Per case: every word round-trips through decode / encode; replayed in queue order, every task's
// polled counts are met; the final counters are the closed form (tests/dag_model.py final_counts).
// tests/test_dag_protocol.py builds and runs it.
#include <cstdio>
#include <cstdlib>

#include "dag_schedule.hip"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (T=%d slot %zu)\n", __FILE__, __LINE__, #c, T, s); exit(1); } } while (0)

static size_t run(int T, int order, int kb, int kg, int tf) {
  using namespace gps;
  const std::vector<uint32_t> tl = dag_task_list(T, order, true, kb, kg, tf);
  std::vector<int> cnt(2 * T * T, 0);  // acnt at 0, xcnt at T·T
  size_t s = 0;
  for (; s < tl.size(); ++s) {
    const dag::Task t = dag::decode(tl[s]);
    CHECK(dag::encode(t) == tl[s]);
    int c[3] = {-1, -1, -1}, v[3] = {0, 0, 0};
    dag::poll_rule<int>(t.type, t.i, t.j, t.k, t.len, T, 0, T * T, c[0], v[0], c[1], v[1], c[2], v[2]);
    CHECK(c[0] >= 0);
    for (int q = 0; q < 3; ++q) CHECK(c[q] < 0 || cnt.at(c[q]) >= v[q]);
    int out = -1, out2 = -1, inc = 0;
    dag::arrival_rule<int>(t, T, 0, T * T, out, inc, out2);
    cnt.at(out) += inc;
    if (out2 >= 0) cnt.at(out2) += 1;
  }
  for (int i = 0; i < T; ++i)
    for (int j = 0; j <= i; ++j) {
      CHECK(cnt[i * T + j] == (i == j ? dag::U * i + 1 : dag::U * (j + 1)));
      CHECK(cnt[T * T + i * T + j] == (i == j ? 1 : dag::U * (i - j + 1)));
    }
  return tl.size();
}

int main() {
  size_t words = 0;
  for (int T : {2, 3, 5, 8, 21})
    for (int order : {1, 0, 2}) {
      words += run(T, order, 1, 0, 0);            // single terms
      words += run(T, order, 8, 0, 2 | 1 << 4);   // batches of 8, tile form from 2 terms, d = 1
      words += run(T, order, 4, 1, 0);            // batches of 4 in strips, the last term single
    }
  words += run(40, 1, 8, 0, 2 | 2 << 4);          // the full GP's block at the library's defaults
  printf("ok: %zu words\n", words);
  return 0;
}
