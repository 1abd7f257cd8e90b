// Host build of metamaps_amd/csrc/mm_edit_trace_core.hpp for tests/test_edit_trace_core.py: one answer line per input line.
//   S strand max_dist =READ =WINDOW            ->  dist begin end n_runs run ...     the serial form (window coordinates, half-open; dist -1: not aligned)
//   P strand max_dist =READ =WINDOW            ->  dist begin end n_runs run ...     the pipeline of 64 emulated lanes
//   W m n                                      ->  the words of a job's scratch
//   L budget_words max_jobs k {m dist a b} x k ->  launches scratch_words slot_words | cut ... | scr_off ... | slot_off ...
#include "../metamaps_amd/csrc/mm_edit_trace_core.hpp"
#include <iostream>
#include <sstream>
#include <string>

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char kind = 0;
    in >> kind;
    if (kind == 'S' || kind == 'P') {
      int strand; long long md; std::string q, w;
      in >> strand >> md >> q >> w;
      const mm::TraceHostResult r = mm::bv_trace_host(q.data() + 1, (int64_t)q.size() - 1, strand, w.data() + 1, (int64_t)w.size() - 1, (int32_t)md, kind == 'P');
      std::cout << r.dist << " " << r.begin << " " << r.end << " " << r.n_runs;
      for (const uint32_t x : r.runs) std::cout << " " << x;
      std::cout << "\n";
    } else if (kind == 'W') {
      int m, n;
      in >> m >> n;
      std::cout << mm::bv_trace_words(m, n) << "\n";
    } else if (kind == 'L') {
      long long budget, max_jobs; int k;
      in >> budget >> max_jobs >> k;
      std::vector<int32_t> m(k), d(k), a(k), b(k);
      for (int i = 0; i < k; ++i) in >> m[i] >> d[i] >> a[i] >> b[i];
      const mm::TracePlan P = mm::bv_trace_plan(k, m.data(), d.data(), a.data(), b.data(), budget, max_jobs);
      std::cout << P.cut.size() - 1 << " " << P.scratch_words << " " << P.slot_words << " |";
      for (const int64_t x : P.cut) std::cout << " " << x;
      std::cout << " |";
      for (const int64_t x : P.scr_off) std::cout << " " << x;
      std::cout << " |";
      for (const int64_t x : P.slot_off) std::cout << " " << x;
      std::cout << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
