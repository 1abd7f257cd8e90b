// Host build of metamaps_amd/csrc/mm_edit_core.hpp for tests/test_edit_core.py: one answer line per input line.
//   A strand max_dist =READ =WINDOW            ->  dist begin end           (window coordinates, half-open; dist -1: not aligned)
//   R strand pi ref_start =READ =CONTIG        ->  dist first last | NA     (a mapping record by the window and cap rules; inclusive contig coordinates)
//   W ref_start L C                            ->  ws we
//   C L pi                                     ->  cap
//   K read strand contig max_dist ws we n_reads n_contigs len...   ->  the refusal code of the job
#include "../metamaps_amd/csrc/mm_edit_core.hpp"
#include <iostream>
#include <sstream>
#include <string>

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char kind = 0;
    in >> kind;
    if (kind == 'A') {
      int strand; long long md; std::string q, w;
      in >> strand >> md >> q >> w;
      const mm::EditHostResult r = mm::edit_infix_host(q.data() + 1, (int64_t)q.size() - 1, strand, w.data() + 1, (int64_t)w.size() - 1, (int32_t)md);
      std::cout << r.dist << " " << r.begin << " " << r.end << "\n";
    } else if (kind == 'R') {
      int strand; float pi; long long start; std::string q, c;
      in >> strand >> pi >> start >> q >> c;
      const int64_t L = (int64_t)q.size() - 1, C = (int64_t)c.size() - 1;
      int64_t ws, we;
      mm::edit_window(start, L, C, &ws, &we);
      const mm::EditHostResult r = mm::edit_infix_host(q.data() + 1, L, strand, c.data() + 1 + ws, we - ws, mm::edit_cap(L, pi));
      if (r.dist < 0) std::cout << "NA\n"; else std::cout << r.dist << " " << ws + r.begin << " " << ws + r.end - 1 << "\n";
    } else if (kind == 'W') {
      long long s, L, C; int64_t ws, we;
      in >> s >> L >> C;
      mm::edit_window(s, L, C, &ws, &we);
      std::cout << ws << " " << we << "\n";
    } else if (kind == 'C') {
      long long L; float pi;
      in >> L >> pi;
      std::cout << mm::edit_cap(L, pi) << "\n";
    } else if (kind == 'K') {
      long long v[8];
      for (long long& x : v) in >> x;
      std::vector<int32_t> len; long long x;
      while (in >> x) len.push_back((int32_t)x);
      std::cout << mm::edit_job_check(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], len.data()) << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
