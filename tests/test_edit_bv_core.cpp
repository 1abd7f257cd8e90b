// Host build of metamaps_amd/csrc/mm_edit_bv_core.hpp for tests/test_edit_bv_core.py: one answer line per input line.
//   S strand max_dist =READ =WINDOW            ->  dist begin end           the serial form (window coordinates, half-open; dist -1: not aligned)
//   P strand max_dist =READ =WINDOW            ->  dist begin end           the pipeline of 64 emulated lanes
//   B m                                        ->  blocks per_lane class last_lane
#include "../metamaps_amd/csrc/mm_edit_bv_core.hpp"
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
      const mm::EditHostResult r = mm::bv_infix_host(q.data() + 1, (int64_t)q.size() - 1, strand, w.data() + 1, (int64_t)w.size() - 1, (int32_t)md, kind == 'P');
      std::cout << r.dist << " " << r.begin << " " << r.end << "\n";
    } else if (kind == 'B') {
      int m;
      in >> m;
      const mm::BvPass P = mm::bv_pass(m, 0, false);
      std::cout << P.blocks << " " << P.B << " " << mm::bv_class(P.B) << " " << P.last_lane << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
