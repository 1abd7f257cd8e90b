// CPU unit test of the text rules of mapDirectly --error-profile, metamaps_amd/csrc/host/errprof_out.hpp, compiled on its own: nothing else of the program is
// included and nothing of the C ABI is called.  stdin: MM_ERRPROF_COUNTERS counters, the number of listed contigs, their indexes, then (that number + 1) rows of
// mmep::STATS values.  stdout: the four texts over the contigs cA, kraken:taxid|9|cB, cC, each behind a line "== name", then the accumulator's sums and kept entries.
#include "../metamaps_amd/csrc/host/errprof_out.hpp"
#include <cstdio>
#include <iostream>

int main() {
  std::vector<uint64_t> c(mmep::COUNTERS);
  for (auto& v : c) std::cin >> v;
  size_t n = 0;
  std::cin >> n;
  std::vector<int32_t> contig(n);
  for (auto& v : contig) std::cin >> v;
  std::vector<int64_t> stats((n + 1) * mmep::STATS);
  for (auto& v : stats) std::cin >> v;
  if (!std::cin) { fprintf(stderr, "bad input\n"); return 2; }
  const std::vector<std::string> cname{"cA", "kraken:taxid|9|cB", "cC"};
  const std::vector<int> clen{7, 2500, 3};
  std::string t = "== substitutions\n" + errprof_substitutions_text(c.data()) + "== indels\n" + errprof_indels_text(c.data()) + "== qualities\n" + errprof_qualities_text(c.data());
  t += "== contigs\n" + errprof_contigs_text(contig, stats, cname, clen);
  t += std::string("== any quality\n") + (errprof_any_quality(c.data()) ? "1\n" : "0\n");
  ErrprofAcc acc;                                                   // two batches: the sums add, the entries that do not count are dropped
  acc.add(c.data(), {5, mmep::NO_KEY, 7}, {1, 2, 3, 4, 5, 6, 9, 9, 9, 9, 9, 9, 7, 8, 9, 10, 11, 12});
  acc.add(c.data(), {mmep::NO_KEY}, {0, 0, 0, 0, 0, 0});
  t += "== accumulator\n";
  bool twice = true;
  for (uint32_t k = 0; k < mmep::COUNTERS; ++k) twice = twice && acc.counters[k] == 2 * c[k];
  t += twice ? "twice" : "not twice";
  for (uint64_t k : acc.key) t += " " + std::to_string(k);
  for (int32_t v : acc.cols) t += " " + std::to_string(v);
  t += "\n";
  fwrite(t.data(), 1, t.size(), stdout);
  return 0;
}
