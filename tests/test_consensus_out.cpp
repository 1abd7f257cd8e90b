// CPU unit test of the text rules of mapDirectly --consensus, metamaps_amd/csrc/host/consensus_out.hpp, compiled on its own: nothing else of the program is
// included and nothing of the C ABI is called.  The expected values are the Python side's (tests/test_consensus_out.py).
//   text                       the .tsv's header, one row and a ">contigID" line
//   opts [KEY VALUE]...        the thresholds those options give: "on min_depth min_frac min_called" (or the program ends with status 1 and a message)
//   groups MAX LEN... : C...   the groups of contigs of the lengths LEN for intervals on the contigs C (any order) at MAX bases: "lo hi" per group
#include "../metamaps_amd/csrc/host/consensus_out.hpp"
#include <cstdio>
#include <cstring>

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "text") {
    std::string t = cons_tsv_header();
    const int64_t stats[mmc::STATS] = {200, 28594, 1, 29997, 29, 6, 39, 3, 36, 0};
    cons_tsv_row("kraken:taxid|9|cB", 30000, stats, t);
    t += cons_fasta_name("kraken:taxid|9|cB");
    fwrite(t.data(), 1, t.size(), stdout);
    return 0;
  }
  if (mode == "opts") {
    Options o;
    for (int i = 2; i + 1 < argc; i += 2) o.v[argv[i]] = argv[i + 1];
    const ConsOpts p = consensus_options(o);
    printf("%d %lld %.17g %.17g\n", (int)p.on, p.min_depth, p.min_frac, p.min_called);
    return 0;
  }
  if (mode == "groups" && argc > 2) {
    std::vector<int> clen; std::vector<int32_t> contig;
    int i = 3;
    for (; i < argc && strcmp(argv[i], ":") != 0; ++i) clen.push_back(atoi(argv[i]));
    for (++i; i < argc; ++i) contig.push_back(atoi(argv[i]));
    std::vector<int32_t> sorted;
    for (size_t k : cons_interval_order(contig)) sorted.push_back(contig[k]);
    for (const ConsGroupRange& g : cons_groups(clen, sorted, atoll(argv[2]))) printf("%d %d\n", g.lo, g.hi);
    return 0;
  }
  fprintf(stderr, "usage: test_consensus_out text|opts|groups ...\n");
  return 2;
}
