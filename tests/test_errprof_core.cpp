// Host driver of metamaps_amd/csrc/mm_errprof_core.hpp (tests/test_errprof_core.py), the one-lane form of what the kernels of mm_errprof.hip run.
// The jobs of stdin, one per line
//   read n_reads contig n_contigs strand first dist use =READ =QUAL(two hex digits per base, or - for none) =CONTIG n_ops op...
// are checked (mmp::count_job) and walked into ONE table of exactly mmep::COUNTERS words on the heap (an index too many is the sanitizer's to see).
// stdout: per job "J eq x insRuns insBases delRuns delBases key", or "E rule" for a job that breaks a rule (it adds nothing); then "T" and the counters.
#include "../metamaps_amd/csrc/mm_errprof_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Read {                                                      // (at: an index outside the read throws)
  const std::string* s; const std::vector<uint8_t>* q;
  uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); }
  uint8_t qual(int64_t i) const { return q->empty() ? mmb::QUAL_NONE : q->at((size_t)i); }
};
struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); } };

int main() {
  uint64_t* const table = (uint64_t*)calloc(mmep::COUNTERS, sizeof(uint64_t));
  mmep::HostCounters t{table};
  mmp::HostLanes lanes;
  std::string line;
  size_t n_line = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    long long read_idx, n_reads, contig_idx, n_contigs, strand, first, dist, use;
    std::string read, qhex, contig; size_t n_ops = 0;
    in >> read_idx >> n_reads >> contig_idx >> n_contigs >> strand >> first >> dist >> use >> read >> qhex >> contig >> n_ops;
    std::vector<uint32_t> ops(n_ops);
    for (auto& w : ops) in >> w;
    if (!in) { fprintf(stderr, "bad line %zu\n", n_line); return 2; }
    ++n_line;
    read.erase(0, 1); qhex.erase(0, 1); contig.erase(0, 1);
    std::vector<uint8_t> qual;
    if (qhex != "-") for (size_t k = 0; k + 1 < qhex.size(); k += 2) qual.push_back((uint8_t)strtoul(qhex.substr(k, 2).c_str(), nullptr, 16));
    if (qhex != "-" && qual.size() != read.size()) { fprintf(stderr, "line %zu: %zu qualities for %zu bases\n", n_line, qual.size(), read.size()); return 2; }
    int64_t cols[mmep::COLS] = {0, 0, 0, 0, 0, 0};
    uint64_t key = mmep::NO_KEY;
    if (use && dist >= 0) {
      // (the sets of one job: the lengths of its read and its contig sit at its own indexes)
      std::vector<int32_t> q_len((size_t)std::max<long long>(n_reads, 0), (int32_t)read.size()), r_len((size_t)std::max<long long>(n_contigs, 0), (int32_t)contig.size());
      int64_t events = 0;
      const int rule = mmp::count_job(lanes, read_idx, n_reads, contig_idx, n_contigs, (int32_t)strand, q_len.data(), r_len.data(), first, ops.data(), (int64_t)ops.size(), &events);
      if (rule) { printf("E %d\n", rule); continue; }
      mmep::walk_job(lanes, Read{&read, &qual}, Bytes{&contig}, (int64_t)read.size(), (int32_t)strand, first, (int64_t)contig.size(), ops.data(), (int64_t)ops.size(), t, cols);
      key = mmep::ident_key(contig_idx, cols);
    }
    printf("J %lld %lld %lld %lld %lld %lld %llu\n", (long long)cols[0], (long long)cols[1], (long long)cols[2], (long long)cols[3], (long long)cols[4], (long long)cols[5],
           (unsigned long long)key);
  }
  printf("T");
  for (uint32_t k = 0; k < mmep::COUNTERS; ++k) printf(" %llu", (unsigned long long)table[k]);
  printf("\n");
  free(table);
  return 0;
}
