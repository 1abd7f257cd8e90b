// Host driver of metamaps_amd/csrc/mm_bam_core.hpp (tests/test_bam_core.py): the problems of stdin, one per line
//   =NAME read n_reads contig n_contigs strand first dist flag mapq =READ =CONTIG n_ops op...
// are sized, checked and written back to back into ONE buffer of exactly the sum of their sizes, as the kernels do (so records start at any byte
// offset and a byte too many is the sanitizer's to see).  One line of stdout per problem: the record in hex, "-" (no record: dist < 0 or an empty
// read) or "E rule".
#include "../metamaps_amd/csrc/mm_bam_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)(*s)[(size_t)i]; } };
struct Problem {
  std::string name, read, contig; std::vector<uint32_t> ops;
  long long read_idx, n_reads, contig_idx, n_contigs, strand, first, dist, flag, mapq;
  int rule = 0; int64_t size = 0;
};

int main() {
  std::vector<Problem> ps;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Problem p; size_t n_ops = 0;
    in >> p.name >> p.read_idx >> p.n_reads >> p.contig_idx >> p.n_contigs >> p.strand >> p.first >> p.dist >> p.flag >> p.mapq >> p.read >> p.contig >> n_ops;
    p.name.erase(0, 1); p.read.erase(0, 1); p.contig.erase(0, 1);
    p.ops.resize(n_ops);
    for (auto& w : p.ops) in >> w;
    if (!in) { fprintf(stderr, "bad line %zu\n", ps.size()); return 2; }
    ps.push_back(std::move(p));
  }
  mmb::HostLanes lanes;
  int64_t total = 0;
  for (auto& p : ps) {
    p.rule = mmb::check_set(p.read_idx, p.n_reads, p.contig_idx, p.n_contigs);
    if (p.rule || p.dist < 0 || p.read.empty()) continue;
    p.rule = mmb::check_head((int32_t)p.strand, (uint32_t)p.flag, (int64_t)p.name.size());
    if (p.rule) continue;
    const mmb::Walk w = mmb::md_walk<false>(lanes, Bytes{&p.contig}, p.ops.data(), (int64_t)p.ops.size(), p.first, nullptr);
    p.rule = mmb::check_walk(w, (int64_t)p.read.size(), p.first, (int64_t)p.contig.size(), p.dist);
    if (!p.rule) { p.size = mmb::record_size((int64_t)p.name.size(), (int64_t)p.read.size(), (int64_t)p.ops.size(), w.md_len); total += p.size; }
  }
  uint8_t* const buf = (uint8_t*)malloc((size_t)total + (total == 0));
  int64_t at = 0;
  for (auto& p : ps) {
    if (p.rule || !p.size) continue;
    const mmb::Job j{p.ops.data(), (int64_t)p.ops.size(), p.name.data(), (int32_t)p.name.size(), p.first, (int32_t)p.read.size(), (int32_t)p.contig_idx, (int32_t)p.strand,
                     (int32_t)p.dist, (uint16_t)p.flag, (uint8_t)p.mapq};
    const int64_t wrote = mmb::write_record(lanes, j, Bytes{&p.read}, Bytes{&p.contig}, buf + at);
    if (wrote != p.size) { fprintf(stderr, "the record's size changed between the two passes\n"); return 3; }
    at += p.size;
  }
  at = 0;
  std::string hex;
  for (auto& p : ps) {                                           // (after every record is written: one that ran over its end has damaged the next)
    if (p.rule) { printf("E %d\n", p.rule); continue; }
    if (!p.size) { printf("-\n"); continue; }
    hex.clear();
    for (int64_t i = 0; i < p.size; ++i) { static const char H[] = "0123456789abcdef"; hex += H[buf[at + i] >> 4]; hex += H[buf[at + i] & 15]; }
    puts(hex.c_str());
    at += p.size;
  }
  free(buf);
  return 0;
}
