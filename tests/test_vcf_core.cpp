// Host driver of metamaps_amd/csrc/mm_vcf_core.hpp (tests/test_vcf_core.py), the one-lane form of what the kernels of mm_vcf.hip run.
//   events   the jobs of stdin, one per line
//              read n_reads contig n_contigs strand first dist use =READ =CONTIG n_ops op...
//            are counted, checked and emitted back to back into ONE pair of buffers of exactly the sum of their bounds, as the kernels do (an allele too
//            many is the sanitizer's to see).  One line of stdout per job: its alleles "w0:w1" in the order of the walk with "skip" for the all-ones
//            pair, "-" (no event, or a job that does not contribute) or "E rule".
//   finish   stdin: "min_count min_frac n_contigs n n_iv", then n_contigs lines "=CONTIG", n lines "w0 w1 count", n_iv lines "contig first last".  The
//            starts and ends are sorted here; key_valid, depth_at, site_kept and window_len do the rest.  stdout: "A w0 w1 count depth WINDOW" per kept
//            allele, the window in hexadecimal; an entry that is no valid key ends the program with status 4.
#include "../metamaps_amd/csrc/mm_vcf_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); } };   // (at: an index outside the sequence throws)
struct Job {
  std::string read, contig; std::vector<uint32_t> ops;
  long long read_idx, n_reads, contig_idx, n_contigs, strand, first, dist, use;
  int rule = 0; int64_t alleles = 0, indels = 0;
};

static int events() {
  std::vector<Job> js;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Job j; size_t n_ops = 0;
    in >> j.read_idx >> j.n_reads >> j.contig_idx >> j.n_contigs >> j.strand >> j.first >> j.dist >> j.use >> j.read >> j.contig >> n_ops;
    j.read.erase(0, 1); j.contig.erase(0, 1);
    j.ops.resize(n_ops);
    for (auto& w : j.ops) in >> w;
    if (!in) { fprintf(stderr, "bad line %zu\n", js.size()); return 2; }
    js.push_back(std::move(j));
  }
  mmp::HostLanes lanes;
  int64_t total = 0;
  for (auto& j : js) {
    if (!j.use || j.dist < 0) continue;
    // (the sets of one job: the lengths of its read and its contig sit at its own indexes)
    std::vector<int32_t> q_len((size_t)std::max<long long>(j.n_reads, 0), (int32_t)j.read.size()), r_len((size_t)std::max<long long>(j.n_contigs, 0), (int32_t)j.contig.size());
    j.rule = mmv::count_job(lanes, j.read_idx, j.n_reads, j.contig_idx, j.n_contigs, (int32_t)j.strand, q_len.data(), r_len.data(), j.first, j.ops.data(), (int64_t)j.ops.size(), &j.alleles,
                            &j.indels);
    if (!j.rule) total += j.alleles;
  }
  uint64_t* const w0 = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(total + (total == 0)));
  uint64_t* const w1 = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(total + (total == 0)));
  int64_t at = 0;
  for (auto& j : js) {
    if (j.rule || !j.alleles) continue;
    const int64_t wrote = mmv::emit_job(lanes, Bytes{&j.read}, (int64_t)j.read.size(), (int32_t)j.strand, Bytes{&j.contig}, j.contig_idx, j.first, j.ops.data(), (int64_t)j.ops.size(),
                                        w0 + at, w1 + at);
    if (wrote != j.alleles) { fprintf(stderr, "the number of alleles changed between the two passes\n"); return 3; }
    at += j.alleles;
  }
  at = 0;
  for (auto& j : js) {                                             // (after every job is emitted: one that ran over its end has damaged the next)
    if (j.rule) { printf("E %d\n", j.rule); continue; }
    if (!j.alleles) { printf("-\n"); continue; }
    int64_t indels = 0;
    for (int64_t i = 0; i < j.alleles; ++i) {
      const uint64_t a = w0[at + i], b = w1[at + i];
      if ((a == mmv::SKIP) != (b == mmv::SKIP)) { fprintf(stderr, "half a skipped pair\n"); return 3; }
      if (a == mmv::SKIP) printf("%sskip", i ? " " : "");
      else printf("%s%llu:%llu", i ? " " : "", (unsigned long long)a, (unsigned long long)b);
      if (a != mmv::SKIP && !mmv::key_valid(a, b, (int64_t)j.contig.size())) { fprintf(stderr, "an emitted key is not valid\n"); return 3; }
      indels += a != mmv::SKIP && mmp::key_code(a) >= mmp::CODE_DEL;
    }
    if (indels > j.indels) { fprintf(stderr, "more indel alleles than count_job announced\n"); return 3; }
    printf("\n");
    at += j.alleles;
  }
  free(w0); free(w1);
  return 0;
}

static int finish() {
  long long min_count, n_contigs, n, n_iv; double min_frac;
  if (!(std::cin >> min_count >> min_frac >> n_contigs >> n >> n_iv)) return 2;
  std::vector<std::string> contigs((size_t)n_contigs);
  for (auto& c : contigs) { std::cin >> c; c.erase(0, 1); }
  std::vector<uint64_t> w0((size_t)n), w1((size_t)n), starts, ends; std::vector<uint32_t> counts((size_t)n);
  for (long long i = 0; i < n; ++i) std::cin >> w0[(size_t)i] >> w1[(size_t)i] >> counts[(size_t)i];
  std::vector<std::pair<uint64_t, uint64_t>> iv;
  for (long long i = 0; i < n_iv; ++i) { long long c, a, b; std::cin >> c >> a >> b; iv.emplace_back(mmp::interval_key(c, a), mmp::interval_key(c, b)); }
  if (!std::cin) return 2;
  std::sort(iv.begin(), iv.end());
  for (auto& x : iv) { starts.push_back(x.first); ends.push_back(x.second); }
  std::sort(ends.begin(), ends.end());
  for (size_t i = 0; i < (size_t)n; ++i) {
    const int64_t c = mmp::key_contig(w0[i]), pos = mmp::key_pos(w0[i]);
    if (c >= n_contigs || !mmv::key_valid(w0[i], w1[i], (int64_t)contigs[(size_t)c].size())) return 4;
    const int64_t d = mmp::depth_at(starts.data(), ends.data(), n_iv, c, pos);
    if (!mmp::site_kept(counts[i], d, min_count, min_frac)) continue;
    printf("A %llu %llu %u %lld ", (unsigned long long)w0[i], (unsigned long long)w1[i], counts[i], (long long)d);
    const int64_t len = mmv::window_len(pos, (int64_t)contigs[(size_t)c].size());
    for (int64_t t = 0; t < mmv::WINDOW; ++t) printf("%02x", t < len ? (unsigned)mmb::upper((uint8_t)contigs[(size_t)c].at((size_t)(pos + t))) : 0u);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "events") return events();
  if (mode == "finish") return finish();
  fprintf(stderr, "usage: test_vcf_core events|finish < input\n");
  return 2;
}
