// Host driver of metamaps_amd/csrc/mm_pileup_core.hpp (tests/test_pileup_core.py), the one-lane form of what the kernels of mm_pileup.hip run.
//   events   the jobs of stdin, one per line
//              read n_reads contig n_contigs strand first dist use =READ contig_len n_ops op...
//            are counted, checked and emitted back to back into ONE buffer of exactly the sum of their counts, as the kernels do (a key too many is the
//            sanitizer's to see).  One line of stdout per job: its keys in the order of the walk, "-" (no event, or a job that does not contribute) or
//            "E rule".
//   finish   stdin: "min_count min_frac n_contigs n n_iv", then n lines "key count", then n_iv lines "contig first last".  The starts and ends are sorted
//            here; depth_at, site_kept and covered_gain do the rest.  stdout: "S key count depth" per kept site, then "C alignments covered sum_depth"
//            per contig.
#include "../metamaps_amd/csrc/mm_pileup_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); } };   // (at: a read index outside the read throws)
struct Job {
  std::string read; std::vector<uint32_t> ops;
  long long read_idx, n_reads, contig_idx, n_contigs, strand, first, dist, use, contig_len;
  int rule = 0; int64_t events = 0;
};

static int events() {
  std::vector<Job> js;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Job j; size_t n_ops = 0;
    in >> j.read_idx >> j.n_reads >> j.contig_idx >> j.n_contigs >> j.strand >> j.first >> j.dist >> j.use >> j.read >> j.contig_len >> n_ops;
    j.read.erase(0, 1);
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
    std::vector<int32_t> q_len((size_t)std::max<long long>(j.n_reads, 0), (int32_t)j.read.size()), r_len((size_t)std::max<long long>(j.n_contigs, 0), (int32_t)j.contig_len);
    j.rule = mmp::count_job(lanes, j.read_idx, j.n_reads, j.contig_idx, j.n_contigs, (int32_t)j.strand, q_len.data(), r_len.data(), j.first, j.ops.data(), (int64_t)j.ops.size(), &j.events);
    if (!j.rule) total += j.events;
  }
  uint64_t* const buf = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(total + (total == 0)));
  int64_t at = 0;
  for (auto& j : js) {
    if (j.rule || !j.events) continue;
    const int64_t wrote = mmp::emit_job(lanes, Bytes{&j.read}, (int64_t)j.read.size(), (int32_t)j.strand, j.contig_idx, j.first, j.ops.data(), (int64_t)j.ops.size(), buf + at);
    if (wrote != j.events) { fprintf(stderr, "the number of events changed between the two passes\n"); return 3; }
    at += j.events;
  }
  at = 0;
  for (auto& j : js) {                                             // (after every job is emitted: one that ran over its end has damaged the next)
    if (j.rule) { printf("E %d\n", j.rule); continue; }
    if (!j.events) { printf("-\n"); continue; }
    for (int64_t i = 0; i < j.events; ++i) printf("%s%llu", i ? " " : "", (unsigned long long)buf[at + i]);
    printf("\n");
    at += j.events;
  }
  free(buf);
  return 0;
}

static int finish() {
  long long min_count, n_contigs, n, n_iv; double min_frac;
  if (!(std::cin >> min_count >> min_frac >> n_contigs >> n >> n_iv)) return 2;
  std::vector<uint64_t> keys((size_t)n), starts, ends; std::vector<uint32_t> counts((size_t)n);
  for (long long i = 0; i < n; ++i) std::cin >> keys[(size_t)i] >> counts[(size_t)i];
  std::vector<std::pair<uint64_t, uint64_t>> iv;
  for (long long i = 0; i < n_iv; ++i) { long long c, a, b; std::cin >> c >> a >> b; iv.emplace_back(mmp::interval_key(c, a), mmp::interval_key(c, b)); }
  if (!std::cin) return 2;
  std::sort(iv.begin(), iv.end());
  for (auto& x : iv) { starts.push_back(x.first); ends.push_back(x.second); }
  std::sort(ends.begin(), ends.end());
  for (long long i = 0; i < n; ++i) {
    const int64_t d = mmp::depth_at(starts.data(), ends.data(), n_iv, mmp::key_contig(keys[(size_t)i]), mmp::key_pos(keys[(size_t)i]));
    if (mmp::site_kept(counts[(size_t)i], d, min_count, min_frac)) printf("S %llu %u %lld\n", (unsigned long long)keys[(size_t)i], counts[(size_t)i], (long long)d);
  }
  std::vector<long long> al((size_t)n_contigs, 0), cov((size_t)n_contigs, 0), sum((size_t)n_contigs, 0);
  uint64_t pmax = 0;
  for (size_t i = 0; i < iv.size(); ++i) {
    const size_t c = (size_t)(iv[i].first >> 32);
    al[c] += 1; sum[c] += (long long)(iv[i].second - iv[i].first + 1); cov[c] += mmp::covered_gain(iv[i].first, iv[i].second, i > 0, pmax);
    pmax = std::max(pmax, iv[i].second);
  }
  for (long long c = 0; c < n_contigs; ++c) printf("C %lld %lld %lld\n", al[(size_t)c], cov[(size_t)c], sum[(size_t)c]);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "events") return events();
  if (mode == "finish") return finish();
  fprintf(stderr, "usage: test_pileup_core events|finish < input\n");
  return 2;
}
