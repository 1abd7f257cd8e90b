// Host driver of metamaps_amd/csrc/mm_mods_core.hpp (tests/test_mods_core.py), the one-lane form of what the kernels of mm_mods.hip run.
//   plane    one read per line of stdin:  =READ n_groups { base code mode n skip*n ml*n }*n_groups  (base a letter, mode a byte value).  The groups'
//            ordinals go into ONE array of exactly the number of skips and the plane into one of exactly the read's length (a store too many is the
//            sanitizer's to see).  One line of stdout per read: who and prob as hex strings, or "E group".
//   events   one job per line:  read n_reads contig n_contigs strand first dist use read_len contig_len T PLANE n_ops op*n_ops  with PLANE four hex
//            digits per base (who, prob) or "-" for a read without a plane.  The jobs are counted, checked and emitted back to back into ONE buffer of
//            exactly the sum of their counts.  One line per job: its keys in ascending order, "-" or "E rule".
//   rows     stdin: "min_coverage code_bases n", then n lines "key count ref_byte" (the byte's value) with ascending unique keys.  stdout: one line
//            "site n_mod n_canonical n_other n_fail" per row.
#include "../metamaps_amd/csrc/mm_mods_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); } };   // (at: an index outside the read throws)
struct Calls { const std::vector<uint16_t>* v; uint16_t call(int64_t s) const { return v->at((size_t)s); } };

static int plane() {
  std::string line;
  mmp::HostLanes lanes;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string read; int n_groups = 0;
    in >> read >> n_groups;
    read.erase(0, 1);
    std::vector<uint8_t> base, mode, ml; std::vector<int8_t> code; std::vector<int64_t> soff{0}; std::vector<uint32_t> skips;
    for (int g = 0; g < n_groups; ++g) {
      char b; int c, m; size_t n;
      in >> b >> c >> m >> n;
      base.push_back((uint8_t)mmp::base_code((uint8_t)b)); code.push_back((int8_t)c); mode.push_back((uint8_t)m);
      for (size_t k = 0; k < n; ++k) { unsigned long long v; in >> v; skips.push_back((uint32_t)v); }
      for (size_t k = 0; k < n; ++k) { unsigned v; in >> v; ml.push_back((uint8_t)v); }
      soff.push_back((int64_t)skips.size());
    }
    if (!in) { fprintf(stderr, "bad line\n"); return 2; }
    // exactly as many words as there are skips and bases (malloc: the sanitizer sees the first byte beyond)
    uint32_t* const ord = (uint32_t*)malloc(sizeof(uint32_t) * std::max<size_t>(skips.size(), 1));
    uint16_t* const out = (uint16_t*)malloc(sizeof(uint16_t) * std::max<size_t>(read.size(), 1));
    for (int g = 0; g < n_groups; ++g) mmd::group_ordinals(lanes, skips.data() + soff[(size_t)g], soff[(size_t)g + 1] - soff[(size_t)g], ord + soff[(size_t)g]);
    const mmd::Groups G{base.data(), code.data(), mode.data(), soff.data(), ord, ml.data()};
    const int bad = mmd::plane_read(lanes, Bytes{&read}, (int64_t)read.size(), G, 0, n_groups, out);
    if (bad >= 0) printf("E %d\n", bad);
    else {
      for (size_t i = 0; i < read.size(); ++i) printf("%02x", out[i] & 255u);
      printf(" ");
      for (size_t i = 0; i < read.size(); ++i) printf("%02x", out[i] >> 8);
      printf("\n");
    }
    free(ord); free(out);
  }
  return 0;
}

struct Job {
  std::vector<uint32_t> ops; std::vector<uint16_t> calls; bool has_plane = false;
  long long read_idx, n_reads, contig_idx, n_contigs, strand, first, dist, use, read_len, contig_len, T;
  int rule = 0; int64_t events = 0;
};

static int events() {
  std::vector<Job> js;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Job j; size_t n_ops = 0; std::string pl;
    in >> j.read_idx >> j.n_reads >> j.contig_idx >> j.n_contigs >> j.strand >> j.first >> j.dist >> j.use >> j.read_len >> j.contig_len >> j.T >> pl >> n_ops;
    j.has_plane = pl != "-";
    j.calls.assign((size_t)j.read_len, 0);
    if (j.has_plane)
      for (size_t i = 0; i < (size_t)j.read_len; ++i) {
        const unsigned v = (unsigned)std::stoul(pl.substr(4 * i, 4), nullptr, 16);
        j.calls[i] = (uint16_t)((v >> 8) | (v & 255u) << 8);       // (who first in the text, in the low byte of the word)
      }
    j.ops.resize(n_ops);
    for (auto& w : j.ops) in >> w;
    if (!in) { fprintf(stderr, "bad line %zu\n", js.size()); return 2; }
    js.push_back(std::move(j));
  }
  mmp::HostLanes lanes;
  int64_t total = 0;
  for (auto& j : js) {
    if (!j.use || j.dist < 0) continue;
    std::vector<int32_t> q_len((size_t)std::max<long long>(j.n_reads, 0), (int32_t)j.read_len), r_len((size_t)std::max<long long>(j.n_contigs, 0), (int32_t)j.contig_len);
    int64_t unused = 0;
    j.rule = mmp::count_job(lanes, j.read_idx, j.n_reads, j.contig_idx, j.n_contigs, (int32_t)j.strand, q_len.data(), r_len.data(), j.first, j.ops.data(), (int64_t)j.ops.size(), &unused);
    if (!j.rule && j.has_plane)
      j.events = mmd::walk_job(lanes, Calls{&j.calls}, j.read_len, (int32_t)j.strand, j.contig_idx, j.first, j.ops.data(), (int64_t)j.ops.size(), (int32_t)j.T, nullptr);
    total += j.events;
  }
  uint64_t* const buf = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(total + (total == 0)));
  int64_t at = 0;
  for (auto& j : js) {
    if (j.rule || !j.events) continue;
    const int64_t wrote = mmd::walk_job(lanes, Calls{&j.calls}, j.read_len, (int32_t)j.strand, j.contig_idx, j.first, j.ops.data(), (int64_t)j.ops.size(), (int32_t)j.T, buf + at);
    if (wrote != j.events) { fprintf(stderr, "the number of events changed between the two passes\n"); return 3; }
    at += j.events;
  }
  at = 0;
  for (auto& j : js) {                                             // (after every job is emitted: one that ran over its end has damaged the next)
    if (j.rule) { printf("E %d\n", j.rule); continue; }
    if (!j.events) { printf("-\n"); continue; }
    std::sort(buf + at, buf + at + j.events);
    for (int64_t i = 0; i < j.events; ++i) printf("%s%llu", i ? " " : "", (unsigned long long)buf[at + i]);
    printf("\n");
    at += j.events;
  }
  free(buf);
  return 0;
}

static int rows() {
  long long min_cov, n; std::string bases;
  if (!(std::cin >> min_cov >> bases >> n)) return 2;
  std::vector<uint64_t> keys((size_t)n); std::vector<uint32_t> counts((size_t)n); std::vector<unsigned> ref((size_t)n);
  for (long long i = 0; i < n; ++i) std::cin >> keys[(size_t)i] >> counts[(size_t)i] >> ref[(size_t)i];
  if (!std::cin) return 2;
  mmd::CodeBases cb{};
  cb.n = (int)bases.size();
  for (int k = 0; k < cb.n; ++k) cb.b[k] = (uint8_t)bases[(size_t)k];
  for (long long i = 0; i < n; ++i) {
    if (i > 0 && mmd::key_site(keys[(size_t)i]) == mmd::key_site(keys[(size_t)i - 1])) continue;
    mmd::Row out[mmd::MAX_CODES];
    const int k = mmd::segment_rows(keys.data(), counts.data(), i, n, (uint8_t)ref[(size_t)i], cb, min_cov, out);
    if (k != mmd::segment_rows(keys.data(), counts.data(), i, n, (uint8_t)ref[(size_t)i], cb, min_cov, nullptr)) { fprintf(stderr, "the counting pass disagrees\n"); return 3; }
    for (int t = 0; t < k; ++t)
      printf("%llu %llu %llu %llu %llu\n", (unsigned long long)out[t].site, (unsigned long long)out[t].n_mod, (unsigned long long)out[t].n_canonical, (unsigned long long)out[t].n_other,
             (unsigned long long)out[t].n_fail);
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "plane") return plane();
  if (mode == "events") return events();
  if (mode == "rows") return rows();
  fprintf(stderr, "usage: test_mods_core plane|events|rows < input\n");
  return 2;
}
