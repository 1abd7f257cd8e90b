// Host driver of the quality floor of metamaps_amd/csrc/mm_pileup_core.hpp and mm_vcf_core.hpp and of the QUAL field of mm_bam_core.hpp
// (tests/test_qual_core.py), the one-lane form of what the kernels of mm_pileup.hip, mm_vcf.hip and mm_bam.hip run.
//   pileup FLOOR | vcf FLOOR   the jobs of stdin, one per line
//                                read n_reads contig n_contigs strand first dist use =READ QUAL =CONTIG n_ops op...
//                              (QUAL: the stored Phred bytes in hexadecimal, "-" for a read without) are counted, checked and emitted back to back into
//                              ONE buffer of exactly the sum of their counts, as the kernels do.  One line of stdout per job: its kept keys (pileup) or
//                              kept alleles "w0:w1" (vcf) in the order of the walk, "-" for none or "E rule".  With FLOOR 0 every job is also emitted
//                              by the walk without a floor (emit_job), and a difference between the two ends the program with status 3.
//   qual                       stdin: lines "strand first =READ QUAL =CONTIG n_ops op..."; the record of write_record_q and that of write_record (no
//                              qualities: QUAL all 0xFF).  stdout: the former's QUAL in hexadecimal, then "same" if every other byte of the two agrees
#include "../metamaps_amd/csrc/mm_vcf_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); } };   // (at: an index outside the sequence throws)
struct Quals {                                                     // bytes and stored qualities; has == false: a read without
  const std::string* s; const std::vector<uint8_t>* q; bool has;
  uint8_t byte(int64_t i) const { return (uint8_t)s->at((size_t)i); }
  uint8_t qual(int64_t i) const { return has ? q->at((size_t)i) : mmb::QUAL_NONE; }
};
struct Job {
  std::string read, contig, qhex; std::vector<uint8_t> qual; std::vector<uint32_t> ops;
  long long read_idx, n_reads, contig_idx, n_contigs, strand, first, dist, use;
  int rule = 0; int64_t places = 0, indels = 0;
};

static bool unhex(const std::string& h, std::vector<uint8_t>* out) {
  if (h == "-") return false;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out->push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return true;
}

static int events(bool vcf, int32_t floor) {
  std::vector<Job> js;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Job j; size_t n_ops = 0;
    in >> j.read_idx >> j.n_reads >> j.contig_idx >> j.n_contigs >> j.strand >> j.first >> j.dist >> j.use >> j.read >> j.qhex >> j.contig >> n_ops;
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
    std::vector<int32_t> q_len((size_t)std::max<long long>(j.n_reads, 0), (int32_t)j.read.size()), r_len((size_t)std::max<long long>(j.n_contigs, 0), (int32_t)j.contig.size());
    if (vcf) j.rule = mmv::count_job(lanes, j.read_idx, j.n_reads, j.contig_idx, j.n_contigs, (int32_t)j.strand, q_len.data(), r_len.data(), j.first, j.ops.data(), (int64_t)j.ops.size(), &j.places, &j.indels);
    else j.rule = mmp::count_job(lanes, j.read_idx, j.n_reads, j.contig_idx, j.n_contigs, (int32_t)j.strand, q_len.data(), r_len.data(), j.first, j.ops.data(), (int64_t)j.ops.size(), &j.places);
    if (!j.rule) total += j.places;
  }
  const size_t cap = (size_t)(total + (total == 0));
  uint64_t* const w0 = (uint64_t*)malloc(sizeof(uint64_t) * cap);
  uint64_t* const w1 = (uint64_t*)malloc(sizeof(uint64_t) * cap);
  uint64_t* const p0 = (uint64_t*)malloc(sizeof(uint64_t) * cap);  // the walk without a floor
  uint64_t* const p1 = (uint64_t*)malloc(sizeof(uint64_t) * cap);
  int64_t at = 0;
  for (auto& j : js) {
    if (j.rule || !j.places) continue;
    const bool has = unhex(j.qhex, &j.qual);
    if (has && j.qual.size() != j.read.size()) { fprintf(stderr, "a quality string of another length than its read\n"); return 2; }
    const Quals q{&j.read, &j.qual, has};
    const int64_t m = (int64_t)j.read.size(), n_ops = (int64_t)j.ops.size();
    const int64_t wrote = vcf ? mmv::emit_job_q(lanes, q, m, (int32_t)j.strand, Bytes{&j.contig}, j.contig_idx, j.first, j.ops.data(), n_ops, floor, w0 + at, w1 + at)
                              : mmp::emit_job_q(lanes, q, m, (int32_t)j.strand, j.contig_idx, j.first, j.ops.data(), n_ops, floor, w0 + at);
    if (wrote != j.places) { fprintf(stderr, "the number of places changed between the two passes\n"); return 3; }
    if (floor == 0) {
      const int64_t plain = vcf ? mmv::emit_job(lanes, Bytes{&j.read}, m, (int32_t)j.strand, Bytes{&j.contig}, j.contig_idx, j.first, j.ops.data(), n_ops, p0 + at, p1 + at)
                                : mmp::emit_job(lanes, Bytes{&j.read}, m, (int32_t)j.strand, j.contig_idx, j.first, j.ops.data(), n_ops, p0 + at);
      if (plain != wrote || memcmp(p0 + at, w0 + at, sizeof(uint64_t) * (size_t)wrote) || (vcf && memcmp(p1 + at, w1 + at, sizeof(uint64_t) * (size_t)wrote))) {
        fprintf(stderr, "floor 0 differs from the walk without a floor\n"); return 3;
      }
    }
    at += j.places;
  }
  at = 0;
  for (auto& j : js) {                                             // (after every job is emitted: one that ran over its end has damaged the next)
    if (j.rule) { printf("E %d\n", j.rule); continue; }
    int64_t shown = 0;
    for (int64_t i = 0; i < j.places; ++i) {
      const uint64_t a = w0[at + i];
      if (vcf) {
        const uint64_t b = w1[at + i];
        if ((a == mmv::SKIP) != (b == mmv::SKIP)) { fprintf(stderr, "half a skipped pair\n"); return 3; }
        if (a == mmv::SKIP) continue;
        if (!mmv::key_valid(a, b, (int64_t)j.contig.size())) { fprintf(stderr, "an emitted key is not valid\n"); return 3; }
        printf("%s%llu:%llu", shown++ ? " " : "", (unsigned long long)a, (unsigned long long)b);
      } else {
        if (a == mmp::DROPPED) continue;
        if (mmp::key_code(a) >= mmp::N_CODES) { fprintf(stderr, "an emitted key has no code\n"); return 3; }
        printf("%s%llu", shown++ ? " " : "", (unsigned long long)a);
      }
    }
    printf(shown ? "\n" : "-\n");
    at += j.places;
  }
  free(w0); free(w1); free(p0); free(p1);
  return 0;
}

static int qual() {
  std::string line;
  mmb::HostLanes lanes;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    long long strand, first; std::string read, contig, hex; size_t n_ops = 0;
    in >> strand >> first >> read >> hex >> contig >> n_ops;
    read.erase(0, 1); contig.erase(0, 1);
    std::vector<uint32_t> ops(n_ops);
    for (auto& w : ops) in >> w;
    if (!in) { fprintf(stderr, "bad line\n"); return 2; }
    std::vector<uint8_t> q;
    const bool has = unhex(hex, &q);
    const int64_t m = (int64_t)read.size();
    mmb::Job j;
    j.ops = ops.data(); j.n_ops = (int64_t)n_ops; j.name = "r"; j.l_name = 1; j.first = first; j.m = (int32_t)m; j.refid = 0; j.strand = (int32_t)strand;
    j.flag = strand < 0 ? 0x10 : 0; j.mapq = 9;
    const mmb::Walk w = mmb::md_walk<false>(lanes, Bytes{&contig}, j.ops, j.n_ops, j.first, nullptr);
    j.dist = (int32_t)w.edits;
    const int64_t size = mmb::record_size(j.l_name, m, j.n_ops, w.md_len);
    std::vector<uint8_t> with((size_t)size, 0xAA), without((size_t)size, 0xAA);
    const mmb::QualBytes src{(const uint8_t*)read.data(), has ? q.data() : nullptr};
    if (mmb::write_record_q(lanes, j, src, Bytes{&contig}, with.data()) != size || mmb::write_record(lanes, j, Bytes{&read}, Bytes{&contig}, without.data()) != size) {
      fprintf(stderr, "a record of another size than record_size gave\n"); return 3;
    }
    const size_t at = mmb::FIXED + (size_t)j.l_name + 1 + 4 * n_ops + (size_t)(m + 1) / 2;
    for (int64_t i = 0; i < m; ++i) { printf("%02x", with[at + (size_t)i]); if (without[at + (size_t)i] != 0xFF) { fprintf(stderr, "QUAL of a read without qualities is not 0xFF\n"); return 3; } }
    memset(with.data() + at, 0xFF, (size_t)m);
    printf(with == without ? " same\n" : " differs\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if ((mode == "pileup" || mode == "vcf") && argc > 2) return events(mode == "vcf", (int32_t)atoi(argv[2]));
  if (mode == "qual") return qual();
  fprintf(stderr, "usage: test_qual_core pileup FLOOR | vcf FLOOR | qual < input\n");
  return 2;
}
