// mapDirectly --consensus [--consensus-min-depth D] [--consensus-min-frac F] [--consensus-min-called C] (implies --edit-distance; not in the reference):
// PREFIX.consensus.fa and PREFIX.consensus.tsv, the sequence of the strain the reads come from, built on the device from the alleles --vcf accumulates and the
// intervals of the primary alignments (the definition: csrc/mm_cons_core.hpp).  Both are plain text whatever --compress-output says; an empty run writes an
// empty .fa and the header of the .tsv alone.
//   PREFIX.consensus.fa   the written contigs in the reference's order: ">contigID" and the consensus in lines of 60 columns.  A position holds the majority
//                         allele where at least D (default 3) primary alignments span it and F (default 0.5) of them carry the allele, the reference's base
//                         where D span it and no allele is applied, and N elsewhere; a contig is written where at least max(1, ceil(C * length)) positions
//                         (C default 0) are spanned by D.
//   PREFIX.consensus.tsv  a header line and one line per contig with a primary alignment: contigID length alignments called written consensusLength snvs
//                         deletions deletedBases insertions insertedBases dropped
//   groups                mm_consensus takes a range of contigs at a time: consecutive contigs from one with an alignment on whose lengths add up to at most
//                         MM_CONS_GROUP_BASES (2^28); a longer contig is a group alone.  Contigs without an alignment at a group's end are left out of it.
// Text, arrays and the option values only: nothing here calls the device.
#pragma once
#include "../mm_cons_core.hpp"
#include "pileup_out.hpp"
#include <numeric>

namespace {

constexpr int CONS_LINE_WIDTH = 60;

// the three thresholds: validated before any work; refused without --consensus
struct ConsOpts { bool on = false; long long min_depth = 3; double min_frac = 0.5, min_called = 0.0; };
ConsOpts consensus_options(const Options& o) {
  ConsOpts p;
  p.on = o.v.count("consensus") != 0;
  auto decimal_of = [&](const char* name, double lo, const char* range, double* out) {
    if (!o.v.count(name)) return;
    const std::string& v = o.v.at(name);
    if (!p.on) die(std::string("--") + name + " needs --consensus");
    const DecimalValue x = decimal_value(v);
    if (!x.ok || !(x.value >= lo && x.value <= 1.0)) die(std::string("--consensus: --") + name + " takes a decimal from " + range + " to 1, not '" + v + "'");
    *out = x.value;
  };
  if (o.v.count("consensus-min-depth")) {
    const std::string& v = o.v.at("consensus-min-depth");
    if (!p.on) die("--consensus-min-depth needs --consensus");
    const IntegerValue x = integer_value(v, 9);
    if (!x.ok || x.value < 1) die("--consensus: --consensus-min-depth takes an integer from 1 to 999999999, not '" + v + "'");
    p.min_depth = (long long)x.value;
  }
  decimal_of("consensus-min-frac", 0.5, "0.5", &p.min_frac);
  decimal_of("consensus-min-called", 0.0, "0", &p.min_called);
  return p;
}

// the order that puts a file's intervals in contig order (stable: equal contigs keep theirs)
std::vector<size_t> cons_interval_order(const std::vector<int32_t>& contig) {
  std::vector<size_t> idx(contig.size());
  std::iota(idx.begin(), idx.end(), (size_t)0);
  std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return contig[a] < contig[b]; });
  return idx;
}
// The groups [lo, hi) of contigs, from the ascending contigs of the intervals: every contig with an interval lies in exactly one group, a group starts and ends
// at one, and the lengths of its contigs (those without an interval between them included) add up to at most max_bases unless it is one contig.
struct ConsGroupRange { int32_t lo, hi; };
std::vector<ConsGroupRange> cons_groups(const std::vector<int>& clen, const std::vector<int32_t>& sorted_contig, int64_t max_bases) {
  std::vector<ConsGroupRange> out;
  size_t i = 0;
  while (i < sorted_contig.size()) {
    const int32_t lo = sorted_contig[i];
    int32_t last = lo;                                             // the last contig the group holds
    int64_t bases = clen[(size_t)lo];                              // of [lo, last]
    for (++i; i < sorted_contig.size(); ++i) {
      const int32_t c = sorted_contig[i];
      if (c == last) continue;
      int64_t more = 0;
      for (int32_t k = last + 1; k <= c; ++k) more += clen[(size_t)k];
      if (bases + more > max_bases) break;
      bases += more; last = c;
    }
    out.push_back(ConsGroupRange{lo, last + 1});
  }
  return out;
}

std::string cons_fasta_name(const std::string& contig_id) { return ">" + contig_id + "\n"; }
std::string cons_tsv_header() {
  return "contigID\tlength\talignments\tcalled\twritten\tconsensusLength\tsnvs\tdeletions\tdeletedBases\tinsertions\tinsertedBases\tdropped\n";
}
// stats: mmc::STATS counters, in the columns' order
void cons_tsv_row(const std::string& contig_id, int len, const int64_t* stats, std::string& t) {
  t += contig_id; t += '\t'; append_int(t, len);
  for (int k = 0; k < mmc::STATS; ++k) { t += '\t'; append_int(t, (long long)stats[k]); }
  t += '\n';
}

}  // namespace
