// mapDirectly --error-profile (implies --edit-distance; not in the reference): PREFIX.errorProfile.substitutions, .indels, .qualities and .contigs, what the
// PRIMARY alignments of the run say about the reads and about the distance between the sample and the database genomes (the definition:
// csrc/mm_errprof_core.hpp; one mm_errprof_events call per batch on the device that mapped it, one mm_errprof_finish per query file on the first device).
// All four are plain text whatever --compress-output says; an empty run writes the headers alone.
//   PREFIX.errorProfile.substitutions  #truth A C G T N, then the rows A .. N: how often the sequencer wrote the column's letter where the reference (in the
//                                      read's orientation) has the row's; = and X columns alike, so the diagonal holds the matches
//   PREFIX.errorProfile.indels         #kind length homopolymer other: one row per kind (I, then D) and length with a count; the last bin prints as 64+
//   PREFIX.errorProfile.qualities      #quality matches mismatches inserted errorRate empiricalQ: one row per reported quality with a base, ascending, then `none`
//                                      for the bases without (all of them without --base-qualities); errorRate = (mismatches + inserted) / total as %.6f,
//                                      empiricalQ = -10 log10(errorRate) as %.2f, inf at rate 0
//   PREFIX.errorProfile.contigs        a # header, per contig with a primary alignment (the reference's order) contigID length alignments readBases refBases
//                                      matches mismatches insertions insertedBases deletions deletedBases identity gapCompressedIdentity minIdentity q1Identity
//                                      medianIdentity q3Identity maxIdentity, and a last row * over all alignments with the listed contigs' summed length;
//                                      identity = matches / (matches + mismatches + insertedBases + deletedBases), the gap-compressed one counts an indel run
//                                      once; the five order statistics are per-alignment identities (ppm / 10^6); all seven %.6f
// Text and arrays only (the flag itself is OutputPlan's, output_plan.hpp): nothing here calls the device.
#pragma once
#include "../mm_errprof_core.hpp"
#include "cli_common.hpp"
#include "fast_format.hpp"
#include <cmath>
#include <cstdio>
#include <mutex>

namespace {

// what the batches of one query file leave behind: the counters' sums and (key, six columns) of every contributing alignment
struct ErrprofAcc {
  std::mutex m;
  uint64_t counters[mmep::COUNTERS] = {};
  std::vector<uint64_t> key; std::vector<int32_t> cols;
  void add(const uint64_t* c, const std::vector<uint64_t>& k, const std::vector<int32_t>& six) {
    std::lock_guard<std::mutex> lk(m);
    for (uint32_t i = 0; i < mmep::COUNTERS; ++i) counters[i] += c[i];
    for (size_t i = 0; i < k.size(); ++i)
      if (k[i] != mmep::NO_KEY) { key.push_back(k[i]); cols.insert(cols.end(), six.begin() + (long)(i * mmep::COLS), six.begin() + (long)((i + 1) * mmep::COLS)); }
  }
};

void errprof_append_fixed(std::string& t, double x, int digits) {
  char buf[64];
  t.append(buf, (size_t)snprintf(buf, sizeof buf, "%.*f", digits, x));
}
std::string errprof_substitutions_text(const uint64_t* c) {
  std::string t = "#truth\tA\tC\tG\tT\tN\n";
  uint64_t columns = 0;
  for (uint32_t k = 0; k < mmep::N_SUB; ++k) columns += c[mmep::SUB + k];
  for (uint32_t a = 0; columns && a < 5; ++a) {                    // (an empty run: the header alone)
    t += "ACGTN"[a];
    for (uint32_t b = 0; b < 5; ++b) { t += '\t'; append_int(t, (long long)c[mmep::sub_at(a, b)]); }
    t += '\n';
  }
  return t;
}
std::string errprof_indels_text(const uint64_t* c) {
  std::string t = "#kind\tlength\thomopolymer\tother\n";
  for (uint32_t kind = 0; kind < 2; ++kind)
    for (int64_t n = 1; n <= (int64_t)mmep::BINS; ++n) {
      const uint64_t hp = c[mmep::indel_at(kind, true, n)], other = c[mmep::indel_at(kind, false, n)];
      if (!hp && !other) continue;
      t += kind ? 'D' : 'I'; t += '\t'; append_int(t, (long long)n); if (n == (int64_t)mmep::BINS) t += '+';
      t += '\t'; append_int(t, (long long)hp); t += '\t'; append_int(t, (long long)other); t += '\n';
    }
  return t;
}
// whether any base of the counters carried a quality
bool errprof_any_quality(const uint64_t* c) {
  for (uint32_t cls = 0; cls < 3; ++cls)
    for (uint32_t q = 0; q + 1 < mmep::QROWS; ++q) if (c[mmep::qual_at(cls, (uint8_t)q)]) return true;
  return false;
}
std::string errprof_qualities_text(const uint64_t* c) {
  std::string t = "#quality\tmatches\tmismatches\tinserted\terrorRate\tempiricalQ\n";
  for (uint32_t row = 0; row < mmep::QROWS; ++row) {
    const uint8_t q = row + 1 < mmep::QROWS ? (uint8_t)row : (uint8_t)0xFF;
    const uint64_t eq = c[mmep::qual_at(0, q)], x = c[mmep::qual_at(1, q)], ins = c[mmep::qual_at(2, q)];
    if (!eq && !x && !ins) continue;
    if (row + 1 < mmep::QROWS) append_int(t, (long long)row); else t += "none";
    for (uint64_t v : {eq, x, ins}) { t += '\t'; append_int(t, (long long)v); }
    const double rate = (double)(x + ins) / (double)(eq + x + ins);
    t += '\t'; errprof_append_fixed(t, rate, 6); t += '\t';
    if (x + ins == 0) t += "inf"; else errprof_append_fixed(t, -10.0 * std::log10(rate) + 0.0, 2);   // (+ 0.0: rate 1 prints 0.00, not -0.00)
    t += '\n';
  }
  return t;
}
std::string errprof_contigs_header() {
  return "#contigID\tlength\talignments\treadBases\trefBases\tmatches\tmismatches\tinsertions\tinsertedBases\tdeletions\tdeletedBases\tidentity\tgapCompressedIdentity\tminIdentity"
         "\tq1Identity\tmedianIdentity\tq3Identity\tmaxIdentity\n";
}
// s: the mmep::STATS values of a row
void errprof_contig_row(const std::string& name, long long length, const int64_t* s, std::string& t) {
  const int64_t eq = s[1], x = s[2], ir = s[3], ib = s[4], dr = s[5], db = s[6];
  t += name; t += '\t'; append_int(t, length);
  for (int64_t v : {s[mmep::ALIGNMENTS], eq + x + ib, eq + x + db, eq, x, ir, ib, dr, db}) { t += '\t'; append_int(t, (long long)v); }
  const int64_t all = eq + x + ib + db, gap = eq + x + ir + dr;
  t += '\t'; errprof_append_fixed(t, all ? (double)eq / (double)all : 0.0, 6);
  t += '\t'; errprof_append_fixed(t, gap ? (double)eq / (double)gap : 0.0, 6);
  for (int k = mmep::PPM_MIN; k <= mmep::PPM_MAX; ++k) { t += '\t'; errprof_append_fixed(t, (double)s[k] / 1e6, 6); }
  t += '\n';
}
// contig: the listed contigs; stats: their rows and the row of all alignments behind them
std::string errprof_contigs_text(const std::vector<int32_t>& contig, const std::vector<int64_t>& stats, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string t = errprof_contigs_header();
  if (contig.empty()) return t;                                   // (an empty run: the header alone)
  long long listed = 0;
  for (size_t j = 0; j < contig.size(); ++j) {
    errprof_contig_row(cname[(size_t)contig[j]], clen[(size_t)contig[j]], &stats[j * mmep::STATS], t);
    listed += clen[(size_t)contig[j]];
  }
  errprof_contig_row("*", listed, &stats[contig.size() * mmep::STATS], t);
  return t;
}

}  // namespace
