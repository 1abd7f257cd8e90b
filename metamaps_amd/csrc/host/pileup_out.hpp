// mapDirectly --pileup [--pileup-min-count N] [--pileup-min-frac F] (implies --edit-distance; not in the reference): PREFIX.pileup and PREFIX.pileup.contigs,
// what a column-by-column count over the PRIMARY records of PREFIX.bam gives (the definition: csrc/mm_pileup_core.hpp).  Both are plain text whatever
// --compress-output says; an empty run writes two empty files.
//   PREFIX.pileup          one tab-separated line per kept entry in key order (contig in the reference's order, position, code):
//                          contigID  pos (0-based)  ref (the contig's byte as the set holds it)  alt  count  depth
//                          alt: A C G T N, - for a deleted base, + for an insertion behind this base (before it where it leads the alignment).
//                          Kept: count >= N (default 3) and count >= F * depth (default 0.2); mm_pileup_finish decides, on the first device.
//   PREFIX.pileup.contigs  one line per contig with a contributing alignment, in the reference's order: contigID  length  alignments  covered  sumDepth
//   primary                a read's aligned record without 0x100 in bam_fields' flags (bam_out.hpp): under --all a read counts once.
//   accumulator            a batch's (key, count) pairs and the (contig, first, last) of its contributing alignments are appended under a mutex; above
//                          MM_PILEUP_MERGE_PAIRS pairs (64 * 2^20) the pairs are replaced by their mm_pileup_merge (batch_outputs.hpp).
// Text, arrays and the option values only (the key's fields: mm_pileup_core.hpp, plain host code here): nothing here calls the device.
#pragma once
#include "../mm_pileup_core.hpp"
#include "cli_common.hpp"
#include "side_files.hpp"
#include "fast_format.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

// --pileup-min-count N, --pileup-min-frac F: validated before any work; refused without --pileup
// --base-qualities, --min-base-quality Q (QualOpts, cli_common.hpp): Q an integer 0..93, which implies --base-qualities and needs an output that counts evidence;
// --base-qualities alone needs one that uses the qualities (--bam, --error-profile).  (The refusals by sub-command and by --hpc are output_plan's, under the flag's own name.)
QualOpts qual_options(const Options& o) {
  QualOpts q;
  q.keep = o.v.count("base-qualities") != 0;
  if (o.v.count("min-base-quality")) {
    const std::string& v = o.v.at("min-base-quality");
    const IntegerValue x = integer_value(v, 2);
    if (!x.ok || x.value > 93) die("--min-base-quality takes an integer from 0 to 93, not '" + v + "'");
    if (!o.v.count("pileup") && !o.v.count("vcf") && !o.v.count("consensus")) die("--min-base-quality needs --pileup, --vcf or --consensus: nothing else counts a base's evidence");
    q.min_base_quality = (int)x.value; q.keep = true;
  } else if (q.keep && !o.v.count("bam") && !o.v.count("error-profile") && !reads_out_asked(o))
    die("--base-qualities needs --bam or --min-base-quality (or --error-profile, --extract-unmapped, --extract-mapped, --extract-taxa, --deplete-taxa): nothing else would use the qualities");
  return q;
}
struct PileupOpts { bool on = false; long long min_count = 3; double min_frac = 0.2; };
PileupOpts pileup_options(const Options& o) {
  PileupOpts p;
  p.on = o.v.count("pileup") != 0;
  if (o.v.count("pileup-min-count")) {
    const std::string& v = o.v.at("pileup-min-count");
    if (!p.on) die("--pileup-min-count needs --pileup");
    const IntegerValue x = integer_value(v, 9);
    if (!x.ok || x.value < 1) die("--pileup: --pileup-min-count takes an integer from 1 to 999999999, not '" + v + "'");
    p.min_count = (long long)x.value;
  }
  if (o.v.count("pileup-min-frac")) {
    const std::string& v = o.v.at("pileup-min-frac");
    if (!p.on) die("--pileup-min-frac needs --pileup");
    const DecimalValue x = decimal_value(v);
    if (!x.ok || !(x.value >= 0.0 && x.value <= 1.0)) die("--pileup: --pileup-min-frac takes a decimal from 0 to 1, not '" + v + "'");
    p.min_frac = x.value;
  }
  return p;
}

// use[i] of mm_pileup_events: record i is aligned and is its read's primary record (flag: bam_fields')
std::vector<uint8_t> pileup_use(const std::vector<uint16_t>& flag, const std::vector<int32_t>& dist) {
  std::vector<uint8_t> use(flag.size());
  for (size_t i = 0; i < flag.size(); ++i) use[i] = dist[i] >= 0 && !(flag[i] & 0x100) ? 1 : 0;
  return use;
}

// (key, count) rows of the pileup (w1 empty) or of the VCF (w1: the keys' second words), as they come from the device and go back to it
struct VariantRows {
  std::vector<uint64_t> w0, w1; std::vector<uint32_t> counts;
  void resize(size_t n, bool two_words) { w0.resize(n); if (two_words) w1.resize(n); counts.resize(n); }
};
// what the batches of one query file leave behind for its pileup or for its VCF: rows, merged now and then (keys may repeat)
struct VariantAcc { std::mutex m; VariantRows rows; };
// every contributing alignment of a query file's run, once for the pileup and the VCF
struct Intervals {
  std::mutex m;
  std::vector<int32_t> contig; std::vector<int64_t> first, last;
  void add_intervals(const std::vector<uint8_t>& use, const std::vector<int32_t>& c, const std::vector<int64_t>& f, const std::vector<int64_t>& l) {
    std::lock_guard<std::mutex> lk(m);
    for (size_t i = 0; i < use.size(); ++i) if (use[i]) { contig.push_back(c[i]); first.push_back(f[i]); last.push_back(l[i]); }
  }
};

std::string pileup_text(const std::vector<uint64_t>& key, const std::vector<uint32_t>& count, const std::vector<uint32_t>& depth, const std::vector<uint8_t>& ref_byte,
                        const std::vector<std::string>& cname) {
  std::string t;
  t.reserve(key.size() * 48);
  for (size_t i = 0; i < key.size(); ++i) {
    t += cname[(size_t)mmp::key_contig(key[i])]; t += '\t'; append_int(t, (long long)mmp::key_pos(key[i])); t += '\t'; t += (char)ref_byte[i]; t += '\t';
    t += mmp::code_letter(mmp::key_code(key[i])); t += '\t'; append_int(t, (long long)count[i]); t += '\t'; append_int(t, (long long)depth[i]); t += '\n';
  }
  return t;
}
std::string pileup_contigs_text(const std::vector<int64_t>& alignments, const std::vector<int64_t>& covered, const std::vector<int64_t>& sum_depth,
                                const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string t;
  for (size_t c = 0; c < alignments.size(); ++c) {
    if (!alignments[c]) continue;
    t += cname[c]; t += '\t'; append_int(t, clen[c]); t += '\t'; append_int(t, (long long)alignments[c]); t += '\t'; append_int(t, (long long)covered[c]); t += '\t';
    append_int(t, (long long)sum_depth[c]); t += '\n';
  }
  return t;
}

}  // namespace
