// mapDirectly --vcf [--vcf-min-count N] [--vcf-min-frac F] (implies --edit-distance; not in the reference): PREFIX.vcf (VCFv4.2, sites only), the SNV, deletion and
// insertion alleles of the PRIMARY records of PREFIX.bam, every indel left-aligned so that equal variants of different reads count together (the definition:
// csrc/mm_vcf_core.hpp).  Plain text whatever --compress-output says; an empty run writes the header alone.
//   header     ##fileformat, ##source, one ##contig per contig in the reference's order, ##INFO for DP AO SVTYPE SVLEN END, ##ALT for INS and DEL, #CHROM
//   lines      one per kept allele in key order (contig, position, code, w1): CHROM POS ID REF ALT QUAL FILTER INFO with ID, QUAL and FILTER "."; several
//              lines may share a POS (no multi-allelic records).  POS = pos + 1; a reference byte outside A C G T prints as N.
//                SNV              REF ref[pos]          ALT the base           INFO DP=depth;AO=count
//                DEL, n <= 24     REF ref[a .. a + n]   ALT ref[a]
//                INS, n <= 24     REF ref[a]            ALT ref[a] + bases
//                DEL, n > 24      REF ref[a]            ALT <DEL>              INFO ...;SVTYPE=DEL;SVLEN=-n;END=a + 1 + n
//                INS, n > 24      REF ref[a]            ALT <INS>              INFO ...;SVTYPE=INS;SVLEN=n;END=a + 1
//              Kept: count >= N (default 3) and count >= F * depth (default 0.2); mm_vcf_finish decides, on the first device, and hands back the
//              reference bytes ref[pos .. pos + 25) that REF is printed from.
//   accumulator  a batch's (w0, w1, count) triples are appended under a mutex, 20 bytes each; above MM_VCF_MERGE_PAIRS triples (64 * 2^20) they are replaced by
//              their mm_vcf_merge (batch_outputs.hpp).  The accumulator and the intervals of the contributing alignments are pileup_out.hpp's: one copy of the intervals serves both.
// Text, arrays and the option values only (the key's fields: mm_vcf_core.hpp, plain host code here): nothing here calls the device.
#pragma once
#include "../mm_vcf_core.hpp"
#include "pileup_out.hpp"

namespace {

// --vcf-min-count N, --vcf-min-frac F: validated before any work; refused without --vcf
struct VcfOpts { bool on = false; long long min_count = 3; double min_frac = 0.2; };
VcfOpts vcf_options(const Options& o) {
  VcfOpts p;
  p.on = o.v.count("vcf") != 0;
  if (o.v.count("vcf-min-count")) {
    const std::string& v = o.v.at("vcf-min-count");
    if (!p.on) die("--vcf-min-count needs --vcf");
    const IntegerValue x = integer_value(v, 9);
    if (!x.ok || x.value < 1) die("--vcf: --vcf-min-count takes an integer from 1 to 999999999, not '" + v + "'");
    p.min_count = (long long)x.value;
  }
  if (o.v.count("vcf-min-frac")) {
    const std::string& v = o.v.at("vcf-min-frac");
    if (!p.on) die("--vcf-min-frac needs --vcf");
    const DecimalValue x = decimal_value(v);
    if (!x.ok || !(x.value >= 0.0 && x.value <= 1.0)) die("--vcf: --vcf-min-frac takes a decimal from 0 to 1, not '" + v + "'");
    p.min_frac = x.value;
  }
  return p;
}

// (min_base_quality > 0, --min-base-quality: one more line, which names the floor the alleles were counted under)
std::string vcf_header(const std::vector<std::string>& cname, const std::vector<int>& clen, int min_base_quality = 0) {
  std::string t = "##fileformat=VCFv4.2\n##source=metamaps mapDirectly --vcf\n";
  if (min_base_quality > 0) { t += "##minBaseQuality="; append_int(t, min_base_quality); t += "\n"; }
  for (size_t c = 0; c < cname.size(); ++c) { t += "##contig=<ID="; t += cname[c]; t += ",length="; append_int(t, clen[c]); t += ">\n"; }
  t += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Primary alignments that span the position\">\n"
       "##INFO=<ID=AO,Number=1,Type=Integer,Description=\"Primary alignments that carry the allele\">\n"
       "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of a symbolic allele\">\n"
       "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"Length of a symbolic allele, negative for a deletion\">\n"
       "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last reference position of a symbolic allele\">\n"
       "##ALT=<ID=INS,Description=\"Insertion of more than 24 bases\">\n"
       "##ALT=<ID=DEL,Description=\"Deletion of more than 24 bases\">\n"
       "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
  return t;
}
char vcf_ref_letter(uint8_t b) { return mmp::base_code(b) < 4 ? (char)mmb::upper(b) : 'N'; }
// the lines of the kept alleles; window: mmv::WINDOW reference bytes per allele from its position on (mm_vcf_result_fetch)
std::string vcf_lines(const std::vector<uint64_t>& w0, const std::vector<uint64_t>& w1, const std::vector<uint32_t>& count, const std::vector<uint32_t>& depth,
                      const std::vector<uint8_t>& window, const std::vector<std::string>& cname) {
  std::string t;
  t.reserve(w0.size() * 64);
  for (size_t i = 0; i < w0.size(); ++i) {
    const uint8_t* win = &window[i * (size_t)mmv::WINDOW];
    const long long pos = (long long)mmp::key_pos(w0[i]);
    const uint32_t code = mmp::key_code(w0[i]);
    const long long n = code == mmp::CODE_DEL ? (long long)w1[i] : code == mmp::CODE_INS ? (long long)mmv::ins_len(w1[i]) : 0;
    const bool symbolic = n > mmv::INS_BASES_MAX;
    t += cname[(size_t)mmp::key_contig(w0[i])]; t += '\t'; append_int(t, pos + 1); t += "\t.\t";
    t += vcf_ref_letter(win[0]);
    if (code == mmp::CODE_DEL && !symbolic) for (long long j = 1; j <= n; ++j) t += vcf_ref_letter(win[j]);
    t += '\t';
    if (code < 4) t += "ACGT"[code];
    else if (symbolic) t += code == mmp::CODE_DEL ? "<DEL>" : "<INS>";
    else {
      t += vcf_ref_letter(win[0]);
      if (code == mmp::CODE_INS) for (long long j = 0; j < n; ++j) t += "ACGT"[mmv::ins_bases(w1[i]) >> (2 * j) & 3u];
    }
    t += "\t.\t.\tDP="; append_int(t, (long long)depth[i]); t += ";AO="; append_int(t, (long long)count[i]);
    if (symbolic) {
      t += code == mmp::CODE_DEL ? ";SVTYPE=DEL;SVLEN=-" : ";SVTYPE=INS;SVLEN="; append_int(t, n);
      t += ";END="; append_int(t, code == mmp::CODE_DEL ? pos + 1 + n : pos + 1);
    }
    t += '\n';
  }
  return t;
}

}  // namespace
