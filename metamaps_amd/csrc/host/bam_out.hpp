// mapDirectly --bam (implies --edit-distance; not in the reference): PREFIX.bam, one BAM record (SAM/BAM specification v1.6) per ALIGNED line of PREFIX in
// that order: the lines that have a PAF line under --paf.  The file is BGZF throughout: the header's members, then every batch's, then the 28-byte
// end-of-file block (side_files.hpp).
//   header    BAM\1, "@HD VN:1.6 SO:unsorted GO:query" (a read's records are consecutive;
//             "@HD VN:1.6 SO:coordinate" for PREFIX.sorted.bam: bam_sort_out.hpp), one @SQ per contig in the reference's order with the contig ID
//             as field 6 of PREFIX has it, "@PG ID:metamaps PN:metamaps" (no command line: the file is a function of the inputs), the binary reference
//             list in the same order.  Built here, deflated by mm_bgzf_deflate on the first device (run_outputs.hpp).
//   records   encoded and deflated on the device that mapped the batch, from the alignment the PAF path fetched (mm_bam_encode, csrc/mm_bam_core.hpp;
//             called from batch_outputs.hpp): only the members come back.  This file supplies what the device cannot know: the name, the flag and the
//             mapping quality (bam_fields).
//   mapq      from the TEXT of field 14 of the record's own line of PREFIX, q: 0 if q <= 0, 60 if 1 - q <= 1e-6, else min(60, floor(-10 log10(1 - q) + 0.5)).
//   flag      0x10 for strand -; 0x100 on every record of a read but its primary, the aligned record with the largest q, the first of equals.
// Bytes and arrays only: nothing here calls the device.
#pragma once
#include "../../../include/metamaps_hip.h"
#include "cli_common.hpp"
#include "fast_format.hpp"
#include <cmath>
#include <cstdlib>

namespace {

void bam_put32(std::string& s, int32_t v) { for (int k = 0; k < 4; ++k) s += (char)((uint32_t)v >> (8 * k)); }

// the inflated header of PREFIX.bam
std::string bam_header(const std::vector<std::string>& cname, const std::vector<int>& clen, bool sorted = false) {   // sorted: PREFIX.sorted.bam's first line
  std::string text = sorted ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
  for (size_t c = 0; c < cname.size(); ++c) { text += "@SQ\tSN:"; text += cname[c]; text += "\tLN:"; append_int(text, clen[c]); text += '\n'; }
  text += "@PG\tID:metamaps\tPN:metamaps\n";
  std::string h("BAM\1", 4);
  bam_put32(h, (int32_t)text.size()); h += text; bam_put32(h, (int32_t)cname.size());
  for (size_t c = 0; c < cname.size(); ++c) { bam_put32(h, (int32_t)cname[c].size() + 1); h += cname[c]; h += '\0'; bam_put32(h, clen[c]); }
  return h;
}

uint8_t bam_mapq(double q) {
  if (q <= 0) return 0;
  if (1 - q <= 1e-6) return 60;
  const double v = std::floor(-10 * std::log10(1 - q) + 0.5);
  return (uint8_t)(v < 0 ? 0 : v > 60 ? 60 : v);
}
// field 14 (the last one) of every line of a batch's text, parsed as the double a reader of PREFIX gets
std::vector<double> bam_line_q(const std::string& text, size_t n_lines) {
  std::vector<double> q; q.reserve(n_lines);
  for (size_t at = 0; at < text.size();) {
    size_t end = text.find('\n', at); if (end == std::string::npos) end = text.size();
    const size_t sp = text.rfind(' ', end - 1);
    q.push_back(strtod(text.c_str() + (sp == std::string::npos || sp < at ? at : sp + 1), nullptr));
    at = end + 1;
  }
  if (q.size() != n_lines) die("internal error: the lines of a batch and its records differ in number");
  return q;
}

// what mm_bam_encode takes per record beside the alignment, in the order of the lines of PREFIX
struct BamFields {
  std::vector<int32_t> read, strand, contig;
  std::vector<uint16_t> flag;
  std::vector<uint8_t> mapq;
  std::vector<int64_t> name_off;                                 // record i's name: all_names[name_off[i] .. name_off[i + 1])
  std::string all_names;
};
// ... of one batch: dist is the alignment's (-1: not aligned), text the batch's formatted lines.  A read with an aligned record must have a name BAM
// can hold (1-254 bytes); a read without one gets no record, so its name is not looked at.
BamFields bam_fields(const std::vector<int32_t>& dist, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names, const std::vector<int64_t>& off,
                     const std::string& text) {
  const size_t n = rec.size();
  const std::vector<double> q = bam_line_q(text, n);
  BamFields F;
  F.read.resize(n); F.strand.resize(n); F.contig.resize(n); F.flag.resize(n); F.mapq.resize(n); F.name_off.assign(n + 1, 0);
  for (size_t r = 0; r + 1 < off.size(); ++r) {
    int64_t primary = -1;
    for (int64_t i = off[r]; i < off[r + 1]; ++i) if (dist[(size_t)i] >= 0 && (primary < 0 || q[(size_t)i] > q[(size_t)primary])) primary = i;
    if (primary >= 0 && (names[r].empty() || names[r].size() > 254))
      die("--bam: the ID of read '" + names[r].substr(0, 80) + "' has 0 or more than 254 bytes: BAM cannot hold it");
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      const mm_map_record& x = rec[(size_t)i];
      F.read[(size_t)i] = x.read; F.strand[(size_t)i] = x.strand; F.contig[(size_t)i] = x.ref_contig;
      F.flag[(size_t)i] = (uint16_t)((x.strand == 1 ? 0 : 0x10) | (i == primary ? 0 : 0x100));
      F.mapq[(size_t)i] = bam_mapq(q[(size_t)i]);
      F.all_names += names[r];
      F.name_off[(size_t)i + 1] = (int64_t)F.all_names.size();
    }
  }
  return F;
}

}  // namespace
