// mapDirectly --bam (implies --edit-distance; not in the reference): PREFIX.bam, one BAM record (SAM/BAM specification v1.6) per ALIGNED line of PREFIX in
// that order: the lines that have a PAF line under --paf.  The file is BGZF throughout: the header's members, then every batch's, then the 28-byte
// end-of-file block.
//   header    BAM\1, "@HD VN:1.6 SO:unsorted GO:query" (a read's records are consecutive), one @SQ per contig in the reference's order with the contig ID
//             as field 6 of PREFIX has it, "@PG ID:metamaps PN:metamaps" (no command line: the file is a function of the inputs), the binary reference
//             list in the same order.  Built here, deflated by mm_bgzf_deflate on the first device.
//   records   encoded and deflated on the device that mapped the batch, from the alignment the PAF path fetched (mm_bam_encode, csrc/mm_bam_core.hpp):
//             only the members come back.  This file supplies what the device cannot know: the name, the flag and the mapping quality.
//   mapq      from the TEXT of field 14 of the record's own line of PREFIX, q: 0 if q <= 0, 60 if 1 - q <= 1e-6, else min(60, floor(-10 log10(1 - q) + 0.5)).
//   flag      0x10 for strand -; 0x100 on every record of a read but its primary, the aligned record with the largest q, the first of equals.
#pragma once
#include "paf_out.hpp"
#include <cmath>

namespace {

void bam_put32(std::string& s, int32_t v) { for (int k = 0; k < 4; ++k) s += (char)((uint32_t)v >> (8 * k)); }

// the inflated header of PREFIX.bam
std::string bam_header(const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
  for (size_t c = 0; c < cname.size(); ++c) { text += "@SQ\tSN:"; text += cname[c]; text += "\tLN:"; append_int(text, clen[c]); text += '\n'; }
  text += "@PG\tID:metamaps\tPN:metamaps\n";
  std::string h("BAM\1", 4);
  bam_put32(h, (int32_t)text.size()); h += text; bam_put32(h, (int32_t)cname.size());
  for (size_t c = 0; c < cname.size(); ++c) { bam_put32(h, (int32_t)cname[c].size() + 1); h += cname[c]; h += '\0'; bam_put32(h, clen[c]); }
  return h;
}
// ... as BGZF members
std::string bam_header_members(mm_ctx* ctx, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  const std::string h = bam_header(cname, clen);
  std::string gz((size_t)mm_bgzf_deflate_bound((int64_t)h.size()), '\0');
  int64_t nbytes = 0; int32_t nblocks = 0;
  ck(ctx, mm_bgzf_deflate(ctx, (const uint8_t*)h.data(), (int64_t)h.size(), (uint8_t*)&gz[0], (int64_t)gz.size(), &nbytes, &nblocks), "deflate the BAM header");
  gz.resize((size_t)nbytes);
  return gz;
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

// the members of one batch's records into `out`
void bam_members(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const BatchAlignment& A, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names,
                 const std::vector<int64_t>& off, const std::string& text, std::string& out) {
  const size_t n = rec.size();
  out.clear();
  if (!n) return;
  const std::vector<double> q = bam_line_q(text, n);
  std::vector<int32_t> read(n), strand(n), contig(n);
  std::vector<uint16_t> flag(n); std::vector<uint8_t> mapq(n);
  std::vector<int64_t> name_off(n + 1, 0);
  std::string all_names;
  for (size_t r = 0; r + 1 < off.size(); ++r) {
    int64_t primary = -1;
    for (int64_t i = off[r]; i < off[r + 1]; ++i) if (A.dist[(size_t)i] >= 0 && (primary < 0 || q[(size_t)i] > q[(size_t)primary])) primary = i;
    if (primary >= 0 && (names[r].empty() || names[r].size() > 254)) die("--bam: the ID of read '" + names[r].substr(0, 80) + "' has 0 or more than 254 bytes: BAM cannot hold it");
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      const mm_map_record& x = rec[(size_t)i];
      read[(size_t)i] = x.read; strand[(size_t)i] = x.strand; contig[(size_t)i] = x.ref_contig;
      flag[(size_t)i] = (uint16_t)((x.strand == 1 ? 0 : 0x10) | (i == primary ? 0 : 0x100));
      mapq[(size_t)i] = bam_mapq(q[(size_t)i]);
      all_names += names[r];
      name_off[(size_t)i + 1] = (int64_t)all_names.size();
    }
  }
  mm_bam* b = nullptr;
  ck(ctx, mm_bam_encode(ctx, reads, reference, (int64_t)n, read.data(), strand.data(), contig.data(), A.dist.data(), A.first.data(), A.op_off.data(), A.ops.data(), flag.data(), mapq.data(),
                        name_off.data(), all_names.data(), 0, &b), "BAM records");
  int64_t n_records = 0, raw = 0, bytes = 0;
  mm_bam_sizes(b, &n_records, &raw, &bytes);
  out.resize((size_t)bytes);
  if (bytes) mm_bam_fetch(b, (uint8_t*)&out[0]);
  mm_bam_destroy(b);
}

}  // namespace
