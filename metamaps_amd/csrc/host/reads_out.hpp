// mapDirectly --extract-unmapped, --extract-mapped, --extract-taxa LIST, --deplete-taxa LIST (not in the reference, whose util/extractReads.pl re-reads the
// FASTQ on the host): selected reads of every query file as BGZF FASTQ (under --base-qualities) or FASTA beside PREFIX, written on the device from the
// batch's packed reads (mm_reads_encode, csrc/mm_reads_out_core.hpp; the call sits in batch_outputs.hpp).  Here: the options, the table of labels and
// suffixes, and which reads of a batch each file takes.  No device call.
//   unmapped   every read without a line in PREFIX: the reads .meta counts as ReadsTooShort and as ReadsNotMapped
//   mapped     every read with at least one line
//   taxa       the mapped reads whose primary line (the largest printed field 14, the first of equals: bam_fields' rule, read from the formatted text)
//              lies on a contig whose taxon (extract_taxon, compared as a string) is in the list
//   depleted   every read that `taxa` with the same list would not take, unmapped and too-short reads included (host depletion)
// All in query order.  A list is 1 to 64 distinct tokens x?[0-9]+; exact IDs only.
#pragma once
#include "side_files.hpp"
#include "taxonomy.hpp"
#include <cstring>
#include <set>
#include <zlib.h>

namespace {

enum { EX_UNMAPPED, EX_MAPPED, EX_TAXA, EX_DEPLETED, N_EXTRACT };
struct ExtractFile { const char* flag; int side; bool list; };   // the option as Options::v names it, its row of kSideFiles, whether it takes a list
constexpr ExtractFile kExtract[N_EXTRACT] = {
  {"extract-unmapped", SIDE_X_UNMAPPED, false},
  {"extract-mapped", SIDE_X_MAPPED, false},
  {"extract-taxa", SIDE_X_TAXA, true},
  {"deplete-taxa", SIDE_X_DEPLETED, true},
};
constexpr size_t EXTRACT_LIST_MAX = 64;

struct ReadsOutOpts {
  std::array<bool, N_EXTRACT> on{};
  std::vector<std::string> list[N_EXTRACT];                      // the tokens of the two taxon flags
  bool with_qual = false;                                        // --base-qualities (given, or implied by --min-base-quality): FASTQ records and .fq.gz, else FASTA and .fa.gz;
                                                                 // the one value both the record kind and the file's suffix go by
  bool any() const { for (bool b : on) if (b) return true; return false; }
  const char* first_flag() const { for (int f = 0; f < N_EXTRACT; ++f) if (on[(size_t)f]) return kExtract[f].flag; return ""; }
};

// the tokens of a list; refused under the flag's name: no token, an empty or malformed token, a repeated one, more than 64
inline std::vector<std::string> extract_list(const std::string& flag, const std::string& v) {
  std::vector<std::string> out;
  std::set<std::string> seen;
  if (v.empty()) die("--" + flag + " takes a list of 1 to 64 taxon IDs (x?[0-9]+, comma-separated), not an empty one");
  for (size_t a = 0; a <= v.size();) {
    size_t b = v.find(',', a); if (b == std::string::npos) b = v.size();
    const std::string t = v.substr(a, b - a);
    const size_t d0 = !t.empty() && t[0] == 'x' ? 1 : 0;
    if (t.size() == d0 || t.find_first_not_of("0123456789", d0) != std::string::npos) die("--" + flag + ": '" + t + "' is not a taxon ID (x?[0-9]+)");
    if (!seen.insert(t).second) die("--" + flag + ": the taxon ID " + t + " is listed twice");
    out.push_back(t);
    a = b + 1;
  }
  if (out.size() > EXTRACT_LIST_MAX) die("--" + flag + " takes at most 64 taxon IDs, not " + std::to_string(out.size()));
  return out;
}
inline ReadsOutOpts reads_out_options(const Options& o) {
  ReadsOutOpts r;
  for (int f = 0; f < N_EXTRACT; ++f) {
    if (!o.v.count(kExtract[f].flag)) continue;
    r.on[(size_t)f] = true;
    if (kExtract[f].list) r.list[f] = extract_list(kExtract[f].flag, o.v.at(kExtract[f].flag));
  }
  r.with_qual = o.v.count("base-qualities") != 0 || o.v.count("min-base-quality") != 0;   // (--min-base-quality implies --base-qualities: qual_options)
  return r;
}

// per contig, once: whether its taxon is in the list of --extract-taxa ([0]) and of --deplete-taxa ([1]).  A contig without the key ends the run with
// extract_taxon's message.
struct ContigHits { std::vector<uint8_t> hit[2]; };
inline ContigHits contig_hits(const ReadsOutOpts& r, const std::vector<std::string>& cname) {
  ContigHits h;
  if (!r.on[EX_TAXA] && !r.on[EX_DEPLETED]) return h;
  const std::set<std::string> s0(r.list[EX_TAXA].begin(), r.list[EX_TAXA].end()), s1(r.list[EX_DEPLETED].begin(), r.list[EX_DEPLETED].end());
  h.hit[0].resize(cname.size()); h.hit[1].resize(cname.size());
  for (size_t c = 0; c < cname.size(); ++c) { const std::string t = extract_taxon(cname[c]); h.hit[0][c] = s0.count(t) != 0; h.hit[1][c] = s1.count(t) != 0; }
  return h;
}

// Under a taxon flag, before any device work: the header lines of the reference FASTA (plain or gzip; zlib reads both) are scanned once and every contig ID
// (the header up to the first blank) must carry a taxon.  A sequence line never starts with '>'.  (MapRun asks the parsed names again behind the loader.)
inline void check_reference_taxa(const ReadsOutOpts& r, const std::string& path) {
  if (!r.on[EX_TAXA] && !r.on[EX_DEPLETED]) return;
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) die("Cannot open reference file " + path);
  gzbuffer(f, 1 << 20);
  std::vector<char> buf((size_t)1 << 16);
  bool line_start = true;
  while (gzgets(f, buf.data(), (int)buf.size())) {
    const size_t n = strlen(buf.data());
    if (line_start && buf[0] == '>') {
      std::string id(buf.data() + 1, n - 1);
      id = id.substr(0, id.find_first_of(" \t\r\n"));
      (void)extract_taxon(id);
    }
    line_start = n > 0 && buf[n - 1] == '\n';
  }
  gzclose(f);
}

// the contig of every read's primary line, -1 for a read without a line.  off: the reads' lines [off[r], off[r + 1]); contig and q: per line its contig
// and its printed field 14
inline std::vector<int32_t> primary_contigs(const std::vector<int64_t>& off, const std::vector<int32_t>& contig, const std::vector<double>& q) {
  std::vector<int32_t> out(off.empty() ? 0 : off.size() - 1, -1);
  for (size_t r = 0; r + 1 < off.size(); ++r) {
    int64_t primary = -1;
    for (int64_t i = off[r]; i < off[r + 1]; ++i) if (primary < 0 || q[(size_t)i] > q[(size_t)primary]) primary = i;
    if (primary >= 0) out[r] = contig[(size_t)primary];
  }
  return out;
}
// the reads of a batch that file f takes, ascending
inline std::vector<int32_t> extract_selection(int f, const std::vector<int32_t>& primary, const ContigHits& h) {
  std::vector<int32_t> sel;
  for (size_t r = 0; r < primary.size(); ++r) {
    const bool mapped = primary[r] >= 0;
    const bool take = f == EX_UNMAPPED ? !mapped : f == EX_MAPPED ? mapped : f == EX_TAXA ? mapped && h.hit[0][(size_t)primary[r]] : !(mapped && h.hit[1][(size_t)primary[r]]);
    if (take) sel.push_back((int32_t)r);
  }
  return sel;
}

}  // namespace
