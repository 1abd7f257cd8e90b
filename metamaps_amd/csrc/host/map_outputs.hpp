// The side outputs of a batch of mapDirectly (the rows of side_files.hpp: PREFIX.editDistances, .paf, .bam) and the device calls they need.  The text
// and byte rules are in edit_dist.hpp, paf_out.hpp and bam_out.hpp, which call nothing; everything here runs on the context that mapped the batch.
#pragma once
#include "bam_out.hpp"
#include "cli_device.hpp"
#include "edit_dist.hpp"
#include "paf_out.hpp"
#include "side_files.hpp"
#include <memory>

namespace {

// a batch's reads on the device, held by one owner: destroyed once, when the last output that needs them is made (or when that owner goes)
struct SeqsetDestroy { void operator()(mm_seqset* s) const { mm_seqset_destroy(s); } };
using ReadsPtr = std::unique_ptr<mm_seqset, SeqsetDestroy>;

using SideBytes = std::array<std::string, N_SIDE>;               // what one batch adds to every side file

// `raw` as BGZF members (mm_bgzf_deflate: blocks of 65 280 bytes, each a member of its own, so what is deflated piece by piece concatenates)
void bgzf_members(mm_ctx* ctx, const std::string& raw, std::string& gz, const char* what) {
  gz.resize((size_t)mm_bgzf_deflate_bound((int64_t)raw.size()));
  int64_t nbytes = 0; int32_t nblocks = 0;
  ck(ctx, mm_bgzf_deflate(ctx, (const uint8_t*)raw.data(), (int64_t)raw.size(), (uint8_t*)&gz[0], (int64_t)gz.size(), &nbytes, &nblocks), what);
  gz.resize((size_t)nbytes);
}
// the header of PREFIX.bam (bam_out.hpp) as BGZF members
std::string bam_header_members(mm_ctx* ctx, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string gz;
  bgzf_members(ctx, bam_header(cname, clen), gz, "deflate the BAM header");
  return gz;
}

// The side outputs of one batch, in the two steps the order of a batch's device calls leaves: the alignment needs the mapping, which goes before the
// lines are formatted; the BAM records need the formatted lines (their mapping qualities are read from the text).  One alignment serves all three files.
struct BatchSideOutputs {
  const SideSet& on;
  BatchAlignment al;

  // while the mapping lives: d, first, last (and the runs, where .paf or .bam want them) fetched once -> the lines of .editDistances and .paf.
  // The reads go here unless .bam needs them for SEQ.  Nothing happens without reads (no side file was asked for).
  void from_mapping(mm_ctx* ctx, const mm_mapping* m, ReadsPtr& reads, const mm_seqset* reference, float pi, const std::vector<mm_map_record>& rec,
                    const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off, const std::vector<std::string>& cname,
                    const std::vector<int>& clen, SideBytes& out) {
    if (!reads) return;
    const size_t n = rec.size();
    if (on[SIDE_PAF] || on[SIDE_BAM]) {
      mm_alignment* a = nullptr;
      ck(ctx, mm_mapping_align(ctx, m, reads.get(), reference, pi, &a), "alignments");
      int64_t n_jobs = 0, n_ops = 0;
      mm_alignment_sizes(a, &n_jobs, &n_ops);
      if (n_jobs != (int64_t)n) die("internal error: alignments and records differ in number");
      al.dist.resize(n); al.first.resize(n); al.last.resize(n); al.op_off.resize(n + 1); al.ops.resize((size_t)n_ops);
      mm_alignment_fetch(a, al.dist.data(), al.first.data(), al.last.data(), al.op_off.data(), al.ops.data());
      mm_alignment_destroy(a);
    } else {                                                       // --edit-distance alone: the distances without the traceback
      al.dist.resize(n); al.first.resize(n); al.last.resize(n);
      ck(ctx, mm_mapping_edit_distances(ctx, m, reads.get(), reference, pi, al.dist.data(), al.first.data(), al.last.data(), (int64_t)n), "edit distances");
    }
    edit_distance_text(al.dist.data(), al.first.data(), al.last.data(), names, off, rec, cname, out[SIDE_EDIT]);
    if (on[SIDE_PAF]) paf_text(al, names, lens, off, rec, cname, clen, out[SIDE_PAF]);
    if (!on[SIDE_BAM]) reads.reset();
  }

  // once the lines are formatted: the batch's BAM records as BGZF members, encoded and deflated on the device; the reads, kept for this, go
  void from_text(mm_ctx* ctx, ReadsPtr& reads, const mm_seqset* reference, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names,
                 const std::vector<int64_t>& off, const std::string& text, SideBytes& out) {
    if (!reads) return;
    std::string& members = out[SIDE_BAM];
    members.clear();
    if (!rec.empty()) {
      const BamFields F = bam_fields(al.dist, rec, names, off, text);
      mm_bam* b = nullptr;
      ck(ctx, mm_bam_encode(ctx, reads.get(), reference, (int64_t)rec.size(), F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(),
                            al.op_off.data(), al.ops.data(), F.flag.data(), F.mapq.data(), F.name_off.data(), F.all_names.data(), 0, &b), "BAM records");
      int64_t n_records = 0, raw = 0, bytes = 0;
      mm_bam_sizes(b, &n_records, &raw, &bytes);
      members.resize((size_t)bytes);
      if (bytes) mm_bam_fetch(b, (uint8_t*)&members[0]);
      mm_bam_destroy(b);
    }
    reads.reset();
  }
};

}  // namespace
