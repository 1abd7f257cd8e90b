// What runs once per batch of mapDirectly for the outputs of an OutputPlan (output_plan.hpp), on the context that mapped the batch: its device calls and BatchSideOutputs.
#pragma once
#include "bam_out.hpp"
#include "bam_sort_out.hpp"
#include "mapping_lines.hpp"
#include "cli_device.hpp"
#include "cli_switches.hpp"
#include "edit_dist.hpp"
#include "errprof_out.hpp"
#include "output_plan.hpp"
#include "paf_out.hpp"
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

// The device's calls of --pileup and of --vcf in one shape, for the two functions below: a pileup table has one-word keys, a VCF table two.
// fetch: the rows behind a handle, which goes.
struct PileupCalls {
  using Table = mm_pileup;
  static constexpr const char* events_what = "pileup events"; static constexpr const char* merge_what = "pileup merge";
  static constexpr auto events = mm_pileup_events_q;
  static int merge(mm_ctx* ctx, const VariantRows& v, Table** t) { return mm_pileup_merge(ctx, (int64_t)v.w0.size(), v.w0.data(), v.counts.data(), t); }
  static void fetch(Table* t, VariantRows& v) {
    int64_t n = 0;
    mm_pileup_sizes(t, &n); v.resize((size_t)n, false); mm_pileup_fetch(t, v.w0.data(), v.counts.data()); mm_pileup_destroy(t);
  }
};
struct VcfCalls {
  using Table = mm_vcf;
  static constexpr const char* events_what = "vcf events"; static constexpr const char* merge_what = "vcf merge";
  static constexpr auto events = mm_vcf_events_q;
  static int merge(mm_ctx* ctx, const VariantRows& v, Table** t) { return mm_vcf_merge(ctx, (int64_t)v.w0.size(), v.w0.data(), v.w1.data(), v.counts.data(), t); }
  static void fetch(Table* t, VariantRows& v) {
    int64_t n = 0;
    mm_vcf_sizes(t, &n); v.resize((size_t)n, true); mm_vcf_fetch(t, v.w0.data(), v.w1.data(), v.counts.data()); mm_vcf_destroy(t);
  }
};
// --mods in the same shape: one-word keys; the int32 behind `use` is the ML threshold where the other two take the base-quality floor
struct ModCalls {
  using Table = mm_mod;
  static constexpr const char* events_what = "modification events"; static constexpr const char* merge_what = "modification merge";
  static constexpr auto events = mm_mod_events;
  static int merge(mm_ctx* ctx, const VariantRows& v, Table** t) { return mm_mod_merge(ctx, (int64_t)v.w0.size(), v.w0.data(), v.counts.data(), t); }
  static void fetch(Table* t, VariantRows& v) {
    int64_t n = 0;
    mm_mod_sizes(t, &n); v.resize((size_t)n, false); mm_mod_fetch(t, v.w0.data(), v.counts.data()); mm_mod_destroy(t);
  }
};
// rows and their sums through the output's merge, which leaves them unique and ascending
template <class C> void merge_rows(mm_ctx* ctx, VariantRows& v) {
  typename C::Table* t = nullptr;
  ck(ctx, C::merge(ctx, v, &t), C::merge_what);
  C::fetch(t, v);
}
// --pileup and --vcf, per batch: the events (alleles) of the primary aligned records (use) counted on the context that mapped the batch, appended to the
// file's accumulator; above merge_pairs rows the accumulator is replaced by its merge.  min_base_quality: --min-base-quality's floor (0: none)
template <class C> void add_batch(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const BamFields& F, const BatchAlignment& al, const std::vector<uint8_t>& use,
                                  int32_t min_base_quality, size_t merge_pairs, VariantAcc& acc) {
  typename C::Table* t = nullptr;
  ck(ctx, C::events(ctx, reads, reference, (int64_t)use.size(), F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(), al.op_off.data(), al.ops.data(),
                    use.data(), min_base_quality, &t), C::events_what);
  VariantRows got;
  C::fetch(t, got);
  std::lock_guard<std::mutex> lk(acc.m);
  VariantRows& a = acc.rows;
  a.w0.insert(a.w0.end(), got.w0.begin(), got.w0.end()); a.w1.insert(a.w1.end(), got.w1.begin(), got.w1.end()); a.counts.insert(a.counts.end(), got.counts.begin(), got.counts.end());
  if (a.w0.size() > merge_pairs) merge_rows<C>(ctx, a);
}
// --error-profile, per batch: the counters, columns and identity keys of the primary aligned records (use) walked on the context that mapped the batch
void errprof_add_batch(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const BamFields& F, const BatchAlignment& al, const std::vector<uint8_t>& use, ErrprofAcc& acc) {
  uint64_t counters[MM_ERRPROF_COUNTERS];
  std::vector<int32_t> cols(use.size() * MM_ERRPROF_COLS); std::vector<uint64_t> key(use.size());
  ck(ctx, mm_errprof_events(ctx, reads, reference, (int64_t)use.size(), F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(), al.op_off.data(), al.ops.data(),
                            use.data(), counters, cols.data(), key.data()), "error profile");
  acc.add(counters, key, cols);
}
// --extract-*, --deplete-taxa, per batch: the reads each file takes (reads_out.hpp) written as FASTQ / FASTA records and deflated on the context that holds the
// batch's reads (mm_reads_encode); only the members come back.  A batch without a selected read adds nothing to the file.  hits: the contigs the two lists take
void extract_batch(mm_ctx* ctx, const mm_seqset* reads, const ReadsOutOpts& ro, const ContigHits& hits, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names,
                   const std::vector<int64_t>& off, const std::string& text, SideBytes& out) {
  std::vector<int32_t> contig(rec.size());
  for (size_t i = 0; i < rec.size(); ++i) contig[i] = rec[i].ref_contig;
  const std::vector<int32_t> primary = primary_contigs(off, contig, bam_line_q(text, rec.size()));
  for (int f = 0; f < N_EXTRACT; ++f) {
    if (!ro.on[(size_t)f]) continue;
    std::string& members = out[(size_t)kExtract[f].side];
    members.clear();
    const std::vector<int32_t> sel = extract_selection(f, primary, hits);
    if (sel.empty()) continue;
    std::vector<int64_t> name_off(sel.size() + 1, 0); std::string all;
    for (size_t i = 0; i < sel.size(); ++i) { all += names[(size_t)sel[i]]; name_off[i + 1] = (int64_t)all.size(); }
    mm_reads_text* t = nullptr;
    ck(ctx, mm_reads_encode(ctx, reads, (int64_t)sel.size(), sel.data(), name_off.data(), all.data(), ro.with_qual ? 1 : 0, 0, &t), (std::string("--") + kExtract[f].flag).c_str());
    int64_t n_records = 0, raw = 0, bytes = 0;
    mm_reads_text_sizes(t, &n_records, &raw, &bytes);
    members.resize((size_t)bytes);
    if (bytes) mm_reads_text_fetch(t, (uint8_t*)&members[0]);
    mm_reads_text_destroy(t);
  }
}

// what the batches of one query file add to, until RunOutputs::write (run_outputs.hpp) makes its files of them: the primary alignments' intervals, the tables
// of --pileup, of --vcf and --consensus and of --mods, and the error profile's sums
struct FileAcc { Intervals iv; VariantAcc pile, vcf, mods; ErrprofAcc errprof; };

// The side outputs of one batch, in the two steps the order of a batch's device calls leaves: the alignment needs the mapping, which goes before the
// lines are formatted; the BAM records need the formatted lines (their mapping qualities are read from the text).  One alignment serves every output.
// Made by RunOutputs::batch, which binds it to the batch's query file.
struct BatchSideOutputs {
  const OutputPlan& plan; const CliSwitches& sw;
  FileAcc* file;                                                 // the accumulators of the batch's query file (null without plan.per_file_state())
  SortedRun* sorted;                                             // --bam-sorted: the batch's sorted run (null without)
  const ContigHits& hits;                                        // the read files: which contigs the two taxon lists take
  BatchAlignment al{};

  // while the mapping lives: d, first, last (and the runs, under plan.traceback()) fetched once -> the lines of .editDistances and .paf.
  // The reads go here unless plan.reads_until_text().
  // Nothing happens without reads (no side file was asked for), and nothing here for the read files alone: they need no alignment, and their reads wait.
  void from_mapping(mm_ctx* ctx, const mm_mapping* m, ReadsPtr& reads, const mm_seqset* reference, float pi, const std::vector<mm_map_record>& rec,
                    const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off, const std::vector<std::string>& cname,
                    const std::vector<int>& clen, SideBytes& out) {
    if (!reads || !plan.edit()) return;
    const size_t n = rec.size();
    if (plan.traceback()) {
      mm_alignment* a = nullptr;
      ck(ctx, mm_mapping_align(ctx, m, reads.get(), reference, pi, &a), "alignments");
      int64_t n_jobs = 0, n_ops = 0;
      mm_alignment_sizes(a, &n_jobs, &n_ops);
      if (n_jobs != (int64_t)n) die("internal error: alignments and records differ in number");
      al.dist.resize(n); al.first.resize(n); al.last.resize(n); al.op_off.resize(n + 1); al.ops.resize((size_t)n_ops);
      mm_alignment_fetch(a, al.dist.data(), al.first.data(), al.last.data(), al.op_off.data(), al.ops.data());
      mm_alignment_destroy(a);
    } else {                                                       // the distances without the traceback
      al.dist.resize(n); al.first.resize(n); al.last.resize(n);
      ck(ctx, mm_mapping_edit_distances(ctx, m, reads.get(), reference, pi, al.dist.data(), al.first.data(), al.last.data(), (int64_t)n), "edit distances");
    }
    edit_distance_text(al.dist.data(), al.first.data(), al.last.data(), names, off, rec, cname, out[SIDE_EDIT]);
    if (plan.side[SIDE_PAF]) paf_text(al, names, lens, off, rec, cname, clen, out[SIDE_PAF]);
    if (!plan.reads_until_text()) reads.reset();
  }

  // once the lines are formatted: the batch's read files, what it adds to its query file's accumulators and to the sorted BAM, and its BAM records as BGZF
  // members, encoded and deflated on the device (all but the first go by bam_fields' primary record, which needs the lines); the reads, kept for this, go
  void from_text(mm_ctx* ctx, ReadsPtr& reads, const mm_seqset* reference, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names,
                 const std::vector<int64_t>& off, const std::string& text, SideBytes& out) {
    if (!reads) return;
    if (plan.reads.any()) extract_batch(ctx, reads.get(), plan.reads, hits, rec, names, off, text, out);   // (every read of the batch: one without a line is `unmapped`)
    std::string& members = out[SIDE_BAM];
    members.clear();
    if (plan.edit() && !rec.empty()) {
      const BamFields F = bam_fields(al.dist, rec, names, off, text);
      if (plan.per_file_state()) {
        const int32_t min_q = plan.qual.min_base_quality;          // --min-base-quality: the floor of the pileup's events and of the alleles (not of the modification counts)
        const std::vector<uint8_t> use = pileup_use(F.flag, al.dist);
        if (plan.errprof) errprof_add_batch(ctx, reads.get(), reference, F, al, use, file->errprof);
        if (plan.mods.on) add_batch<ModCalls>(ctx, reads.get(), reference, F, al, use, plan.mods.min_ml, sw.mods_merge_pairs, file->mods);
        if (plan.intervals()) file->iv.add_intervals(use, F.contig, al.first, al.last);
        if (plan.pileup.on) add_batch<PileupCalls>(ctx, reads.get(), reference, F, al, use, min_q, sw.pileup_merge_pairs, file->pile);
        if (plan.vcf_table()) add_batch<VcfCalls>(ctx, reads.get(), reference, F, al, use, min_q, sw.vcf_merge_pairs, file->vcf);
      }
      if (plan.bam_sorted) sorted_run_encode(ctx, reads.get(), reference, F, al, (int64_t)rec.size(), *sorted);
      if (!plan.side[SIDE_BAM]) { reads.reset(); return; }
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

// what a worker of MapRun hands to its writer: the finished text of one batch and what the batch adds to every side file
struct BatchDone {
  size_t file = 0;
  std::vector<std::string> names;
  std::vector<int> lens;
  std::vector<int> clens;                                          // --hpc: the compressed lengths (lens stay raw)
  std::vector<int64_t> off;
  std::string text;
  std::string gz;                                                  // --compress-output: the text as BGZF members
  SideBytes side;                                                  // what the batch adds to every side file (side_files.hpp): lines, or BGZF members
  SortedRun sorted;                                                // --bam-sorted: the batch's sorted run
  std::vector<LineMeta> meta;
  double t_mapq = 0, t_fetch = 0, t_format = 0;
};

}  // namespace
