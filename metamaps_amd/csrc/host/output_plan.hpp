// What the command line asks mapDirectly to write beside PREFIX (OutputPlan): every output's options parsed once, before any device work, and every question
// the run asks about their combination answered in one place.  The option parsers of the *_out.hpp headers and the table of side_files.hpp only: no device call,
// nothing of the C ABI (tests/test_output_plan.cpp compiles this header alone).
//
// Adding a run output: its options parser and its writers in a *_out.hpp of its own, one member and its place in the predicates here, one call in
// BatchSideOutputs::from_text (batch_outputs.hpp) and one in RunOutputs::write (run_outputs.hpp).
#pragma once
#include "consensus_out.hpp"
#include "depth_out.hpp"
#include "motif_out.hpp"
#include "reads_out.hpp"
#include "side_files.hpp"
#include "vcf_out.hpp"

namespace {

struct OutputPlan {
  SideSet side{};                                                // the files a batch adds to as it is written (side_files.hpp); side[SIDE_EDIT] is edit()
  PileupOpts pileup; VcfOpts vcf; ConsOpts cons; ModsOpts mods; MotifOpts motifs; DepthOpts depth;   // the outputs with a table per query file, written after the last batch
  QualOpts qual;                                                 // --base-qualities, --min-base-quality: the batches carry the reads' qualities to the device
  ReadsOutOpts reads;                                            // --extract-*, --deplete-taxa: the read files (rows of `side` that need no alignment)
  bool bam_sorted = false, errprof = false;                      // --bam-sorted, --error-profile: bare flags

  // --vcf and --consensus keep one table of alleles between them (PREFIX.vcf is written under --vcf alone)
  bool vcf_table() const { return vcf.on || cons.on; }
  // An aligned output was asked for (--edit-distance, or one of the nine that imply it).  Governs: the packed reference stays on every device, every batch is
  // aligned (from_mapping), PREFIX.editDistances is written, and the run is refused where the reference is not resident (flag_name()).
  bool edit() const { return side[SIDE_EDIT]; }
  // The name those refusals are made under: the most specific output asked for
  const char* flag_name() const {
    return errprof ? "--error-profile" : depth.on ? "--depth" : mods.on ? (motifs.on ? "--mod-motifs" : "--mods") : cons.on ? "--consensus" : vcf.on ? "--vcf" : pileup.on ? "--pileup"
           : side[SIDE_BAM] ? "--bam" : bam_sorted ? "--bam-sorted" : side[SIDE_PAF] ? "--paf" : "--edit-distance";
  }
  // The alignments' op runs are needed: from_mapping calls mm_mapping_align; without (plain --edit-distance, --depth) mm_mapping_edit_distances, the distances alone.
  // An output missing here would get empty runs.
  bool traceback() const { return side[SIDE_PAF] || side[SIDE_BAM] || bam_sorted || pileup.on || vcf_table() || mods.on || errprof; }
  // A batch's reads on the device outlive from_mapping and go at the end of from_text, which reads their bases, qualities or calls (--depth reads none of them,
  // but from_text does nothing without reads).  An output missing here would find them destroyed.
  bool reads_until_text() const { return side[SIDE_BAM] || bam_sorted || pileup.on || vcf_table() || mods.on || depth.on || errprof || reads.any(); }
  // A batch's reads outlive its mapping at all (else the worker drops them before the records are fetched)
  bool keep_reads() const { return edit() || reads.any(); }
  // The (contig, first, last) of every primary alignment of a query file are kept for the end of the run (mm_pileup_finish, mm_vcf_finish, mm_consensus, mm_depth_profile)
  bool intervals() const { return pileup.on || vcf_table() || depth.on; }
  // The run keeps accumulators per query file (RunOutputs::File)
  bool per_file_state() const { return pileup.on || vcf_table() || mods.on || depth.on || errprof; }
};

// The plan of a command line for sub-command `mode`.  Every parser ends the program on a malformed value, in this order; the three refusals by place (outside
// mapDirectly, --hpc, an index that is sharded or streamed) stand between them where they have always been said, each under its own flag's name.
inline OutputPlan output_plan(const Options& o, const std::string& mode) {
  OutputPlan p;
  p.pileup = pileup_options(o); p.vcf = vcf_options(o); p.cons = consensus_options(o);
  p.mods = mods_options(o); p.motifs = motif_options(o, p.mods); p.depth = depth_options(o);
  p.qual = qual_options(o);
  if (o.v.count("base-qualities") || o.v.count("min-base-quality")) {
    const std::string flag = o.v.count("min-base-quality") ? "--min-base-quality" : "--base-qualities";
    if (mode != "mapDirectly") die(flag + " belongs to mapDirectly: it carries the qualities of a run's reads to the device that aligns them");
    if (o.v.count("hpc")) die(flag + " cannot be combined with --hpc: a homopolymer-compressed read has no per-base qualities");
    if (o.stream || o.shard) die(flag + " cannot be combined with --shard-index or --stream-chunks: the whole reference must be resident where the reads are");
  }
  p.reads = reads_out_options(o);
  if (p.reads.any()) {
    const std::string flag = std::string("--") + p.reads.first_flag();
    if (mode != "mapDirectly") die(flag + " belongs to mapDirectly: it writes a run's reads from the batches that run holds on the device");
    if (o.v.count("hpc")) die(flag + " cannot be combined with --hpc: the raw reads do not stay on the device");
    if (o.stream || o.shard) die(flag + " cannot be combined with --shard-index or --stream-chunks: a batch's reads stay on the device only when every chunk index is resident");
  }
  p.bam_sorted = o.v.count("bam-sorted") != 0; p.errprof = o.v.count("error-profile") != 0;
  p.side = side_files_of(o);
  p.side[SIDE_EDIT] = o.v.count("edit-distance") || p.side[SIDE_PAF] || p.side[SIDE_BAM] || p.bam_sorted || p.pileup.on || p.vcf.on || p.cons.on || p.mods.on || p.depth.on || p.errprof;
  if (p.edit()) {
    const std::string flag = p.flag_name();
    if (mode != "mapDirectly") die(flag + " belongs to mapDirectly: it aligns a run's reads to the reference that run has packed on the device");
    if (o.v.count("hpc")) die(flag + " cannot be combined with --hpc: the raw reference does not stay on the device");
    if (o.stream || o.shard) die(flag + " cannot be combined with --shard-index or --stream-chunks: the whole reference must be resident where the reads are");
  }
  return p;
}

}  // namespace
