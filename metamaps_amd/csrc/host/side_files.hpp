// The files mapDirectly writes beside PREFIX when asked to: one table that MapRun's workers (batch_outputs.hpp) and writer go by.  No device call.
#pragma once
#include "cli_common.hpp"
#include <array>

namespace {

struct SideFile {
  const char* flag;                                              // the option that asks for it, as Options::v names it
  const char* suffix;                                            // PREFIX + suffix
  bool bgzf;                                                     // BGZF members, kBgzfEof at close; else plain text
  bool head;                                                     // the BAM header (as BGZF members) at open; else an empty head
  bool aligned;                                                  // made from the batch's alignment: implies --edit-distance
  const char* suffix_no_qual;                                    // the suffix without --base-qualities where that differs (the read files: FASTA), else null
};
enum { SIDE_EDIT, SIDE_PAF, SIDE_BAM, SIDE_X_UNMAPPED, SIDE_X_MAPPED, SIDE_X_TAXA, SIDE_X_DEPLETED, N_SIDE };
constexpr SideFile kSideFiles[N_SIDE] = {
  {"edit-distance", ".editDistances", false, false, true, nullptr},
  {"paf", ".paf", false, false, true, nullptr},
  {"bam", ".bam", true, true, true, nullptr},
  {"extract-unmapped", ".unmapped.fq.gz", true, false, false, ".unmapped.fa.gz"},   // the four read files (reads_out.hpp)
  {"extract-mapped", ".mapped.fq.gz", true, false, false, ".mapped.fa.gz"},
  {"extract-taxa", ".taxa.fq.gz", true, false, false, ".taxa.fa.gz"},
  {"deplete-taxa", ".depleted.fq.gz", true, false, false, ".depleted.fa.gz"},
};
inline std::string side_suffix(int s, bool with_qual) { return !with_qual && kSideFiles[s].suffix_no_qual ? kSideFiles[s].suffix_no_qual : kSideFiles[s].suffix; }
using SideSet = std::array<bool, N_SIDE>;

inline bool reads_out_asked(const Options& o) { for (int s = 0; s < N_SIDE; ++s) if (!kSideFiles[s].aligned && o.v.count(kSideFiles[s].flag)) return true; return false; }
// the rows a command line asks for: --paf and --bam imply --edit-distance (their alignment is the one whose distances that file lists)
// --bam-sorted (bam_sort_out.hpp) is no row: its two files are written after the run's last batch; it implies --edit-distance too.  (So do the outputs that
// keep a table per query file, which have no row either: OutputPlan, output_plan.hpp, adds them.)
inline SideSet side_files_of(const Options& o) {
  SideSet on{};
  for (int s = 0; s < N_SIDE; ++s) on[(size_t)s] = o.v.count(kSideFiles[s].flag) != 0;
  for (int s = 0; s < N_SIDE; ++s) if (on[(size_t)s] && kSideFiles[s].aligned) on[SIDE_EDIT] = true;   // (the read files need no alignment)
  if (o.v.count("bam-sorted")) on[SIDE_EDIT] = true;
  return on;
}

// BGZF's end-of-file marker (SAM/BAM specification v1.6, section 4.1.2): an empty member, the last 28 bytes of PREFIX.gz and of PREFIX.bam
constexpr unsigned char kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace
