// The files mapDirectly writes beside PREFIX when asked to: one table that MapRun's workers (map_outputs.hpp) and writer go by.  No device call.
#pragma once
#include "cli_common.hpp"
#include <array>

namespace {

struct SideFile {
  const char* flag;                                              // the option that asks for it, as Options::v names it
  const char* suffix;                                            // PREFIX + suffix
  bool bgzf;                                                     // BGZF members: a head at open (the BAM header), kBgzfEof at close; else plain text
};
enum { SIDE_EDIT, SIDE_PAF, SIDE_BAM, N_SIDE };
constexpr SideFile kSideFiles[N_SIDE] = {
  {"edit-distance", ".editDistances", false},
  {"paf", ".paf", false},
  {"bam", ".bam", true},
};
using SideSet = std::array<bool, N_SIDE>;

// the rows a command line asks for: --paf and --bam imply --edit-distance (their alignment is the one whose distances that file lists)
// --bam-sorted (bam_sort_out.hpp) is no row: its two files are written after the run's last batch; it implies --edit-distance too
inline bool bam_sorted_of(const Options& o) { return o.v.count("bam-sorted") != 0; }
inline SideSet side_files_of(const Options& o) {
  SideSet on{};
  for (int s = 0; s < N_SIDE; ++s) on[(size_t)s] = o.v.count(kSideFiles[s].flag) != 0;
  for (int s = 0; s < N_SIDE; ++s) if (on[(size_t)s]) on[SIDE_EDIT] = true;
  if (bam_sorted_of(o)) on[SIDE_EDIT] = true;
  return on;
}

// BGZF's end-of-file marker (SAM/BAM specification v1.6, section 4.1.2): an empty member, the last 28 bytes of PREFIX.gz and of PREFIX.bam
constexpr unsigned char kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace
