// mapDirectly --paf: PREFIX.paf beside PREFIX and PREFIX.editDistances, one line per ALIGNED line of PREFIX in that order (tab-separated):
//   readID  L  0  L  +|-  contigID  contigLen  first  last+1  n_eq  n_eq+n_X+n_I+n_D  255  NM:i:d  cg:Z:<runs with = X I D>
// The read is aligned whole (query start 0, end L); first / last+1 are the alignment's 0-based half-open contig coordinates; for strand - the CIGAR is that
// of the reverse-complemented read along the forward contig, as PAF has it.  A mapping that is not aligned (NA NA NA in .editDistances) has no line.
// One call (mm_mapping_align, batch_outputs.hpp) on the context that mapped the batch gives d, first, last and the runs, fetched once (BatchAlignment):
// the lines of PREFIX.editDistances (edit_dist.hpp: the bytes of a run with --edit-distance alone), the lines of PREFIX.paf and the records of
// PREFIX.bam (bam_out.hpp) come from the same answer, nothing is aligned twice.  Text only: nothing here calls the device.
#pragma once
#include "../../../include/metamaps_hip.h"
#include "cli_common.hpp"
#include "fast_format.hpp"

namespace {

// what mm_alignment_fetch gives for the records of one batch, in the order of the lines of PREFIX
struct BatchAlignment {
  std::vector<int32_t> dist;                                     // per record: the edit distance, -1: not aligned
  std::vector<int64_t> first, last;                              // per record: the alignment's 0-based inclusive contig coordinates
  std::vector<int64_t> op_off;                                   // per record: where its runs start in ops (one more entry than records)
  std::vector<uint32_t> ops;                                     // the runs, BAM's words: len << 4 | op with I = 1, D = 2, = = 7, X = 8
};

void paf_text(const BatchAlignment& A, const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off, const std::vector<mm_map_record>& rec,
              const std::vector<std::string>& cname, const std::vector<int>& clen, std::string& paf) {
  const std::vector<int32_t>& dist = A.dist;
  const std::vector<int64_t>&first = A.first, &last = A.last, &op_off = A.op_off;
  const std::vector<uint32_t>& ops = A.ops;
  paf.clear();
  paf.reserve(rec.size() * 96 + ops.size() * 4);
  static const char LETTER[16] = {'?', 'I', 'D', '?', '?', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
  for (size_t r = 0; r + 1 < off.size(); ++r)
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      if (dist[(size_t)i] < 0) continue;
      const mm_map_record& x = rec[(size_t)i];
      long long n_eq = 0, n_all = 0;
      for (int64_t k = op_off[(size_t)i]; k < op_off[(size_t)i + 1]; ++k) { const uint32_t w = ops[(size_t)k]; n_all += w >> 4; if ((w & 15u) == 7u) n_eq += w >> 4; }
      paf += names[r]; paf += '\t'; append_int(paf, lens[r]); paf += "\t0\t"; append_int(paf, lens[r]); paf += '\t'; paf += x.strand == 1 ? '+' : '-'; paf += '\t';
      paf += cname[(size_t)x.ref_contig]; paf += '\t'; append_int(paf, clen[(size_t)x.ref_contig]); paf += '\t'; append_int(paf, (long long)first[(size_t)i]); paf += '\t';
      append_int(paf, (long long)last[(size_t)i] + 1); paf += '\t'; append_int(paf, n_eq); paf += '\t'; append_int(paf, n_all); paf += "\t255\tNM:i:"; append_int(paf, dist[(size_t)i]);
      paf += "\tcg:Z:";
      for (int64_t k = op_off[(size_t)i]; k < op_off[(size_t)i + 1]; ++k) { const uint32_t w = ops[(size_t)k]; append_int(paf, (long long)(w >> 4)); paf += LETTER[w & 15u]; }
      paf += '\n';
    }
}

}  // namespace
