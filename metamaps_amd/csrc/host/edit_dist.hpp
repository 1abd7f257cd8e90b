// mapDirectly --edit-distance: PREFIX.editDistances, one line per line of PREFIX in the same order:
//   readID contigID strand d first last        (strand + / -; first, last: 0-based inclusive contig coordinates; "NA NA NA": not aligned)
// d, first and last come from the device (mm_mapping_edit_distances: Myers' bit-vector alignment of every record inside the window around its
// mapped position, within floor(1.5 L (100 - pi) / 100) edits).  The context that mapped a batch aligns it, against its device's packed reference,
// before the batch's reads and mapping are destroyed (batch_outputs.hpp).  Text only: nothing here calls the device.
#pragma once
#include "../../../include/metamaps_hip.h"
#include "cli_common.hpp"
#include "fast_format.hpp"

namespace {

// the lines of one batch from its records' d, first, last; rec: the batch's records as fetched (the order of the lines of PREFIX)
void edit_distance_text(const int32_t* dist, const int64_t* first, const int64_t* last, const std::vector<std::string>& names, const std::vector<int64_t>& off,
                        const std::vector<mm_map_record>& rec, const std::vector<std::string>& cname, std::string& out) {
  out.clear();
  out.reserve(rec.size() * 64);
  for (size_t r = 0; r + 1 < off.size(); ++r)
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      const mm_map_record& x = rec[(size_t)i];
      out += names[r]; out += ' '; out += cname[(size_t)x.ref_contig]; out += ' '; out += x.strand == 1 ? '+' : '-';
      if (dist[(size_t)i] < 0) { out += " NA NA NA\n"; continue; }
      out += ' '; append_int(out, dist[(size_t)i]); out += ' '; append_int(out, (long long)first[(size_t)i]); out += ' '; append_int(out, (long long)last[(size_t)i]); out += '\n';
    }
}

}  // namespace
