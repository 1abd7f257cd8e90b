// classify --min-identity T [--refit] (the reference's util/filterLowIdentityEntities.pl; DESIGN.md section 4, "Identity filter"): the host side of the
// identity filter.  The arithmetic — every read's largest identity, the genomes' median best identities, which genomes go, the EM problem that is
// left — runs on the first device (mm_ident_filter); here are the identity field of a mapping line, the text of PREFIX.extractedIdentities placed by
// the device's order, and the filtered WIMP.  ClassifyRun (classify_run.hpp) owns the lines; its writers (classify_outputs.hpp) call these.  No device call in here.
#pragma once
#include "taxonomy.hpp"
#include <cstring>

namespace {
namespace identf {

// what mm_ident_filter returned for the EM problem of a run (identities in percent)
struct Filter {
  double thr = 0;
  std::vector<double> ident, sorted_max, taxon_median;
  int64_t n_with = 0, n_le = 0, n_reads_out = 0, n_entries_out = 0;
  std::vector<int64_t> taxon_reads, read_src, entry_src, read_off_out;
  std::vector<uint8_t> taxon_removed, read_removed;
  size_t genomes_hit() const { size_t n = 0; for (int64_t c : taxon_reads) n += c > 0; return n; }
  size_t genomes_removed() const { size_t n = 0; for (uint8_t c : taxon_removed) n += c != 0; return n; }
  size_t reads_removed() const { size_t n = 0; for (uint8_t c : read_removed) n += c != 0; return n; }
};

// 0-based field 12 of a mapping line (the upper-bound identity in percent, what the script reads; NOT field 9, the identity --genes uses): the text
// between the last two blanks of the line.  `line` .. `line + last_space` ends at the blank before field 13.
inline void identity_field(const char* line, size_t last_space, const char** beg, size_t* len) {
  const char* e = line + last_space; const char* b = e;
  while (b > line && b[-1] != ' ') --b;
  *beg = b; *len = (size_t)(e - b);
}
inline double identity_value(const char* line, size_t last_space) {
  const char* b; size_t n; identity_field(line, last_space, &b, &n);
  char* end = nullptr;
  const double v = strtod(b, &end);                                // (the field ends in a blank)
  if (end != b + n || n == 0) die("--min-identity: a mapping line's identity field '" + std::string(b, n) + "' is not a number");
  return v;
}

// PREFIX.extractedIdentities: sorted_max, every value as the text of the field it came from; equal values in read order.  The order is the device's:
// read r's text goes to the first free place among the places of its value in sorted_max.  max_line(r): the line and last_space of the read's first
// entry that carries its largest identity.
template <class Lines> void write_identities(const std::string& fn, const Filter& F, const std::vector<int64_t>& off, const Lines& lines) {
  const size_t n = (size_t)F.n_with;
  std::vector<std::pair<const char*, size_t>> text(n, {nullptr, 0});
  std::vector<int64_t> used(n, 0);                                 // per first place of a value: how many of its places are taken
  for (size_t r = 0; r + 1 < off.size(); ++r) {
    if (off[r + 1] == off[r]) continue;
    size_t at = (size_t)off[r];
    for (size_t i = at + 1; i < (size_t)off[r + 1]; ++i) if (F.ident[i] > F.ident[at]) at = i;
    const size_t first = (size_t)(std::lower_bound(F.sorted_max.begin(), F.sorted_max.end(), F.ident[at]) - F.sorted_max.begin());
    const size_t place = first + (size_t)used[first]++;
    if (place >= n || F.sorted_max[place] != F.ident[at]) die("--min-identity: internal error, the device's sorted identities do not hold a read's largest identity");
    identity_field(lines[at].p, lines[at].last_space, &text[place].first, &text[place].second);
  }
  std::string out;
  for (auto& t : text) { out.append(t.first, t.second); out += '\n'; }
  std::ofstream o(fn);
  o.write(out.data(), (std::streamsize)out.size());
}

// PREFIX.EM-filtered.WIMP: per level the kept reads of every genome at its ancestor of that rank (the genome itself counts, `no rank` nodes do not), at
// 0 where it has none; 0 starts at the unmapped reads and takes the removed ones.  kept[t]: reads whose best genome is taxon t and stays.
inline void write_filtered_wimp(const std::string& fn, const Taxonomy& T, const std::vector<std::string>& taxa, const std::vector<int64_t>& kept, size_t n_removed_reads,
                                size_t n_unmapped, size_t n_with_mapping) {
  static const char* const levels[] = {"definedGenomes", "species", "genus", "family"};
  const std::set<std::string> want{"species", "genus", "family"};
  std::vector<std::map<std::string, std::string>> up(taxa.size());
  for (size_t t = 0; t < taxa.size(); ++t) if (kept[t] > 0) up[t] = T.upward_by_ranks(taxa[t], want);
  const double total = (double)(n_unmapped + n_with_mapping);
  std::ofstream o(fn);
  o << "AnalysisLevel\ttaxonID\tName\tAbsolute\tEMFrequency\tPotFrequency\n";
  char num[64];
  for (const char* level : levels) {
    std::map<std::string, size_t> dist;
    size_t zero = n_unmapped + n_removed_reads;
    for (size_t t = 0; t < taxa.size(); ++t) {
      if (kept[t] <= 0) continue;
      const std::string& id = level == levels[0] ? taxa[t] : up[t].at(level);
      if (id == "Undefined") zero += (size_t)kept[t]; else dist[id] += (size_t)kept[t];
    }
    std::vector<std::pair<std::string, size_t>> rows(dist.begin(), dist.end());   // (by taxon ID as bytes)
    std::stable_sort(rows.begin(), rows.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
    snprintf(num, sizeof num, "%.15g", (double)zero / total);
    o << level << "\t0\tUnclassified\t" << zero << "\tNA\t" << num << "\n";
    for (auto& r : rows) {
      snprintf(num, sizeof num, "%.15g", (double)r.second / total);
      o << level << "\t" << r.first << "\t" << T.T.at(r.first).sci << "\t" << r.second << "\tNA\t" << num << "\n";
    }
  }
}

}  // namespace identf
}  // namespace
