// From the mapping lines of a `classify` run to the EM problem: PREFIX.meta, DB/taxonInfo.txt, the taxon of every contig, and per mapping its taxon, its
// quality and 1/nLoc (read_tables, per_mapping_fields); what the EM hands on (EmResult); the statistics of a row of the bootstrap file.  No device call and
// no C ABI in here: tests/test_mapping_lines.cpp compiles it on its own.
#pragma once
#include "mapping_lines.hpp"
#include "taxonomy.hpp"

namespace {

struct ClassifyTables {
  std::vector<std::string> taxa;                                  // the taxa of the mapped contigs, in std::set order: index = taxon number on the device
  std::vector<int> contig_tx; std::vector<long long> contig_len_ti;   // per contig: taxon index; length per taxonInfo (-1: not listed)
  std::vector<int32_t> taxon; std::vector<double> mapq, inv;      // per mapping
  std::map<std::string, size_t> st; size_t nUnmapped = 0, nTooShort = 0, nTotal = 0;   // PREFIX.meta
  // read_tables -> per_mapping_fields
  std::vector<std::string> contig_taxon_id;
  std::map<std::string, std::map<std::string, size_t>> TI;       // fEM.h:1320-1364
};
struct EmResult { std::vector<double> f, post; std::vector<int64_t> best; };   // per taxon; per mapping; per read (index into the whole mapping list)

// the taxa of the mapped contigs, PREFIX.meta, DB/taxonInfo.txt
inline ClassifyTables read_tables(const MappingLines& M, const std::string& mapped, const std::string& db) {
  ClassifyTables C;
  std::set<std::string> taxaSet;
  C.contig_taxon_id.assign(M.contig_id.size(), std::string());
  for (size_t c = 0; c < M.contig_id.size(); ++c) { C.contig_taxon_id[c] = extract_taxon(M.contig_id[c]); taxaSet.insert(C.contig_taxon_id[c]); }
  if (taxaSet.empty()) die("No relevant taxon IDs found in your mappings file - is it possible that none of your reads are mapped?");
  C.taxa.assign(taxaSet.begin(), taxaSet.end());
  { std::ifstream s(mapped + ".meta");
    if (!s.is_open()) die("The file " + mapped + ".meta is not present or could not be opened - this file is generated automatically as part of the "
                          "mapping process, so please check whether the mapping process finished successfully.");
    std::string a; size_t b; while (s >> a >> b) C.st[a] = b; }
  C.nUnmapped = C.st.at("ReadsNotMapped"); C.nTooShort = C.st.at("ReadsTooShort"); C.nTotal = C.st.at("TotalReads");
  { std::ifstream s(db + "/taxonInfo.txt"); if (!s.is_open()) die("Could not open file " + db + "/taxonInfo.txt -- perhaps you have specified an incomplete DB?");
    std::string ln;
    while (std::getline(s, ln)) {
      if (ln.empty()) continue;
      auto f = split(ln, " ");
      for (auto& c : split(f.at(1), ";")) { auto kv = split(c, "="); C.TI[f.at(0)][kv.at(0)] = std::stoull(kv.at(1)); }
    } }
  return C;
}

// per mapping: taxon, quality, 1/nLoc (getMappingLocations, fEM.h:234-353).  nLoc(read, taxon) = sum over the taxon's contigs of
// (len - L + 1) if len >= L, else 1 if the read has a mapping on that contig (:325-348): sorted lengths + suffix sums per taxon
inline void per_mapping_fields(const MappingLines& M, ClassifyTables& C) {
  const std::vector<std::string>& taxa = C.taxa;
  std::map<std::string, int> tindex; for (size_t i = 0; i < taxa.size(); ++i) tindex[taxa[i]] = (int)i;
  C.contig_tx.assign(M.contig_id.size(), 0); C.contig_len_ti.assign(M.contig_id.size(), -1);
  struct TaxLens { std::vector<long long> len, suffix; };
  std::vector<TaxLens> tl(taxa.size());
  for (size_t t = 0; t < taxa.size(); ++t) {
    auto it = C.TI.find(taxa[t]);
    if (it == C.TI.end()) die("Unknown taxonID '" + taxa[t] + "'; please check that your mappings file was mapped against the database now specified.");
    for (auto& c : it->second) tl[t].len.push_back((long long)c.second);
    std::sort(tl[t].len.begin(), tl[t].len.end());
    tl[t].suffix.assign(tl[t].len.size() + 1, 0);
    for (size_t i = tl[t].len.size(); i-- > 0;) tl[t].suffix[i] = tl[t].suffix[i + 1] + tl[t].len[i];
  }
  for (size_t c = 0; c < M.contig_id.size(); ++c) {
    C.contig_tx[c] = tindex.at(C.contig_taxon_id[c]);
    auto& m = C.TI.at(C.contig_taxon_id[c]); auto it = m.find(M.contig_id[c]);
    if (it != m.end()) C.contig_len_ti[c] = (long long)it->second;
  }
  const std::vector<MapLine>& lines = M.lines;
  C.taxon.assign(lines.size(), 0); C.mapq.assign(lines.size(), 0.0); C.inv.assign(lines.size(), 0.0);
  std::vector<int> seen_c;                                       // distinct contigs of the current read
  for (size_t r = 0; r < M.NRD; ++r) {
    const size_t a0 = (size_t)M.off[r], b0 = (size_t)M.off[r + 1];
    const long long L = lines[a0].len;
    seen_c.clear();
    for (size_t i = a0; i < b0; ++i) if (std::find(seen_c.begin(), seen_c.end(), lines[i].contig) == seen_c.end()) seen_c.push_back(lines[i].contig);
    for (size_t i = a0; i < b0; ++i) {
      const int t = C.contig_tx[(size_t)lines[i].contig];
      const TaxLens& X = tl[(size_t)t];
      const size_t k0 = (size_t)(std::lower_bound(X.len.begin(), X.len.end(), L) - X.len.begin());
      long long n = X.suffix[k0] - (long long)(X.len.size() - k0) * (L - 1);
      for (int c : seen_c) if (C.contig_tx[(size_t)c] == t && C.contig_len_ti[(size_t)c] >= 0 && C.contig_len_ti[(size_t)c] < L) ++n;
      C.taxon[i] = t; C.mapq[i] = lines[i].mapq; C.inv[i] = 1 / (double)(size_t)n;
    }
  }
}

// A row of PREFIX.EM.WIMP.bootstrap over the n >= 2 replicates that drew a read: mean, SD over n - 1, and the 2.5 % and 97.5 % quantiles, linear
// between order statistics (numpy's default)
struct RowStats { double mean, sd, lo, hi; };
inline RowStats bootstrap_row_stats(const std::vector<double>& v) {
  auto quantile = [](const std::vector<double>& x, double q) {
    const double h = q * (double)(x.size() - 1); const size_t k = (size_t)std::floor(h);
    return k + 1 < x.size() ? x[k] + (h - (double)k) * (x[k + 1] - x[k]) : x[k];
  };
  const size_t n = v.size();
  double mean = 0; for (double x : v) mean += x; mean /= (double)n;
  double ss = 0; for (double x : v) ss += (x - mean) * (x - mean);
  std::vector<double> x = v; std::sort(x.begin(), x.end());
  return RowStats{mean, std::sqrt(ss / (double)(n - 1)), quantile(x, 0.025), quantile(x, 0.975)};
}

}  // namespace
