// The files of one `classify` run, written from what the earlier stages left (ClassifyView): the four per-read files formatted in ranges of reads, the
// tallies and coverage windows of the best mappings, the bootstrap file beside the WIMP, the LCA reads file, and the files of --min-identity and --refit.
// No device call in here: ClassifyRun (classify_run.hpp) makes those and calls these in order.
#pragma once
#include "classify_tables.hpp"
#include "ident_filter.hpp"

namespace {

struct ClassifyView { const std::string& mapped; const std::string& db; const MappingLines& M; const ClassifyTables& C; const EmResult& E; const Taxonomy& T; };

// a line of PREFIX.EM: the mapping line with field 14 replaced by std::to_string(posterior) (fEM.h:705)
inline void em_line(std::string& s, const MapLine& L, double p) { s.append(L.p, (size_t)L.last_space + 1); append_f6(s, p); s += '\n'; }
inline void write_text(const std::string& fn, const std::string& text) { std::ofstream o(fn); o.write(text.data(), (std::streamsize)text.size()); }

// what PREFIX.EM.reads2Taxon and its krona form end in: the unmapped and the too short reads (PREFIX.meta.unmappedReadsLengths) at taxon 0
struct UnmappedTail { std::string r2t, krona; };
inline UnmappedTail unmapped_tail(const std::string& mapped) {
  UnmappedTail t; std::string ln;
  std::ifstream s(mapped + ".meta.unmappedReadsLengths");
  while (std::getline(s, ln)) { if (ln.empty()) continue; const std::string id = split(ln, "\t").at(1); t.r2t += id; t.r2t += "\t0\n"; t.krona += id; t.krona += "\t0\t0\n"; }
  return t;
}

// the point estimate or a refit as the WIMP takes it: by taxon ID, through cleanF with n_mapped reads
inline std::map<std::string, double> cleaned_frequencies(const std::vector<std::string>& taxa, const std::vector<double>& f, const std::map<std::string, size_t>& readsPer, size_t n_mapped) {
  std::map<std::string, double> fmap;
  for (size_t i = 0; i < taxa.size(); ++i) fmap[taxa[i]] = f[i];
  clean_frequencies(fmap, readsPer, n_mapped);
  return fmap;
}

// The four per-read / per-line files: PREFIX.EM, .EM.reads2Taxon, .EM.reads2Taxon.krona, .EM.lengthAndIdentitiesPerMappingUnit.  Opened (and emptied)
// before anything is formatted, as the reference opens them.
struct PerReadText { std::string em, r2, kr, li; };
struct PerReadFiles {
  std::ofstream emf, r2t, kr, li;
  explicit PerReadFiles(const std::string& mapped)
      : emf(mapped + ".EM"), r2t(mapped + ".EM.reads2Taxon"), kr(mapped + ".EM.reads2Taxon.krona"), li(mapped + ".EM.lengthAndIdentitiesPerMappingUnit") {
    li << "AnalysisLevel\tID\treadI\tIdentity\tLength\n";
  }
  void put(const std::vector<PerReadText>& outs) {                // the ranges in read order, PREFIX.EM beside the three small ones
    auto one = [&](std::ofstream& f, std::string PerReadText::*m) { for (auto& O : outs) f.write((O.*m).data(), (std::streamsize)(O.*m).size()); };
    std::thread w1([&] { one(r2t, &PerReadText::r2); one(kr, &PerReadText::kr); one(li, &PerReadText::li); });
    one(emf, &PerReadText::em);
    w1.join();
  }
  void close() { emf.close(); r2t.close(); kr.close(); li.close(); }
};
// reads [r0, r1) of the four files (fEM.h:684-779); tax_nonx: getFirstNonXNode per taxon (taxonomy.h:51-74)
inline void format_reads(const ClassifyView& V, const std::vector<std::string>& tax_nonx, size_t r0, size_t r1, PerReadText& O) {
  const std::vector<MapLine>& lines = V.M.lines; const std::vector<int64_t>& off = V.M.off;
  if (r1 <= r0) return;
  { size_t bytes = 0; for (size_t i = (size_t)off[r0]; i < (size_t)off[r1]; ++i) bytes += lines[i].n + 5; O.em.reserve(bytes + 64); }
  char num[64];
  for (size_t r = r0; r < r1; ++r) {
    for (size_t i = (size_t)off[r]; i < (size_t)off[r + 1]; ++i) em_line(O.em, lines[i], V.E.post[i]);
    const size_t b = (size_t)V.E.best[r];
    const MapLine& B = lines[b];
    const std::string_view rid = read_id(B);
    O.li += "EqualCoverageUnit\t"; O.li += V.M.contig_id[(size_t)B.contig]; O.li += '\t';
    snprintf(num, sizeof num, "%zu\t%g\t%lld\n", r, B.ident, B.len); O.li += num;                  // :711
    O.r2 += rid; O.r2 += '\t'; O.r2 += V.C.taxa[(size_t)V.C.taxon[b]]; O.r2 += '\n';
    O.kr += rid; O.kr += '\t'; O.kr += tax_nonx[(size_t)V.C.taxon[b]];
    snprintf(num, sizeof num, "\t%g\n", V.E.post[b]); O.kr += num;
  }
}

// What the best mappings add up to, in read order: reads and identities per taxon (fEM.h:691, :718), the longest read (:692, :719-722), coverage windows
struct Tallies {
  std::map<std::string, size_t> readsPer; std::map<std::string, std::vector<double>> identsPerTaxon; long long maxReadLen = -1;
  ContigCoverage coverage;
};
// taxon and contig by index, strings only at the end; `HW`: the CPUs the process may keep busy
inline void tally_best_mappings(const ClassifyView& V, unsigned HW, Tallies& Y) {
  const std::vector<MapLine>& lines = V.M.lines; const std::vector<std::string>& taxa = V.C.taxa; const std::vector<long long>& clen = V.C.contig_len_ti;
  const size_t NRD = V.M.NRD;
  std::vector<size_t> readsPerIdx(taxa.size(), 0);
  std::vector<std::vector<double>> identsIdx(taxa.size());
  std::vector<ContigCoverage::Slot> cslot(V.M.contig_id.size());
  for (size_t r = 0; r < NRD; ++r) {                             // the window vectors of every contig with a best mapping (map insertions: one thread)
    const MapLine& B = lines[(size_t)V.E.best[r]];
    const size_t tx = (size_t)V.C.taxon[(size_t)V.E.best[r]];
    const std::string& cg = V.M.contig_id[(size_t)B.contig];
    Y.maxReadLen = std::max(Y.maxReadLen, B.len);
    if (clen[(size_t)B.contig] < 0) die("contig " + cg + " is not listed for taxon " + taxa[tx] + " in " + V.db + "/taxonInfo.txt");
    ContigCoverage::Slot& sl = cslot[(size_t)B.contig];
    if (!sl.v) sl = Y.coverage.slot(taxa[tx], cg, (size_t)clen[(size_t)B.contig]);
  }
  // thread k owns the taxa and the contigs with index % NT2 == k and walks the reads in order
  const size_t NT2 = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)std::max(1u, HW / 2), NRD / 20000 + 1}));
  on_each_caller_first(NT2, [&](size_t k) {
    for (size_t r = 0; r < NRD; ++r) {
      const size_t b = (size_t)V.E.best[r];
      const MapLine& B = lines[b];
      const size_t tx = (size_t)V.C.taxon[b];
      if (tx % NT2 == k) { readsPerIdx[tx]++; identsIdx[tx].push_back(B.ident); }
      if ((size_t)B.contig % NT2 == k) Y.coverage.add(cslot[(size_t)B.contig], (size_t)clen[(size_t)B.contig], B.start, B.stop);
    }
  });
  for (size_t t = 0; t < taxa.size(); ++t) if (readsPerIdx[t]) { Y.readsPer[taxa[t]] = readsPerIdx[t]; Y.identsPerTaxon[taxa[t]] = std::move(identsIdx[t]); }
}
// NTH ranges of reads with about as many lines each formatted by as many threads into their own buffers (4.2 M lines through std::to_string on one
// thread took 1.2 s); the calling thread takes the first range and then the tallies, while the others format
inline std::vector<PerReadText> format_and_tally(const ClassifyView& V, size_t NTH, unsigned HW, Tallies& Y) {
  const size_t NRD = V.M.NRD, NL = V.M.lines.size();
  std::vector<std::string> tax_nonx(V.C.taxa.size());
  for (size_t t = 0; t < V.C.taxa.size(); ++t) tax_nonx[t] = V.T.first_non_x(V.C.taxa[t]);
  std::vector<size_t> rcut(NTH + 1, NRD);
  rcut[0] = 0;
  { size_t t = 1; for (size_t r = 0; r < NRD && t < NTH; ++r) if ((uint64_t)V.M.off[r] >= (uint64_t)NL * t / NTH) rcut[t++] = r; }
  std::vector<PerReadText> outs(NTH);
  on_each_caller_first(NTH, [&](size_t t) { format_reads(V, tax_nonx, rcut[t], rcut[t + 1], outs[t]); if (t == 0) tally_best_mappings(V, HW, Y); });
  return outs;
}

// PREFIX.EM.reads2Taxon.lca: readID, taxon ID, rank and mass of the LCA assignment of every read with a mapping, in the order of reads2Taxon
inline void write_lca_reads(const std::string& fn, const ClassifyView& V, const LcaJob& J) {
  std::string out; char num[48];
  for (size_t r = 0; r < V.M.NRD; ++r) {
    const std::string& id = J.id[(size_t)J.node[r]];
    out += read_id(V.M.lines[(size_t)V.M.off[r]]); out += '\t'; out += id; out += '\t'; out += V.T.T.at(id).rank;
    snprintf(num, sizeof num, "\t%.6f\n", J.mass[r]); out += num;
  }
  write_text(fn, out);
}

// PREFIX.EM.WIMP.bootstrap: the WIMP's rows without the -3 count rows, its EMFrequency text, and over the replicates (each through cleanF with
// the point estimate's best-mapping tallies, then the WIMP's upward sums and per-level normalisation) mean, SD (n - 1), 2.5 % and 97.5 %
// quantiles, n = the replicates that drew a read (the bootstrap has seen to n >= 2).  `pres`, `boot_f`, `boot_empty`: see em_sharded.hpp's BootReplicates.
inline void write_bootstrap(const std::string& fn, const ClassifyView& V, const std::vector<int32_t>& pres, const std::vector<double>& boot_f, const std::vector<char>& boot_empty,
                            const std::map<std::string, double>& fmap, const std::map<std::string, size_t>& readsPer) {
  const size_t B = boot_empty.size(), NP = pres.size(), n_mapped = V.C.st.at("ReadsMapped");
  UpMemo memo;
  const std::map<std::string, WimpLevel> W0 = wimp_em_frequencies(V.T, fmap, readsPer, &memo);
  struct Row { const std::string* L; std::string t; double em; std::vector<double> v; };
  std::vector<Row> rows;
  for (auto& lv : W0) {
    double emUnm = 0;
    for (auto& t : lv.second.keys) { if (t != "Undefined") rows.push_back(Row{&lv.first, t, lv.second.emF.at(t), {}}); else emUnm += lv.second.emF.at(t); }
    rows.push_back(Row{&lv.first, "0", emUnm, {}});
  }
  for (auto& R : rows) R.v.reserve(B);
  for (size_t b = 0; b < B; ++b) {
    if (boot_empty[b]) continue;
    std::map<std::string, double> fm;                              // the replicate's frequencies of the taxa with a mapping (the others: 0, dropped)
    for (size_t j = 0; j < NP; ++j) fm[V.C.taxa[(size_t)pres[j]]] = boot_f[b * NP + j];
    clean_frequencies(fm, readsPer, n_mapped);
    const std::map<std::string, WimpLevel> Wb = wimp_em_frequencies(V.T, fm, readsPer, &memo);
    for (auto& R : rows) {
      auto lv = Wb.find(*R.L);
      double v = 0;
      if (lv != Wb.end()) {
        if (R.t == "0") { auto u = lv->second.emF.find("Undefined"); if (u != lv->second.emF.end()) v = u->second; }
        else { auto e = lv->second.emF.find(R.t); if (e != lv->second.emF.end()) v = e->second; }
      }
      R.v.push_back(v);
    }
  }
  std::ofstream o(fn);
  o << "AnalysisLevel\ttaxonID\tName\tEMFrequency\tBootstrapMean\tBootstrapSD\tLower95\tUpper95\n";
  char num[128];
  for (auto& R : rows) {
    const RowStats s = bootstrap_row_stats(R.v);
    snprintf(num, sizeof num, "\t%.6g\t%.6g\t%.6g\t%.6g\n", s.mean, s.sd, s.lo, s.hi);
    o << *R.L << "\t" << R.t << "\t" << (R.t == "0" ? std::string("Unclassified") : V.T.T.at(R.t).sci) << "\t" << R.em << num;
  }
}

// --min-identity: PREFIX.extractedIdentities and PREFIX.EM-filtered{,.reads2Taxon,.WIMP} from what mm_ident_filter returned (F), and the line of the log
inline void write_identity_filtered(const ClassifyView& V, const identf::Filter& F, const UnmappedTail& tail) {
  identf::write_identities(V.mapped + ".extractedIdentities", F, V.M.off, V.M.lines);
  std::string em, r2;
  std::vector<int64_t> kept(V.C.taxa.size(), 0);
  for (size_t r = 0; r < V.M.NRD; ++r) {
    const size_t b = (size_t)V.E.best[r];
    const MapLine& B = V.M.lines[b];
    r2 += read_id(B); r2 += '\t';
    if (F.read_removed[r]) r2 += '0';
    else { r2 += V.C.taxa[(size_t)V.C.taxon[b]]; em_line(em, B, V.E.post[b]); kept[(size_t)V.C.taxon[b]]++; }
    r2 += '\n';
  }
  write_text(V.mapped + ".EM-filtered", em);
  write_text(V.mapped + ".EM-filtered.reads2Taxon", r2 + tail.r2t);
  identf::write_filtered_wimp(V.mapped + ".EM-filtered.WIMP", V.T, V.C.taxa, kept, F.reads_removed(), V.C.nUnmapped, (size_t)F.n_with);
  char msg[256];
  snprintf(msg, sizeof msg, "Identity filter: threshold %g, median identity %g, %lld of %lld best identities at or below it, %zu of %zu genomes removed, %zu reads set to unclassified",
           F.thr, F.n_with ? F.sorted_max[(size_t)F.n_with / 2] : 0.0, (long long)F.n_le, (long long)F.n_with, F.genomes_removed(), F.genomes_hit(), F.reads_removed());
  std::cout << msg << std::endl;
}

// --refit: PREFIX.EM-filtered.refit (the kept lines with their new posteriors), .refit.reads2Taxon (a read that lost every mapping: 0) and .refit.WIMP
// (such reads count as unmapped).  tx: the taxon of every kept mapping; E2: the EM's result on the kept mappings (F.read_off_out, F.entry_src).
inline void write_refit(const ClassifyView& V, const identf::Filter& F, const std::vector<int32_t>& tx, const EmResult& E2, const UnmappedTail& tail, long long rounds) {
  const std::vector<std::string>& taxa = V.C.taxa;
  const size_t NR2 = (size_t)F.n_reads_out, lost = (size_t)F.n_with - NR2;
  std::string em, r2;
  std::vector<size_t> readsPerIdx(taxa.size(), 0);
  size_t k = 0;                                                  // the next kept read
  for (size_t r = 0; r < V.M.NRD; ++r) {
    r2 += read_id(V.M.lines[(size_t)V.M.off[r]]); r2 += '\t';
    if (k < NR2 && (size_t)F.read_src[k] == r) {
      for (size_t j = (size_t)F.read_off_out[k]; j < (size_t)F.read_off_out[k + 1]; ++j) em_line(em, V.M.lines[(size_t)F.entry_src[j]], E2.post[j]);
      const size_t t = (size_t)tx[(size_t)E2.best[k]];
      r2 += taxa[t]; readsPerIdx[t]++; ++k;
    } else r2 += '0';
    r2 += '\n';
  }
  write_text(V.mapped + ".EM-filtered.refit", em);
  write_text(V.mapped + ".EM-filtered.refit.reads2Taxon", r2 + tail.r2t);
  std::map<std::string, size_t> readsPer;
  for (size_t t = 0; t < taxa.size(); ++t) if (readsPerIdx[t]) readsPer[taxa[t]] = readsPerIdx[t];
  const std::map<std::string, double> fmap = cleaned_frequencies(taxa, E2.f, readsPer, NR2);   // (the kept reads as ReadsMapped)
  write_wimp(V.mapped + ".EM-filtered.refit.WIMP", V.T, fmap, readsPer, V.C.nTotal, V.C.nUnmapped + lost, V.C.nTooShort);
  std::cout << "Refit: " << NR2 << " reads, " << (size_t)F.n_entries_out << " mappings, " << lost << " reads lost every mapping, " << rounds << " EM iterations" << std::endl;
}

}  // namespace
