// Host harness of metamaps_amd/csrc/host/gene_annot.hpp for tests/test_gene_annot.py (g++, plain and with the address / undefined-behaviour sanitizers):
// the parsers of a DB directory's two annotation tables and the writers of classify --genes' files, without a device — the overlaps are found on one
// host thread through mm_gene_core.hpp.
//   test_gene_annot DB_DIR OUT_PREFIX < best mappings, one per line: contigID <tab> start <tab> stop <tab> bit pattern of the identity
// Writes OUT_PREFIX.geneLevelAnalysis and OUT_PREFIX.proteins.TYPE; prints the numbers of the CLI's messages.  A gene::Error: "ERROR: text", exit 1.
#include "../metamaps_amd/csrc/host/gene_annot.hpp"
#include "../metamaps_amd/csrc/mm_gene_core.hpp"
#include <iostream>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string db = argv[1], prefix = argv[2];
  std::unordered_map<std::string, int> relevant;
  std::vector<int32_t> mc, ms, me; std::vector<double> mi;
  for (std::string ln; std::getline(std::cin, ln);) {
    const std::vector<std::string> f = gene::split_tabs(ln);
    if (f.size() != 4) return 2;
    auto it = relevant.find(f[0]);
    if (it == relevant.end()) it = relevant.emplace(f[0], (int)relevant.size()).first;
    const unsigned long long bits = strtoull(f[3].c_str(), nullptr, 10);
    double x; memcpy(&x, &bits, 8);
    mc.push_back(it->second); ms.push_back(atoi(f[1].c_str())); me.push_back(atoi(f[2].c_str())); mi.push_back(x);
  }
  try {
    gene::Annotations A;
    gene::read_annotations(gene::annotations_path(db), relevant, relevant.size(), A);
    gene::read_proteins(gene::proteins_path(db), A);
    const int nc = (int)relevant.size();
    int bad = mm::gene_table_check(nc, A.contig_gene_off.data(), A.start.data(), A.stop.data(), A.group.data(), (int64_t)A.groups.size(), A.group_feat_off.data(),
                                   A.group_feat.data(), (int64_t)A.feat_name.size());
    if (!bad) bad = mm::gene_maps_check((int64_t)mc.size(), mc.data(), ms.data(), me.data(), mi.data(), nc);
    if (bad) throw gene::Error(mm::gene_arg_message(bad));
    std::vector<int32_t> pmax(A.start.size());
    mm::gene_prefix_max(nc, A.contig_gene_off.data(), A.stop.data(), pmax.data());
    const mm::GeneTable T{A.contig_gene_off.data(), A.start.data(), A.stop.data(), pmax.data()};
    gene::Results R;
    R.group_reads.assign(A.groups.size(), 0); R.group_median.assign(A.groups.size(), NAN); R.feat_reads.assign(A.feat_name.size(), 0);
    std::vector<std::vector<double>> idents(A.groups.size());
    std::vector<int64_t> hits(A.start.size() + 1);
    for (size_t m = 0; m < mc.size(); ++m) {
      R.maps_on_annotated += A.contig_gene_off[(size_t)mc[m] + 1] > A.contig_gene_off[(size_t)mc[m]];
      int64_t lo, hi; mm::gene_span(T, mc[m], ms[m], me[m], &lo, &hi);
      mm::GeneEmit em{hits.data()};
      mm::gene_stab(mm::GeneSerial{}, T, lo, hi, ms[m], em);
      std::set<int32_t> mine;
      for (int64_t k = 0; k < em.at; ++k) {
        const size_t g = (size_t)A.group[(size_t)hits[(size_t)k]];
        R.group_reads[g]++; idents[g].push_back(mi[m]);
        mine.insert(A.group_feat.begin() + A.group_feat_off[g], A.group_feat.begin() + A.group_feat_off[g + 1]);
      }
      for (int32_t f : mine) R.feat_reads[(size_t)f]++;
    }
    for (size_t g = 0; g < idents.size(); ++g) if (!idents[g].empty()) { std::sort(idents[g].begin(), idents[g].end()); R.group_median[g] = idents[g][(idents[g].size() - 1) / 2]; }
    gene::write_gene_table(prefix + ".geneLevelAnalysis", A, R);
    const std::vector<std::string> written = gene::write_protein_tables(prefix, A, R, mc.size());
    size_t n_genes, n_prot, n_annot;
    gene::found_counts(A, R, &n_genes, &n_prot, &n_annot);
    std::cout << "relevant " << relevant.size() << " annotated " << A.n_contigs_annotated << " reads " << mc.size() << " on " << R.maps_on_annotated << " genes " << n_genes
              << " proteins " << n_prot << " annotated_proteins " << n_annot << " protein_lines " << A.n_protein_lines << " absent " << A.n_proteins_absent << " files " << written.size() << "\n";
  } catch (const gene::Error& e) { std::cout << "ERROR: " << e.what() << "\n"; return 1; }
  return 0;
}
