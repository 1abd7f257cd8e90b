// classify --genes, host side (DESIGN.md §4 "Gene-level analysis"; the reference does this in geneLevelAnalysis.pl): the two annotation tables of a
// DB directory as the arrays mm_gene_overlap takes, and the files written from its results.  No device call in here: tests/test_gene_annot.cpp
// compiles it alone.
//   DB_annotations.txt          tab-separated, columns by name (ContigId first; Start, Stop, GeneName, GeneLocusTag, CDSProteinId, CDSProduct), empty
//                               fields kept, empty lines skipped.  Only lines of relevant contigs (those that carry a best mapping) are kept.  Lines
//                               with the same GeneName//GeneLocusTag, on any contig, are one gene group; its ProteinId / Product: the last such line's.
//   DB_proteins.faa.annotated   tab-separated with a header; ProteinID, GO_terms, KEGG_KOs, BiGG_reactions, OGs, COG_cat by name; every line as many
//                               fields as the header; a field: whitespace removed, split at ',', values de-duplicated (empty values dropped)
//   PREFIX.EM.geneLevelAnalysis one row per group with a read, in the order of the groups' first kept lines
//   PREFIX.EM.proteins.TYPE     one row per supported value of GO / KEGG / BiGG / OG / COG, sorted by the value's bytes
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <numeric>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace gene {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

constexpr int N_TYPES = 5;
inline const char* type_name(int t) { static const char* const N[N_TYPES] = {"GO", "KEGG", "BiGG", "OG", "COG"}; return N[t]; }
inline const char* type_column(int t) { static const char* const N[N_TYPES] = {"GO_terms", "KEGG_KOs", "BiGG_reactions", "OGs", "COG_cat"}; return N[t]; }
inline std::string annotations_path(const std::string& db) { return db + "/DB_annotations.txt"; }
inline std::string proteins_path(const std::string& db) { return db + "/DB_proteins.faa.annotated"; }

// the 25 COG functional categories (NCBI COG); nullptr for any other value
inline const char* cog_long(const std::string& v) {
  static const std::map<std::string, const char*> M = {
      {"D", "Cell cycle control, cell division, chromosome partitioning"}, {"M", "Cell wall/membrane/envelope biogenesis"}, {"N", "Cell motility"},
      {"O", "Post-translational modification, protein turnover, and chaperones"}, {"T", "Signal transduction mechanisms"},
      {"U", "Intracellular trafficking, secretion, and vesicular transport"}, {"V", "Defense mechanisms"}, {"W", "Extracellular structures"},
      {"Y", "Nuclear structure"}, {"Z", "Cytoskeleton"}, {"A", "RNA processing and modification"}, {"B", "Chromatin structure and dynamics"},
      {"J", "Translation, ribosomal structure and biogenesis"}, {"K", "Transcription"}, {"L", "Replication, recombination and repair"},
      {"C", "Energy production and conversion"}, {"E", "Amino acid transport and metabolism"}, {"F", "Nucleotide transport and metabolism"},
      {"G", "Carbohydrate transport and metabolism"}, {"H", "Coenzyme transport and metabolism"}, {"I", "Lipid transport and metabolism"},
      {"P", "Inorganic ion transport and metabolism"}, {"Q", "Secondary metabolites biosynthesis, transport, and catabolism"},
      {"R", "General function prediction only"}, {"S", "Function unknown"}};
  auto it = M.find(v);
  return it == M.end() ? nullptr : it->second;
}

inline std::vector<std::string> split_tabs(const std::string& ln) {   // trailing empty fields kept
  std::vector<std::string> f;
  for (size_t a = 0;;) { const size_t b = ln.find('\t', a); f.push_back(ln.substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; }
  return f;
}
// index of every wanted column in the header line; -1 if absent
inline std::vector<int> columns(const std::vector<std::string>& header, std::initializer_list<const char*> want) {
  std::vector<int> ix;
  for (const char* w : want) { auto it = std::find(header.begin(), header.end(), w); ix.push_back(it == header.end() ? -1 : (int)(it - header.begin())); }
  return ix;
}
inline int32_t position(const std::string& s, const std::string& file, size_t line_no) {
  char* end = nullptr;
  const long long v = strtoll(s.c_str(), &end, 10);
  if (s.empty() || *end || v < INT32_MIN || v > INT32_MAX) throw Error(file + " line " + std::to_string(line_no) + ": '" + s + "' is not a position");
  return (int32_t)v;
}

struct Group { std::string name, locus, protein, product; };
struct Annotations {
  // genes of the relevant contigs, sorted by (contig, Start); contig c: the index the caller gave the contig
  std::vector<int64_t> contig_gene_off; std::vector<int32_t> start, stop, group;
  std::vector<Group> groups;                                      // in the order of their first kept line
  size_t n_contigs_annotated = 0;
  std::set<std::string> known_proteins;                           // CDSProteinId of every line of the file
  // features: the values of the five annotation types that the groups' proteins carry
  std::vector<std::string> feat_name; std::vector<int> feat_type;
  std::vector<int64_t> group_feat_off{0}; std::vector<int32_t> group_feat;
  std::set<std::string> annotated_proteins;                       // relevant proteins with at least one annotation value
  size_t n_protein_lines = 0, n_proteins_absent = 0;              // lines of the protein table; those whose protein is in no line of DB_annotations.txt
};

// DB_annotations.txt: the lines of the contigs in `relevant` (contig ID -> index in 0 .. n_contigs-1)
inline void read_annotations(const std::string& path, const std::unordered_map<std::string, int>& relevant, size_t n_contigs, Annotations& A) {
  std::ifstream in(path);
  if (!in.is_open()) throw Error("Please supply a gene-annotated database (file " + path + " not found).");
  std::string ln;
  if (!std::getline(in, ln)) throw Error(path + " is empty");
  const std::vector<std::string> header = split_tabs(ln);
  if (header[0] != "ContigId") throw Error(path + ": the header's first field is not ContigId");
  const std::vector<int> col = columns(header, {"Start", "Stop", "GeneName", "GeneLocusTag", "CDSProteinId", "CDSProduct"});
  for (size_t i = 0; i < col.size(); ++i) if (col[i] < 0) throw Error(path + ": the header lacks one of Start, Stop, GeneName, GeneLocusTag, CDSProteinId, CDSProduct");
  struct Gene { int contig; int32_t start, stop, group; };
  std::vector<Gene> genes;
  std::unordered_map<std::string, int32_t> group_of;
  for (size_t line_no = 2; std::getline(in, ln); ++line_no) {
    if (ln.empty()) continue;
    const std::vector<std::string> f = split_tabs(ln);
    auto at = [&](int c) -> const std::string& { static const std::string none; return (size_t)c < f.size() ? f[(size_t)c] : none; };
    A.known_proteins.insert(at(col[4]));
    auto rc = relevant.find(f[0]);
    if (rc == relevant.end()) continue;
    const int32_t s = position(at(col[0]), path, line_no), e = position(at(col[1]), path, line_no);
    if (e < s) throw Error(path + " line " + std::to_string(line_no) + ": Stop lies before Start");
    const std::string id = at(col[2]) + "//" + at(col[3]);
    auto g = group_of.find(id);
    if (g == group_of.end()) { g = group_of.emplace(id, (int32_t)A.groups.size()).first; A.groups.push_back(Group{at(col[2]), at(col[3]), "", ""}); }
    A.groups[(size_t)g->second].protein = at(col[4]); A.groups[(size_t)g->second].product = at(col[5]);
    genes.push_back(Gene{rc->second, s, e, g->second});
  }
  std::stable_sort(genes.begin(), genes.end(), [](const Gene& a, const Gene& b) { return a.contig != b.contig ? a.contig < b.contig : a.start < b.start; });
  A.contig_gene_off.assign(n_contigs + 1, 0);
  for (const Gene& g : genes) A.contig_gene_off[(size_t)g.contig + 1]++;
  for (size_t c = 0; c < n_contigs; ++c) { A.n_contigs_annotated += A.contig_gene_off[c + 1] > 0; A.contig_gene_off[c + 1] += A.contig_gene_off[c]; }
  for (const Gene& g : genes) { A.start.push_back(g.start); A.stop.push_back(g.stop); A.group.push_back(g.group); }
}

// the values of one annotation field: whitespace removed, split at ',', de-duplicated
inline std::vector<std::string> field_values(const std::string& field) {
  std::string s;
  for (char ch : field) if (!isspace((unsigned char)ch)) s += ch;
  std::set<std::string> v;
  for (size_t a = 0; a <= s.size();) { const size_t b = std::min(s.find(',', a), s.size()); if (b > a) v.insert(s.substr(a, b - a)); a = b + 1; }
  return std::vector<std::string>(v.begin(), v.end());
}

// DB_proteins.faa.annotated: the features of the groups' proteins (behind read_annotations)
inline void read_proteins(const std::string& path, Annotations& A) {
  std::ifstream in(path);
  if (!in.is_open()) throw Error("Please supply a protein annotation file (file " + path + " not found).");
  std::string ln;
  if (!std::getline(in, ln)) throw Error(path + " is empty");
  const std::vector<std::string> header = split_tabs(ln);
  const std::vector<int> col = columns(header, {"ProteinID", type_column(0), type_column(1), type_column(2), type_column(3), type_column(4)});
  for (size_t i = 0; i < col.size(); ++i) if (col[i] < 0) throw Error(path + ": the header lacks one of ProteinID, GO_terms, KEGG_KOs, BiGG_reactions, OGs, COG_cat");
  std::set<std::string> relevant;
  for (const Group& g : A.groups) if (!g.protein.empty()) relevant.insert(g.protein);
  std::map<std::pair<int, std::string>, int32_t> feat_of;
  std::unordered_map<std::string, std::vector<int32_t>> feats_of_protein;
  for (size_t line_no = 2; std::getline(in, ln); ++line_no) {
    if (ln.empty()) continue;
    const std::vector<std::string> f = split_tabs(ln);
    if (f.size() != header.size()) throw Error(path + " line " + std::to_string(line_no) + ": " + std::to_string(f.size()) + " fields, the header has " + std::to_string(header.size()));
    const std::string& id = f[(size_t)col[0]];
    if (id.empty()) throw Error(path + " line " + std::to_string(line_no) + ": empty ProteinID");
    ++A.n_protein_lines;
    if (!A.known_proteins.count(id)) ++A.n_proteins_absent;
    if (!relevant.count(id)) continue;
    if (feats_of_protein.count(id)) throw Error(path + " line " + std::to_string(line_no) + ": protein " + id + " is annotated more than once");
    std::vector<int32_t>& mine = feats_of_protein[id];
    for (int t = 0; t < N_TYPES; ++t)
      for (const std::string& v : field_values(f[(size_t)col[(size_t)t + 1]])) {
        auto it = feat_of.find({t, v});
        if (it == feat_of.end()) { it = feat_of.emplace(std::make_pair(t, v), (int32_t)A.feat_name.size()).first; A.feat_name.push_back(v); A.feat_type.push_back(t); }
        mine.push_back(it->second);
      }
    if (!mine.empty()) A.annotated_proteins.insert(id);
  }
  A.group_feat_off.assign(1, 0);
  for (const Group& g : A.groups) {
    auto it = g.protein.empty() ? feats_of_protein.end() : feats_of_protein.find(g.protein);
    if (it != feats_of_protein.end()) A.group_feat.insert(A.group_feat.end(), it->second.begin(), it->second.end());
    A.group_feat_off.push_back((int64_t)A.group_feat.size());
  }
}

struct Results { std::vector<int64_t> group_reads; std::vector<double> group_median; std::vector<int64_t> feat_reads; int64_t maps_on_annotated = 0; };

inline void write_gene_table(const std::string& fn, const Annotations& A, const Results& R) {
  std::string out = "GeneName\tGeneLocusTag\tProteinId\tProduct\tnReads\tmedianIdentity\n";
  char num[64];
  for (size_t g = 0; g < A.groups.size(); ++g) {
    if (R.group_reads[g] < 1) continue;
    const Group& G = A.groups[g];
    out += G.name; out += '\t'; out += G.locus; out += '\t'; out += G.protein; out += '\t'; out += G.product;
    snprintf(num, sizeof num, "\t%lld\t%.15g\n", (long long)R.group_reads[g], R.group_median[g]); out += num;
  }
  std::ofstream o(fn);
  o.write(out.data(), (std::streamsize)out.size());
  if (!o) throw Error("Cannot write " + fn);
}
// PREFIX.EM.proteins.TYPE for every type with a supported value; the files' names
inline std::vector<std::string> write_protein_tables(const std::string& em_prefix, const Annotations& A, const Results& R, size_t n_reads) {
  std::vector<std::string> written;
  for (int t = 0; t < N_TYPES; ++t) {
    std::vector<size_t> rows;
    for (size_t f = 0; f < A.feat_name.size(); ++f) if (A.feat_type[f] == t && R.feat_reads[f] > 0) rows.push_back(f);
    if (rows.empty()) continue;
    std::sort(rows.begin(), rows.end(), [&](size_t a, size_t b) { return A.feat_name[a] < A.feat_name[b]; });
    const bool cog = strcmp(type_name(t), "COG") == 0;
    std::string out = cog ? "Feature\tSupportByReads\tSupportByReadsProportionTotalReads\tFeatureLong\n" : "Feature\tSupportByReads\tSupportByReadsProportionTotalReads\n";
    char num[64];
    for (size_t f : rows) {
      if (cog && !cog_long(A.feat_name[f])) throw Error("Unknown COG category " + A.feat_name[f]);
      out += A.feat_name[f];
      snprintf(num, sizeof num, "\t%lld\t%.15g", (long long)R.feat_reads[f], (double)R.feat_reads[f] / (double)n_reads); out += num;
      if (cog) { out += '\t'; out += cog_long(A.feat_name[f]); }
      out += '\n';
    }
    const std::string fn = em_prefix + ".proteins." + type_name(t);
    std::ofstream o(fn);
    o.write(out.data(), (std::streamsize)out.size());
    if (!o) throw Error("Cannot write " + fn);
    written.push_back(fn);
  }
  return written;
}
// genes with a read, their proteins, and how many of those carry an annotation
inline void found_counts(const Annotations& A, const Results& R, size_t* genes, size_t* proteins, size_t* annotated) {
  std::set<std::string> seen;
  *genes = 0;
  for (size_t g = 0; g < A.groups.size(); ++g) if (R.group_reads[g] > 0) { ++*genes; if (!A.groups[g].protein.empty()) seen.insert(A.groups[g].protein); }
  *proteins = seen.size(); *annotated = 0;
  for (const std::string& p : seen) *annotated += A.annotated_proteins.count(p);
}

}  // namespace gene
