// The host arithmetic of `classify` that needs no device: the NCBI taxonomy, the taxon of a contig, the WIMP's frequencies, the coverage windows,
// the binomial tail of the unknown-species evidence, the tree of the LCA assignment and its Kraken-style report, and how classify reads a mapping
// quality.  The standard library only (no C ABI, no device context): tests/test_cli_units.cpp compiles this on its own.
#pragma once
#include "../cpu_budget.hpp"
#include "cli_common.hpp"
#include "fast_format.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <set>

namespace {

struct TaxNode { std::string parent, rank, sci; };
struct Taxonomy {                                                // meta/taxonomy.h:137-246
  std::map<std::string, TaxNode> T;
  // split(regex_replace(line, "\\s*\\|\\s*", "|"), "|") of taxonomy.h:150-175 without std::regex: cut at every '|', drop the white space
  // that touches a '|' (not the one at the very start or end of the line)
  static std::vector<std::string> fields(const std::string& ln) {
    std::vector<std::string> out;
    if (ln.empty()) return out;
    size_t a = 0;
    for (bool first = true;; first = false) {
      const size_t bar = ln.find('|', a);
      size_t lo = a, hi = bar == std::string::npos ? ln.size() : bar;
      if (!first) while (lo < hi && isspace((unsigned char)ln[lo])) ++lo;
      if (bar != std::string::npos) while (hi > lo && isspace((unsigned char)ln[hi - 1])) --hi;
      out.push_back(ln.substr(lo, hi - lo));
      if (bar == std::string::npos) break;
      a = bar + 1;
    }
    return out;
  }
  explicit Taxonomy(const std::string& dir) {
    std::map<std::string, std::string> sci; std::string ln;
    std::ifstream nm(dir + "/names.dmp"); if (!nm.is_open()) die("Cannot open file " + dir + "/names.dmp -- is '" + dir + "' a valid NCBI taxonomy?");
    while (std::getline(nm, ln)) {
      if (ln.empty()) continue;
      auto f = fields(ln);
      if (f.size() > 3 && f[3] == "scientific name") sci[f[0]] = f[1]; else if (f.size() > 3 && f[3] == "genbank common name") sci[f[0]];
    }
    std::ifstream nd(dir + "/nodes.dmp"); if (!nd.is_open()) die("Cannot open file " + dir + "/nodes.dmp");
    while (std::getline(nd, ln)) {
      if (ln.empty()) continue;
      auto f = fields(ln);
      if (!sci.count(f[0])) die("No name for taxon ID " + f[0] + " in taxonomy directory " + dir);
      T[f[0]] = TaxNode{f[1], f[2], sci[f[0]]};
    }
    std::cout << "Read taxonomy from " << dir << " -- have " << T.size() << " nodes." << std::endl;
  }
  std::map<std::string, std::string> upward_by_ranks(std::string id, const std::set<std::string>& want) const {   // taxonomy.h:76-111
    std::map<std::string, std::string> r;
    std::vector<std::string> up{id};
    while (id != "1") { id = T.at(id).parent; up.push_back(id); }
    for (auto& n : up) {
      const std::string& rank = T.at(n).rank;
      if (!want.count(rank)) continue;
      if (rank != "no rank") { if (r.count(rank)) die("Node " + up[0] + " has multiple entries for rank " + rank); r[rank] = n; }
    }
    for (auto& w : want) if (!r.count(w)) r[w] = "Undefined";
    return r;
  }
  std::string first_non_x(std::string id) const { while (id.find('x') != std::string::npos) id = T.at(id).parent; return id; }   // :51-74
};

// first match of the reference's regex  kraken:taxid\|(x?\d+)  (fEM.h:1396), without std::regex (called per mapping line)
std::string extract_taxon(const std::string& contig) {
  static const std::string key = "kraken:taxid|";
  for (size_t p = contig.find(key); p != std::string::npos; p = contig.find(key, p + 1)) {
    size_t a = p + key.size(), b = a;
    if (b < contig.size() && contig[b] == 'x') ++b;
    const size_t d0 = b;
    while (b < contig.size() && contig[b] >= '0' && contig[b] <= '9') ++b;
    if (b > d0) return contig.substr(a, b - a);
  }
  die("Could not extract taxon ID from contig identifier '" + contig + "' - did you use the MetMaps build scripts to construct your database?");
}

// a mapping quality as `classify` parses the text of field 14 (what mapDirectly --then-classify keeps beside the lines it writes)
static double mapq_as_classify_reads_it(const char* p, size_t n) {
  double v;
  if (parse_g6_text(p, n, &v)) return v;
  const std::string t(p, n);
  errno = 0; v = strtod(t.c_str(), nullptr);
  // (std::stod throws on a denormal; the reference then takes 0, fEM.h:269-275 — an overflow cannot be printed by this program)
  if (errno == ERANGE) v = t.find("e-") != std::string::npos ? 0.0 : v;
  return v;
}

// The EMFrequency column of the WIMP (fEM.h:52-215): the frequencies go up the taxonomy (a sum above 1 is cut to 1 on the way), and per
// level every taxon with a frequency or with reads (the level's keys, in order) gets its frequency over the level's sum.  The bootstrap
// file puts every replicate through the same steps.  `up_memo` (optional) keeps the upward paths of the taxa between calls.
struct WimpLevel { std::set<std::string> keys; std::map<std::string, double> emF; };
using UpMemo = std::map<std::string, std::map<std::string, std::string>>;
std::map<std::string, WimpLevel> wimp_em_frequencies(const Taxonomy& T, const std::map<std::string, double>& freq, const std::map<std::string, size_t>& reads,
                                                     UpMemo* up_memo = nullptr) {
  static const std::set<std::string> levels{"species", "genus", "family", "order", "phylum", "superkingdom"};
  auto upward = [&](const std::string& id) {
    if (up_memo) { auto it = up_memo->find(id); if (it != up_memo->end()) return it->second; }
    auto up = T.upward_by_ranks(id, levels); up["definedGenomes"] = id;
    if (up_memo) (*up_memo)[id] = up;
    return up;
  };
  std::map<std::string, WimpLevel> W;
  std::map<std::string, std::map<std::string, double>> fL;
  for (auto& kv : freq) for (auto& u : upward(kv.first)) { fL[u.first][u.second] += kv.second; W[u.first].keys.insert(u.second); if (fL[u.first][u.second] > 1) fL[u.first][u.second] = 1; }
  for (auto& kv : reads) for (auto& u : upward(kv.first)) W[u.first].keys.insert(u.second);
  for (auto& lv : W) {
    const std::string& L = lv.first; double sumF = 0;
    for (auto& t : lv.second.keys) { double f = fL[L].count(t) ? fL[L][t] : 0; sumF += f; fL[L][t] = f; }
    for (auto& t : lv.second.keys) lv.second.emF[t] = fL[L][t] / sumF;
  }
  return W;
}

// cleanF (fEM.h:1135-1163): taxa whose frequency lies below 0.9 of one read's share of the n_mapped reads and that no read has as its best mapping are
// dropped, the rest made to sum to 1 (added in the map's order)
void clean_frequencies(std::map<std::string, double>& f, const std::map<std::string, size_t>& readsPer, size_t n_mapped) {
  const double minF = 0.9 * (1.0 / (double)n_mapped);
  for (auto it = f.begin(); it != f.end();) if (it->second < minF && !readsPer.count(it->first)) it = f.erase(it); else ++it;
  double s = 0; for (auto& e : f) s += e.second; for (auto& e : f) e.second /= s;
}

void write_wimp(const std::string& fn,const Taxonomy& T, const std::map<std::string, double>& freq, const std::map<std::string, size_t>& reads,
                size_t nTotal, size_t nUnmapped, size_t nTooShort) {   // fEM.h:52-215
  const std::set<std::string> levels{"species", "genus", "family", "order", "phylum", "superkingdom"};
  std::map<std::string, WimpLevel> W = wimp_em_frequencies(T, freq, reads);
  std::map<std::string, std::map<std::string, double>> fL; std::map<std::string, std::map<std::string, size_t>> rL;
  for (auto& kv : reads) { auto up = T.upward_by_ranks(kv.first, levels); up["definedGenomes"] = kv.first;
    for (auto& u : up) rL[u.first][u.second] += kv.second; }
  const long long nMappable = (long long)nTotal - (long long)nTooShort, nMapped = nMappable - (long long)nUnmapped;
  std::ofstream o(fn);
  o << "AnalysisLevel\ttaxonID\tName\tAbsolute\tEMFrequency\tPotFrequency\n";
  for (auto& lv : W) {
    const std::string& L = lv.first; std::map<std::string, double>& emF = lv.second.emF;
    for (auto& t : lv.second.keys) { size_t r = rL[L].count(t) ? rL[L][t] : 0; rL[L][t] = r; fL[L][t] = emF[t]; }
    const double propMapped = (double)nMapped / nMappable; double propNot = (double)nUnmapped / nMappable;
    for (auto& t : lv.second.keys) fL[L][t] *= propMapped;
    double emUnm = 0; size_t nUnmUndef = nUnmapped;
    for (auto& t : lv.second.keys) {
      if (t != "Undefined") o << L << "\t" << t << "\t" << T.T.at(t).sci << "\t" << rL[L][t] << "\t" << emF[t] << "\t" << fL[L][t] << "\n";
      else { nUnmUndef += rL[L][t]; emUnm += emF[t]; propNot += fL[L][t]; }
    }
    o << L << "\t" << 0 << "\tUnclassified\t" << nUnmUndef << "\t" << emUnm << "\t" << propNot << "\n";
    o << L << "\t" << -3 << "\ttotalReads\t" << nTotal << "\t" << 0 << "\t" << 0 << "\n";
    o << L << "\t" << -3 << "\treadsLongEnough\t" << nMappable << "\t" << 0 << "\t" << 0 << "\n";
    o << L << "\t" << -3 << "\treadsLongEnough_unmapped\t" << nUnmapped << "\t" << 0 << "\t" << 0 << "\n";
  }
}

// .EM.contigCoverage: bases of best mappings per 1000-bp window of every contig that carries one (fEM.h:684, :730-776,
// :805-845).  Kept as the reference computes it, including the length it assigns to the last window of a contig that is
// not a multiple of the window size (:744 subtracts after incrementing the window count, so the unsigned value wraps).
struct ContigCoverage {
  const size_t W = 1000;
  std::map<std::string, std::map<std::string, std::vector<size_t>>> cov, reads;   // bases / best mappings per window
  std::map<std::string, std::map<std::string, size_t>> last;
  struct Slot { std::vector<size_t>* v = nullptr; std::vector<size_t>* nr = nullptr; };   // the two window vectors of a contig (map nodes do not move)
  Slot slot(const std::string& tx, const std::string& cg, size_t L) {
    auto& per = cov[tx];
    if (!per.count(cg)) {
      size_t n = L / W;
      if (n == 0) { n = 1; last[tx][cg] = L; }
      else if (n * W != L) { ++n; last[tx][cg] = L - n * W; }
      else last[tx][cg] = W;
      per[cg].assign(n, 0);
      reads[tx][cg].assign(n, 0);
    }
    return Slot{&per[cg], &reads[tx][cg]};
  }
  void add(const std::string& tx, const std::string& cg, size_t L, size_t start, size_t stop_in) { add(slot(tx, cg, L), L, start, stop_in); }
  void add(const Slot& sl, size_t L, size_t start, size_t stop_in) {
    const size_t stop = stop_in >= L ? L - 1 : stop_in;
    std::vector<size_t>& v = *sl.v;
    std::vector<size_t>& nr = *sl.nr;
    for (size_t p = start; p <= stop; p += W) {
      const size_t wi = p / W, ws = wi * W;
      size_t we = (wi + 1) * W - 1;
      if (we > L) we = L - 1;
      v.at(wi) += iv_overlap(ws, we, start, stop);
      nr.at(wi)++;
    }
  }
  void write(const std::string& fn, const Taxonomy& T) const {   // fEM.h:805-832; one line per 1000-base window of every contig with a best mapping: contigs formatted by several threads
    std::ofstream o(fn);
    o << "taxonID\tequalCoverageUnitLabel\tcontigID\tstart\tstop\tnBases\treadCoverage\n";
    struct Item { const std::string* tx; const std::string* sci; const std::string* cg; const std::vector<size_t>* v; size_t last; };
    std::vector<Item> items;
    for (auto& t : cov) for (auto& c : t.second) items.push_back(Item{&t.first, &T.T.at(t.first).sci, &c.first, &c.second, last.at(t.first).at(c.first)});
    std::vector<std::string> txt(items.size());
    std::atomic<size_t> nx{0};
    auto work = [&] {
      for (;;) {
        const size_t i = nx.fetch_add(1);
        if (i >= items.size()) return;
        const Item& it = items[i]; std::string& s = txt[i];
        s.reserve(it.v->size() * (it.tx->size() + it.sci->size() + it.cg->size() + 40));
        for (size_t wi = 0; wi < it.v->size(); ++wi) {
          const size_t wl = wi + 1 == it.v->size() ? it.last : W;
          s += *it.tx; s += '\t'; s += *it.sci; s += '\t'; s += *it.cg; s += '\t'; append_uint(s, wi * W); s += '\t'; append_uint(s, (wi + 1) * W - 1); s += '\t';
          append_uint(s, (*it.v)[wi]); s += '\t'; append_g6(s, (double)(*it.v)[wi] / (double)wl); s += '\n';
        }
      }
    };
    std::vector<std::thread> pool;
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)std::max(1u, mm::cpu_budget() / 4), items.size()}));
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    for (auto& s : txt) o.write(s.data(), (std::streamsize)s.size());
  }
};

// Regularised incomplete beta I_x(a, b) by the continued fraction (modified Lentz), used for the binomial tail below.
double reg_inc_beta(double a, double b, double x) {
  if (x <= 0) return 0;
  if (x >= 1) return 1;
  if (x > (a + 1) / (a + b + 2)) return 1 - reg_inc_beta(b, a, 1 - x);
  const double lead = std::exp(std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x)) / a;
  const double tiny = 1e-300;
  double f = 1, c = 1, d = 0;
  for (int i = 0; i <= 100000; ++i) {
    const int m = i / 2;
    double num;
    if (i == 0) num = 1;
    else if (i % 2 == 0) num = (m * (b - m) * x) / ((a + 2.0 * m - 1) * (a + 2.0 * m));
    else num = -((a + m) * (a + b + m) * x) / ((a + 2.0 * m) * (a + 2.0 * m + 1));
    d = 1 + num * d; if (std::fabs(d) < tiny) d = tiny; d = 1 / d;
    c = 1 + num / c; if (std::fabs(c) < tiny) c = tiny;
    const double cd = c * d;
    f *= cd;
    if (std::fabs(1 - cd) < 1e-16) break;
  }
  return lead * (f - 1);
}
// P(X <= k), X ~ Binomial(n, p)  (boost::math::cdf(binomial_distribution, k), fEM.h:1107)
double binomial_cdf(double n, double p, double k) {
  if (k >= n || p <= 0) return 1;
  if (p >= 1) return 0;
  return reg_inc_beta(n - k, k + 1, 1 - p);
}

// .EM.evidenceUnknownSpecies (fEM.h:846-1132): per taxon with best mappings, (1) a one-degree-of-freedom chi-square test of
// the share of its reads whose identity lies in the bottom third of the best-identity taxon's distribution, (2) the
// number of zero-coverage windows among the "usable" ones (at least a maximum read length of N-poor windows on both
// sides; N counts per 1000-bp window come from DBDIR/contigNstats_windowSize_1000.txt, :1421-1470) against a Poisson
// expectation.  Integer arithmetic as in the reference (size_t, including the wrapped last-window length kept by
// ContigCoverage).  The reference asserts when the contigNstats file is missing (:1427) or an expected count is zero
// (:1049-1050): here the file is skipped with a warning, respectively the row's identity columns are "NA".
bool write_unknown_species(const std::string& fn, const std::string& db, const Taxonomy& T, const ContigCoverage& C,
                           const std::map<std::string, std::vector<double>>& idents, long long maxReadLen, size_t minReads) {
  std::ifstream ns(db + "/contigNstats_windowSize_" + std::to_string(C.W) + ".txt");
  if (!ns.is_open()) return false;
  struct PerTaxon { size_t windows = 0, usable = 0, usableReads = 0, usableZero = 0; };
  std::map<std::string, PerTaxon> G;
  std::set<std::string> seenContigs;
  const size_t need = (size_t)maxReadLen;
  std::string ln;
  while (std::getline(ns, ln)) {
    while (!ln.empty() && (ln.back() == '\r' || ln.back() == '\n')) ln.pop_back();
    if (ln.empty()) continue;
    auto fl = split(ln, "\t");
    if (fl.size() != 3) die("Format error " + db + "/contigNstats_windowSize_1000.txt; wrong number of fields:\n" + ln);
    auto ct = C.cov.find(fl[0]);
    if (ct == C.cov.end() || !ct->second.count(fl[1])) continue;
    if (!seenContigs.insert(fl[1]).second) die("contigNstats: duplicate contig " + fl[1]);
    const std::vector<size_t>& nreads = C.reads.at(fl[0]).at(fl[1]);
    auto nf = split(fl[2], ";");
    if (nf.size() != nreads.size()) die("contigNstats: " + fl[1] + " has " + std::to_string(nf.size()) + " windows, expected " + std::to_string(nreads.size()));
    const size_t nw = nf.size(), lastLen = C.last.at(fl[0]).at(fl[1]);
    std::vector<uint8_t> poor(nw);                               // window has <= 2 % N
    for (size_t i = 0; i < nw; ++i) poor[i] = (double)std::stoull(nf[i]) / (double)(i + 1 == nw ? lastLen : C.W) <= 0.02;
    std::vector<size_t> before(nw), after(nw);                   // N-poor bases running up to / following each window
    size_t run = 0;
    for (size_t i = 0; i < nw; ++i) { before[i] = run; if (poor[i]) run += i + 1 == nw ? lastLen : C.W; else run = 0; }
    run = 0;
    for (size_t i = nw; i-- > 0;) { after[i] = run; if (poor[i]) run += i + 1 == nw ? lastLen : C.W; else run = 0; }
    PerTaxon& g = G[fl[0]];
    g.windows += nw;
    for (size_t i = 0; i < nw; ++i) if (before[i] >= need && after[i] >= need) { ++g.usable; g.usableReads += nreads[i]; g.usableZero += nreads[i] == 0; }
  }
  for (auto& t : C.cov) for (auto& c : t.second) if (!seenContigs.count(c.first)) die("Missing entry " + c.first + " in " + db + "/contigNstats_windowSize_1000.txt");

  // reference distribution: the taxon with the highest median identity among those with enough reads (:846-890)
  bool haveRef = false; double refMedian = 0, cut = 0, cutP = 0;
  for (auto& e : idents) {
    if (e.second.size() < 3 || e.second.size() < minReads) continue;
    std::vector<double> v = e.second; std::sort(v.begin(), v.end());
    const double med = v[v.size() / 2];
    if (haveRef && !(med > refMedian)) continue;
    haveRef = true; refMedian = med;
    cut = v.at((size_t)(v.size() * (1.0 / 3.0)));
    cutP = (double)(std::upper_bound(v.begin(), v.end(), cut) - v.begin()) / (double)v.size();
  }

  std::ofstream o(fn);
  o << "taxonID\tspecies\tgenus\tnReads\tpropBottomThirdReadIdentities\texpectedPropBottomThirdReadIdentities\tpValue_BottomThirdReadIdentities\t"
       "coverageWindows_totalGenome\tcoverageWindows_usable\tcoverageWindows_usable_averageCoverage\tcoverageWindows_usable_coverageIsZero\t"
       "coverageWindows_usable_coverageIsZero_expected\tcoverageWindows_usable_coverageIsZero_P\n";
  for (auto& e : idents) {
    const size_t n = e.second.size();
    std::string c5 = "NA", c6 = "NA", c7 = "NA", c10 = "NA", c12 = "NA", c13 = "NA";
    if (haveRef) {
      size_t low = 0; for (double v : e.second) low += v <= cut;
      const double expLow = cutP * n, expRest = n - expLow;
      if (expLow > 0 && expRest > 0) {
        const double dl = (double)low - expLow, dr = (double)(n - low) - expRest;
        const double stat = dl * dl / expLow + dr * dr / expRest;
        c5 = std::to_string((double)low / (double)n);
        c6 = std::to_string(cutP);
        c7 = std::to_string(1 - std::erf(std::sqrt(stat / 2)));   // 1 - cdf(chi_squared(1), stat)
      } else std::cerr << "evidenceUnknownSpecies: expected count of zero for taxon " << e.first << " (the reference asserts here); identity columns NA\n";
    }
    const PerTaxon& g = G.at(e.first);
    if (g.usable > 0) {
      const double avg = (double)g.usableReads / (double)g.usable;
      c10 = std::to_string(avg);
      if (avg == 0) { c12 = std::to_string(g.usable); c13 = std::to_string(1); }
      else {
        const double p0 = std::exp(-avg);                        // Poisson(avg) mass at zero
        c12 = std::to_string(g.usable * p0);
        c13 = std::to_string(g.usableZero > 0 ? 1 - binomial_cdf((double)g.usable, p0, (double)(g.usableZero - 1)) : 1.0);
      }
    }
    auto up = T.upward_by_ranks(e.first, {"species", "genus"});
    o << e.first << "\t" << up.at("species") << "\t" << up.at("genus") << "\t" << n << "\t" << c5 << "\t" << c6 << "\t" << c7 << "\t" << g.windows << "\t"
      << g.usable << "\t" << c10 << "\t" << g.usableZero << "\t" << c12 << "\t" << c13 << "\n";
  }
  return true;
}

// --lca: the part of the taxonomy above the taxa of the mappings as mm_em_lca takes it — node 0 is taxon "1", parents before children (the nodes
// sorted by depth, then ID) — and what the devices return: per read with a mapping its node and mass, per node the reads assigned to it
struct LcaJob {
  double tau = 0;
  std::vector<std::string> id; std::vector<int32_t> parent, depth, taxon_node;
  std::vector<int32_t> node; std::vector<double> mass; std::vector<int64_t> direct; std::mutex m;
  LcaJob(const Taxonomy& T, const std::vector<std::string>& taxa, double tau_, size_t n_reads) : tau(tau_), node(n_reads, -1), mass(n_reads, 0.0) {
    std::map<std::string, int32_t> dep{{"1", 0}};
    std::function<int32_t(const std::string&)> depth_of = [&](const std::string& t) {
      auto it = dep.find(t); if (it != dep.end()) return it->second;
      auto n = T.T.find(t); if (n == T.T.end()) die("--lca: taxon ID " + t + " is not in the taxonomy");
      if (n->second.parent == t) die("--lca: taxon ID " + t + " is its own parent in the taxonomy");
      const int32_t d = depth_of(n->second.parent) + 1;
      return dep[t] = d;
    };
    for (auto& t : taxa) depth_of(t);
    std::vector<std::pair<int32_t, std::string>> order;
    for (auto& kv : dep) order.emplace_back(kv.second, kv.first);
    std::sort(order.begin(), order.end());
    std::map<std::string, int32_t> index;
    for (auto& e : order) { index[e.second] = (int32_t)id.size(); id.push_back(e.second); depth.push_back(e.first); }
    parent.assign(id.size(), 0);
    for (size_t v = 1; v < id.size(); ++v) parent[v] = index.at(T.T.at(id[v]).parent);
    for (auto& t : taxa) taxon_node.push_back(index.at(t));
    direct.assign(id.size(), 0);
  }
};

// PREFIX.EM.kreport: Kraken's six-column report of the LCA assignments — percentage of all reads in the clade, clade reads, reads assigned to the node
// itself, rank code, taxon ID, name indented by two blanks per depth.  First the unclassified reads (unmapped or too short) if there are any, then the
// tree from taxon 1 depth first: clades without reads are left out, children by clade reads descending, then by taxon ID as text.
void write_kreport(const std::string& fn, const Taxonomy& T, const LcaJob& J, size_t nTotal, size_t nUnclassified) {
  static const std::map<std::string, const char*> code{{"superkingdom", "D"}, {"kingdom", "K"}, {"phylum", "P"}, {"class", "C"}, {"order", "O"}, {"family", "F"},
                                                       {"genus", "G"}, {"species", "S"}};
  const size_t N = J.id.size();
  std::vector<int64_t> clade(J.direct);
  std::vector<std::vector<int32_t>> kids(N);
  for (size_t v = N - 1; v > 0; --v) { clade[(size_t)J.parent[v]] += clade[v]; kids[(size_t)J.parent[v]].push_back((int32_t)v); }
  std::ofstream o(fn);
  char num[96];
  auto line = [&](int64_t c, int64_t d, const char* rank, const std::string& id, int depth, const std::string& name) {
    snprintf(num, sizeof num, "%6.2f\t%lld\t%lld\t%s\t", 100.0 * (double)c / (double)nTotal, (long long)c, (long long)d, rank);
    o << num << id << "\t" << std::string(2 * (size_t)depth, ' ') << name << "\n";
  };
  if (nUnclassified) line((int64_t)nUnclassified, (int64_t)nUnclassified, "U", "0", 0, "unclassified");
  std::function<void(int32_t)> walk = [&](int32_t v) {
    if (clade[(size_t)v] == 0) return;
    const TaxNode& n = T.T.at(J.id[(size_t)v]);
    auto c = code.find(n.rank);
    line(clade[(size_t)v], J.direct[(size_t)v], v == 0 ? "R" : c != code.end() ? c->second : "-", J.id[(size_t)v], J.depth[(size_t)v], n.sci);
    std::vector<int32_t>& k = kids[(size_t)v];
    std::sort(k.begin(), k.end(), [&](int32_t a, int32_t b) { return clade[(size_t)a] != clade[(size_t)b] ? clade[(size_t)a] > clade[(size_t)b] : J.id[(size_t)a] < J.id[(size_t)b]; });
    for (int32_t w : k) walk(w);
  };
  walk(0);
}

}  // namespace
