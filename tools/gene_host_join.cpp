// The join of mm_gene_overlap on ONE host thread through mm_gene_core.hpp, for tools/gene_kernel_stats.py: the comparison figure beside the device's
// stage times.  Reads the raw little-endian arrays that the script left in DIR, prints its wall time and checksums of its results.
//   g++ -O2 -std=c++17 -o gene_host_join tools/gene_host_join.cpp && gene_host_join DIR
#include "../metamaps_amd/csrc/mm_gene_core.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

template <class T> static std::vector<T> load(const std::string& fn) {
  FILE* f = fopen(fn.c_str(), "rb"); if (!f) { fprintf(stderr, "cannot open %s\n", fn.c_str()); exit(2); }
  fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)n / sizeof(T));
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string d = std::string(argv[1]) + "/";
  const auto off = load<int64_t>(d + "off"), foff = load<int64_t>(d + "foff");
  const auto gs = load<int32_t>(d + "gs"), ge = load<int32_t>(d + "ge"), gg = load<int32_t>(d + "gg"), feat = load<int32_t>(d + "feat");
  const auto mc = load<int32_t>(d + "mc"), ms = load<int32_t>(d + "ms"), me = load<int32_t>(d + "me");
  const auto mi = load<double>(d + "mi");
  const size_t n_groups = foff.size() - 1;
  size_t n_feats = 0; for (int32_t f : feat) n_feats = std::max(n_feats, (size_t)f + 1);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> pmax(gs.size());
  mm::gene_prefix_max((int64_t)off.size() - 1, off.data(), ge.data(), pmax.data());
  const mm::GeneTable T{off.data(), gs.data(), ge.data(), pmax.data()};
  std::vector<int64_t> reads(n_groups, 0), feats(n_feats, 0), hits(gs.size() + 1);
  std::vector<std::pair<int32_t, double>> pooled;                 // (group, identity) of every overlap
  std::vector<int32_t> mine;
  for (size_t m = 0; m < mc.size(); ++m) {
    int64_t lo, hi; mm::gene_span(T, mc[m], ms[m], me[m], &lo, &hi);
    mm::GeneEmit em{hits.data()};
    mm::gene_stab(mm::GeneSerial{}, T, lo, hi, ms[m], em);
    mine.clear();
    for (int64_t k = 0; k < em.at; ++k) {
      const int32_t g = gg[(size_t)hits[(size_t)k]];
      reads[(size_t)g]++; pooled.emplace_back(g, mi[m]);
      mine.insert(mine.end(), feat.begin() + foff[(size_t)g], feat.begin() + foff[(size_t)g + 1]);
    }
    std::sort(mine.begin(), mine.end());
    mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
    for (int32_t f : mine) feats[(size_t)f]++;
  }
  std::sort(pooled.begin(), pooled.end());
  double median_sum = 0; size_t at = 0;
  for (size_t g = 0; g < n_groups; ++g) { if (reads[g]) median_sum += pooled[at + (size_t)(reads[g] - 1) / 2].second; at += (size_t)reads[g]; }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  long long fsum = 0; for (int64_t x : feats) fsum += x;
  printf("host join, one thread: %.1f ms; %zu pairs, feature reads sum %lld, sum of medians %.6f\n", 1e3 * secs, pooled.size(), fsum, median_sum);
  return 0;
}
