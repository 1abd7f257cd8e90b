// Host driver of metamaps_amd/csrc/mm_depth_core.hpp (tests/test_depth_core.py), the one-thread form of what the kernels of mm_depth.hip run, in their order:
// the sorted interval keys, the unique breakpoints and their depths, the runs, the prefix sums in start order and in (contig, depth) order, the contigs'
// counters, the windows.  Every array has exactly the entries the definition names: a read beyond one is the sanitizer's to see.
//   stdin    any number of worlds, each "W window n_contigs n_iv n_thresholds", then the lengths, the thresholds and n_iv lines "contig first last".
//   stdout   per world "R <why>" where it is refused; else "r contig start end depth" per run, "c contig win_off <the counters>" per listed contig,
//            "w sum covered" per window, then "E n_windows".
#include "../metamaps_amd/csrc/mm_depth_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

static bool world() {
  std::string tag;
  long long window, n_contigs, n_iv, n_t;
  if (!(std::cin >> tag >> window >> n_contigs >> n_iv >> n_t) || tag != "W") return false;
  std::vector<int64_t> len((size_t)n_contigs), thr((size_t)n_t);
  for (auto& x : len) { long long v; std::cin >> v; x = v; }
  for (auto& x : thr) { long long v; std::cin >> v; x = v; }
  struct Iv { long long c, a, b; };
  std::vector<Iv> iv((size_t)n_iv);
  for (auto& x : iv) std::cin >> x.c >> x.a >> x.b;
  if (!std::cin) { fprintf(stderr, "a world is cut short\n"); exit(2); }

  for (int64_t c = 0; c < n_contigs; ++c) if (!mmdp::length_ok(len[(size_t)c])) { printf("R length\n"); return true; }
  if (window < 1) { printf("R window\n"); return true; }
  if (!mmdp::thresholds_ok((int32_t)n_t, thr.data())) { printf("R thresholds\n"); return true; }
  for (size_t i = 0; i < iv.size(); ++i)
    if (!mmdp::interval_ok(iv[i].c, iv[i].a, iv[i].b, n_contigs, len.data())) { printf("R interval %zu\n", i); return true; }
  std::vector<int64_t> listed;
  for (const auto& x : iv) listed.push_back(x.c);
  std::sort(listed.begin(), listed.end());
  listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
  std::vector<uint64_t> win_off(listed.size() + 1, 0);
  for (size_t j = 0; j < listed.size(); ++j) win_off[j + 1] = win_off[j] + (uint64_t)mmdp::window_count(len[(size_t)listed[j]], window);
  if (win_off.back() > (uint64_t)mmdp::MAX_WINDOWS) { printf("R windows\n"); return true; }
  mmdp::Thresholds T{(int32_t)n_t, {}};
  for (size_t k = 0; k < thr.size(); ++k) T.t[k] = thr[k];
  if (iv.empty()) { printf("E 0\n"); return true; }

  std::vector<uint64_t> starts, ends, bk;
  for (const auto& x : iv) { starts.push_back(mmp::interval_key(x.c, x.a)); ends.push_back(mmp::interval_key(x.c, x.b)); }
  std::sort(starts.begin(), starts.end()); std::sort(ends.begin(), ends.end());
  for (size_t i = 0; i < iv.size(); ++i) { bk.push_back(starts[i]); bk.push_back(mmdp::end_break(ends[i])); }
  std::sort(bk.begin(), bk.end());
  bk.erase(std::unique(bk.begin(), bk.end()), bk.end());
  const size_t m = bk.size();
  std::vector<uint32_t> pd(m);
  for (size_t j = 0; j < m; ++j) pd[j] = mmdp::piece_depth(starts.data(), ends.data(), n_iv, bk[j]);

  std::vector<uint64_t> rstart, rend; std::vector<uint32_t> rdepth;
  for (size_t j = 0; j < m; ++j) {
    if (mmdp::run_head(j > 0, j > 0 ? bk[j - 1] : 0, j > 0 ? pd[j - 1] : 0, bk[j], pd[j])) { rstart.push_back(bk[j]); rdepth.push_back(pd[j]); }
    if (mmdp::run_tail(pd[j], j + 1 < m, j + 1 < m ? pd[j + 1] : 0)) {
      if (j + 1 >= m || rend.size() + 1 != rstart.size()) { fprintf(stderr, "a run has no end\n"); exit(3); }
      rend.push_back(bk[j + 1]);
    }
  }
  const size_t nr = rstart.size();
  if (rend.size() != nr) { fprintf(stderr, "runs and ends differ in number\n"); exit(3); }
  std::vector<uint64_t> plen(nr + 1, 0), psum(nr + 1, 0), dlen(nr + 1, 0);
  std::vector<std::pair<uint64_t, uint64_t>> by_depth(nr);
  for (size_t r = 0; r < nr; ++r) {
    const uint64_t l = rend[r] - rstart[r];
    plen[r + 1] = plen[r] + l; psum[r + 1] = psum[r] + l * rdepth[r];
    by_depth[r] = {(rstart[r] & ~mmdp::POS_MASK) | rdepth[r], l};
  }
  std::stable_sort(by_depth.begin(), by_depth.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  std::vector<uint64_t> dkey(nr);
  for (size_t r = 0; r < nr; ++r) { dkey[r] = by_depth[r].first; dlen[r + 1] = dlen[r] + by_depth[r].second; }
  const mmdp::Runs R{(int64_t)nr, rstart.data(), rend.data(), rdepth.data(), plen.data(), psum.data()};
  const mmdp::RunsByDepth D{dkey.data(), dlen.data()};

  for (size_t r = 0; r < nr; ++r)
    printf("r %lld %lld %lld %u\n", (long long)mmdp::key_contig(rstart[r]), (long long)mmdp::key_pos(rstart[r]), (long long)mmdp::key_pos(rend[r]), rdepth[r]);
  for (size_t j = 0; j < listed.size(); ++j) {
    std::vector<int64_t> out((size_t)(mmdp::STATS + T.n));
    mmdp::contig_stats(listed[j], len[(size_t)listed[j]], starts.data(), n_iv, R, D, T, out.data());
    printf("c %lld %llu", (long long)listed[j], (unsigned long long)win_off[j]);
    for (int64_t x : out) printf(" %lld", (long long)x);
    printf("\n");
  }
  const int64_t n_windows = (int64_t)win_off.back();
  for (int64_t w = 0; w < n_windows; ++w) {
    const int64_t j = mmdp::window_contig(win_off.data(), (int64_t)listed.size(), w);
    int64_t a, b, s = -1, n = -1;
    mmdp::window_span(len[(size_t)listed[(size_t)j]], window, w - (int64_t)win_off[(size_t)j], &a, &b);
    mmdp::window_sums(listed[(size_t)j], a, b, R, &s, &n);
    printf("w %lld %lld\n", (long long)s, (long long)n);
  }
  printf("E %lld\n", (long long)n_windows);
  return true;
}

int main() {
  while (world()) {}
  return 0;
}
