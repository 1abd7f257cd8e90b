// Host driver of metamaps_amd/csrc/mm_cons_core.hpp (tests/test_cons_core.py), the one-lane form of what the kernels of mm_cons.hip run, in their order:
// candidates, the deletions with their footprints, the SNVs and insertions, the positions' lengths and offsets, the text.
//   stdin    any number of worlds, each "W min_depth min_frac min_called width n_contigs n n_iv", then n_contigs lines "=CONTIG", n lines "w0 w1 count" and
//            n_iv lines "contig first last".
//   stdout   per world "R" where it is refused (thresholds out of range, keys not ascending and unique, a key that is no allele, an interval outside its
//            contig); else per contig with an interval "C contig <the STATS counters> bytes\n" followed by the `bytes` bytes of its text (0 where it is not
//            written), then "E".  A contig's text is written into a buffer of exactly text_bytes(consensusLength): a byte too many is the sanitizer's to see.
#include "../metamaps_amd/csrc/mm_cons_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

struct Cand { uint64_t w0, w1; };

static bool world() {
  std::string tag;
  long long D, width, n_contigs, n, n_iv; double F, C;
  if (!(std::cin >> tag >> D >> F >> C >> width >> n_contigs >> n >> n_iv) || tag != "W") return false;
  std::vector<std::string> contigs((size_t)n_contigs);
  for (auto& c : contigs) { std::cin >> c; c.erase(0, 1); }
  std::vector<uint64_t> w0((size_t)n), w1((size_t)n), starts, ends; std::vector<uint32_t> counts((size_t)n);
  for (size_t i = 0; i < (size_t)n; ++i) std::cin >> w0[i] >> w1[i] >> counts[i];
  struct Iv { long long c, a, b; };
  std::vector<Iv> iv((size_t)n_iv);
  for (auto& x : iv) std::cin >> x.c >> x.a >> x.b;
  if (!std::cin) { fprintf(stderr, "a world is cut short\n"); exit(2); }

  bool ok = mmc::thresholds_ok(D, F, C, width);
  for (size_t i = 0; ok && i < (size_t)n; ++i) {
    ok = i == 0 || w0[i - 1] < w0[i] || (w0[i - 1] == w0[i] && w1[i - 1] < w1[i]);
    const int64_t c = mmp::key_contig(w0[i]);
    ok = ok && c < n_contigs && mmv::key_valid(w0[i], w1[i], (int64_t)contigs[(size_t)c].size());
  }
  for (const auto& x : iv) ok = ok && x.c >= 0 && x.c < n_contigs && x.a >= 0 && x.a <= x.b && x.b < (long long)contigs[(size_t)x.c].size();
  if (!ok) { printf("R\n"); return true; }

  std::vector<int64_t> gbase((size_t)n_contigs + 1, 0);
  for (size_t c = 0; c < (size_t)n_contigs; ++c) gbase[c + 1] = gbase[c] + (int64_t)contigs[c].size();
  const int64_t G = gbase.back();
  for (const auto& x : iv) { starts.push_back(mmp::interval_key(x.c, x.a)); ends.push_back(mmp::interval_key(x.c, x.b)); }
  std::sort(starts.begin(), starts.end()); std::sort(ends.begin(), ends.end());
  std::vector<int64_t> stats((size_t)n_contigs * mmc::STATS, 0);
  auto stat = [&](int64_t c, int k) -> int64_t& { return stats[(size_t)c * mmc::STATS + (size_t)k]; };
  for (const auto& x : iv) ++stat(x.c, mmc::ALIGNMENTS);

  mmp::HostLanes lanes;
  std::vector<Cand> cand;
  for (size_t i = 0; i < (size_t)n; ++i)
    if (mmc::candidate(counts[i], mmp::depth_at(starts.data(), ends.data(), n_iv, mmp::key_contig(w0[i]), mmp::key_pos(w0[i])), D, F)) cand.push_back(Cand{w0[i], w1[i]});
  std::vector<uint8_t> state((size_t)G, 0); std::vector<uint32_t> ins((size_t)G, 0);
  uint64_t ends_before = 0;                                        // the exclusive prefix maximum of the deletions' end keys
  for (const Cand& k : cand) {
    const int64_t c = mmp::key_contig(k.w0);
    if (mmc::is_del(k.w0)) {
      const bool applied = mmc::del_applied(k.w0, ends_before);
      mmc::clear_footprint(lanes, state.data(), gbase[(size_t)c] + mmp::key_pos(k.w0) + 1, (int64_t)k.w1, applied);
      if (applied) { ++stat(c, mmc::DELETIONS); stat(c, mmc::DELETED_BASES) += (int64_t)k.w1; } else ++stat(c, mmc::DROPPED);
    }
    ends_before = std::max(ends_before, mmc::del_end_key(k.w0, k.w1));
  }
  for (size_t i = 0; i < cand.size(); ++i) {
    const Cand& k = cand[i];
    if (mmc::is_del(k.w0)) continue;
    const int64_t c = mmp::key_contig(k.w0), g = gbase[(size_t)c] + mmp::key_pos(k.w0);
    if (!mmc::point_applied(k.w0, i > 0, i > 0 ? cand[i - 1].w0 : 0, state[(size_t)g])) { ++stat(c, mmc::DROPPED); continue; }
    if (mmc::is_snv(k.w0)) { state[(size_t)g] = mmc::snv_state(k.w0); ++stat(c, mmc::SNVS); }
    else { ins[(size_t)g] = (uint32_t)i + 1; ++stat(c, mmc::INSERTIONS); stat(c, mmc::INSERTED_BASES) += mmv::ins_len(k.w1); }
  }

  for (int64_t c = 0; c < n_contigs; ++c) {
    if (!stat(c, mmc::ALIGNMENTS)) continue;
    const int64_t len = (int64_t)contigs[(size_t)c].size();
    std::vector<int64_t> depth((size_t)len), off((size_t)len + 1, 0);
    for (int64_t p = 0; p < len; ++p) { depth[(size_t)p] = mmp::depth_at(starts.data(), ends.data(), n_iv, c, p); stat(c, mmc::CALLED) += depth[(size_t)p] >= D; }
    const bool written = stat(c, mmc::CALLED) >= mmc::called_needed(C, len);
    for (int64_t p = 0; p < len; ++p) {
      const size_t g = (size_t)(gbase[(size_t)c] + p);
      off[(size_t)p + 1] = off[(size_t)p] + mmc::out_len(state[g], ins[g] ? mmv::ins_len(cand[ins[g] - 1].w1) : 0, written);
    }
    const int64_t L = off[(size_t)len], bytes = mmc::text_bytes(L, width);
    stat(c, mmc::WRITTEN) = written; stat(c, mmc::LENGTH) = L;
    if (written && L != len - stat(c, mmc::DELETED_BASES) + stat(c, mmc::INSERTED_BASES)) { fprintf(stderr, "the offsets disagree with the counters\n"); exit(3); }
    uint8_t* const text = (uint8_t*)malloc((size_t)bytes + (bytes == 0));
    for (int64_t i = 0; i < bytes; ++i) text[i] = '?';
    for (int64_t p = 0; p < len; ++p) {
      const size_t g = (size_t)(gbase[(size_t)c] + p);
      const bool live = off[(size_t)p + 1] > off[(size_t)p];
      mmc::emit_position(lanes, text, L, width, off[(size_t)p], live, mmc::out_base(state[g], depth[(size_t)p], D, (uint8_t)contigs[(size_t)c][(size_t)p]),
                         live && ins[g] ? cand[ins[g] - 1].w1 : 0);
    }
    printf("C %lld", (long long)c);
    for (int k = 0; k < mmc::STATS; ++k) printf(" %lld", (long long)stat(c, k));
    printf(" %lld\n", (long long)bytes);
    fwrite(text, 1, (size_t)bytes, stdout);
    free(text);
  }
  printf("E\n");
  return true;
}

int main() {
  while (world()) {}
  return 0;
}
