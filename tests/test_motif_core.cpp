// The host instantiation of metamaps_amd/csrc/mm_motif_core.hpp for tests/test_motif_core.py (plain g++, no HIP).
//   t tile            prints mmt::SCAN_TILE and mmt::HALO
//   t profile < text  one world: "n_contigs n_entries code_base n_motifs min_coverage min_frac combine", a line per contig (its bytes), a line "LETTERS pos" per
//                     motif, a line "key count" per entry of the merged table.  Prints "R site motif code n_mod n_canonical n_other n_fail" per row in the
//                     order of the segments and "S contig motif code sites covered modified n_valid_cov n_mod" per (listed contig, motif, applicable code);
//                     "E motif j" for an item that make_motif (or, under combine, own_reverse_complement) refuses.
#include "../metamaps_amd/csrc/mm_motif_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

struct Bytes { const std::string* s; uint8_t byte(int64_t i) const { return (uint8_t)(*s)[(size_t)i]; } };

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "tile")) { printf("%d %d\n", mmt::SCAN_TILE, mmt::HALO); return 0; }
  if (argc != 2 || strcmp(argv[1], "profile")) return 2;
  size_t nc, ne; std::string code_base, frac; int nm, combine; long long min_cov;
  std::cin >> nc >> ne >> code_base >> nm >> min_cov >> frac >> combine;
  const double min_frac = strtod(frac.c_str(), nullptr);
  std::vector<std::string> contigs(nc);
  for (auto& c : contigs) std::cin >> c;
  mmt::Motifs M{};
  M.n = nm;
  for (int j = 0; j < nm; ++j) {
    std::string letters; int pos;
    std::cin >> letters >> pos;
    std::vector<uint8_t> mask;
    for (char x : letters) mask.push_back((uint8_t)mmt::letter_mask((uint8_t)x));
    if (!mmt::make_motif(mask.data(), (int32_t)mask.size(), pos, &M.m[j]) || (combine && !mmt::own_reverse_complement(M.m[j]))) { printf("E motif %d\n", j); return 0; }
  }
  std::vector<uint64_t> keys(ne); std::vector<uint32_t> counts(ne);
  for (size_t i = 0; i < ne; ++i) std::cin >> keys[i] >> counts[i];
  if (!std::cin) return 3;
  mmd::CodeBases cb{};
  cb.n = (int)code_base.size();
  for (int k = 0; k < cb.n; ++k) cb.b[k] = (uint8_t)code_base[(size_t)k];
  const int64_t n = (int64_t)ne;
  std::vector<int64_t> sums(nc * mmt::MAX_MOTIFS * mmd::MAX_CODES * 4, 0);
  std::vector<char> listed(nc, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (i && mmd::key_site(keys[i]) == mmd::key_site(keys[i - 1])) continue;
    const size_t c = (size_t)mmd::key_contig(keys[i]);
    listed[c] = 1;
    mmt::Row rows[mmt::MAX_MOTIFS * mmd::MAX_CODES];
    auto add = [&](int32_t motif, int32_t code, bool modified, uint64_t valid, uint64_t mod) {
      int64_t* q = &sums[((c * mmt::MAX_MOTIFS + (size_t)motif) * mmd::MAX_CODES + (size_t)code) * 4];
      q[0] += 1; q[1] += modified; q[2] += (int64_t)valid; q[3] += (int64_t)mod;
    };
    const int k = mmt::site_rows(keys.data(), counts.data(), i, n, Bytes{&contigs[c]}, (int64_t)contigs[c].size(), cb, M, min_cov, min_frac, combine != 0, rows, add);
    for (int r = 0; r < k; ++r)
      printf("R %llu %d %d %llu %llu %llu %llu\n", (unsigned long long)rows[r].site, rows[r].motif, rows[r].code, (unsigned long long)rows[r].n_mod, (unsigned long long)rows[r].n_canonical,
             (unsigned long long)rows[r].n_other, (unsigned long long)rows[r].n_fail);
  }
  for (size_t c = 0; c < nc; ++c) {
    if (!listed[c]) continue;
    const Bytes ref{&contigs[c]};
    const int64_t len = (int64_t)contigs[c].size();
    for (int j = 0; j < nm; ++j) {
      int64_t sites = 0;
      for (int64_t q = 0; q < len; ++q) sites += (int64_t)mmt::occurs(ref, len, q, false, M.m[j]) + (int64_t)(!combine && mmt::occurs(ref, len, q, true, M.m[j]));
      for (int k = 0; k < cb.n; ++k) {
        if (cb.b[k] != M.m[j].base) continue;
        const int64_t* q = &sums[((c * mmt::MAX_MOTIFS + (size_t)j) * mmd::MAX_CODES + (size_t)k) * 4];
        printf("S %zu %d %d %lld %lld %lld %lld %lld\n", c, j, k, (long long)sites, (long long)q[0], (long long)q[1], (long long)q[2], (long long)q[3]);
      }
    }
  }
  return 0;
}
