// Host build of metamaps_amd/csrc/mm_hpc_core.hpp for tests/test_hpc_core.py: the sequences on stdin (one per line, A/C/G/T, an empty line is an
// empty sequence) are packed as mm_seqset packs them (16 bases per word, every sequence on a word boundary), compressed with the header's
// word-level functions, and printed: per sequence the compressed text, then "raw:rawlast" of the compressed positions 0 .. clen + 2.
#include "../metamaps_amd/csrc/mm_hpc_core.hpp"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

int main() {
  std::vector<std::string> seqs;
  std::string line;
  while (std::getline(std::cin, line)) seqs.push_back(line);
  const size_t n = seqs.size();
  std::vector<uint64_t> base(n + 1, 0);
  std::vector<int32_t> rawlen(n), clen(n);
  for (size_t i = 0; i < n; ++i) { rawlen[i] = (int32_t)seqs[i].size(); base[i + 1] = base[i] + ((seqs[i].size() + 15) & ~(size_t)15); }
  const size_t nwords = base[n] >> 4, nb = (base[n] + 63) >> 6;
  std::vector<uint32_t> packed(nwords + 1, 0);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < seqs[i].size(); ++j) {
      const char c = seqs[i][j];
      const uint32_t code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3;
      packed[(base[i] + j) >> 4] |= code << (2 * ((base[i] + j) & 15));
    }
  // run-start bitmap: keep masks of the words, first base of a sequence forced, pad positions cleared
  std::vector<uint64_t> bitmap(nb + 1, 0), rank(nb + 1, 0);
  for (size_t t = 0; t < nwords; ++t) bitmap[t >> 2] |= (uint64_t)mm::hpc_keep_mask(packed[t], t ? packed[t - 1] >> 30 : 0u) << (16 * (t & 3));
  for (size_t i = 0; i < n; ++i) {
    for (uint64_t g = base[i] + seqs[i].size(); g < base[i + 1]; ++g) bitmap[g >> 6] &= ~(1ull << (g & 63));
    if (!seqs[i].empty()) bitmap[base[i] >> 6] |= 1ull << (base[i] & 63);
  }
  for (size_t b = 0; b < nb; ++b) rank[b + 1] = rank[b] + (uint64_t)mm::hpc_popc64(bitmap[b]);
  // extraction, sequence by sequence: the kept fields of every word are appended to the output words
  std::vector<std::vector<uint32_t>> out(n);
  std::vector<uint64_t> samp_off(n + 1, 0);
  std::vector<uint32_t> samp;
  for (size_t i = 0; i < n; ++i) {
    clen[i] = (int32_t)(mm::hpc_rank(bitmap.data(), rank.data(), base[i + 1]) - mm::hpc_rank(bitmap.data(), rank.data(), base[i]));
    out[i].assign(((size_t)clen[i] + 15) / 16 + 1, 0);
    uint64_t acc = 0; int fill = 0; size_t ow = 0;
    for (uint64_t t = base[i] >> 4; t < base[i + 1] >> 4; ++t) {
      int c = 0;
      const uint32_t f = mm::hpc_extract(packed[t], (uint32_t)(bitmap[t >> 2] >> (16 * (t & 3))) & 0xffffu, &c);
      acc |= (uint64_t)f << (2 * fill); fill += c;
      if (fill >= 16) { out[i][ow++] = (uint32_t)acc; acc >>= 32; fill -= 16; }
    }
    if (fill) out[i][ow++] = (uint32_t)acc;
    for (int64_t p = 0; p < clen[i]; p += 1 << mm::HPC_SAMPLE_SHIFT) {   // kept base p of the sequence: the set bit of rank rank(base) + p
      const uint64_t r = mm::hpc_rank(bitmap.data(), rank.data(), base[i]) + (uint64_t)p;
      size_t b = base[i] >> 6;
      while (rank[b + 1] <= r) ++b;
      samp.push_back((uint32_t)((b << 6) + (uint64_t)mm::hpc_select64(bitmap[b], (int)(r - rank[b])) - base[i]));
    }
    samp_off[i + 1] = samp.size();
  }
  samp.push_back(0);
  const mm::HpcMapView M{bitmap.data(), base.data(), rawlen.data(), clen.data(), samp_off.data(), samp.data(), (int64_t)n};
  for (size_t i = 0; i < n; ++i) {
    std::string s;
    for (int64_t p = 0; p < clen[i]; ++p) s += "ACGT"[(out[i][(size_t)p >> 4] >> (2 * (p & 15))) & 3u];
    printf("%s\n", s.c_str());
    for (int64_t p = 0; p <= (int64_t)clen[i] + 2; ++p) printf("%lld:%lld ", (long long)mm::hpc_raw_first(M, (int64_t)i, p), (long long)mm::hpc_raw_last(M, (int64_t)i, p));
    printf("\n");
  }
  return 0;
}
