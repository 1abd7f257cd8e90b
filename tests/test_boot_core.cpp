// CPU unit test of the bootstrap weights (metamaps_amd/csrc/mm_boot_core.hpp): prints boot_weight for (seed, r, i) triples read from
// stdin as lines "seed r i", one weight per line.  Built and run by tests/test_boot_core.py with g++ (no GPU needed).
#include "../metamaps_amd/csrc/mm_boot_core.hpp"
#include <cstdio>
#include <vector>

int main() {
  unsigned long long seed; unsigned r, i;
  std::vector<char> out;
  out.reserve(1 << 22);
  while (scanf("%llu %u %u", &seed, &r, &i) == 3) { out.push_back((char)('a' + mm::boot_weight(seed, r, i))); }
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
