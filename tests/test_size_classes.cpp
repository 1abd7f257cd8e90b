// CPU harness: metamaps_amd/csrc/mm_size_classes.hpp (which LDS radix sort instance a read of `count` minimizers / seed hits takes)
// against the rule restated as a search: the smallest listed IPT with 256 * IPT >= count, nothing to do for an empty minimizer list and
// for zero or one hit, the segmented sort beyond the last class.  Every count from 0 to <n>.  Prints "ok <n>" or the first fault.
#include "../metamaps_amd/csrc/mm_size_classes.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int ref_class(const std::vector<int>& ipts, unsigned long long count, unsigned long long nothing_up_to) {
  if (count <= nothing_up_to) return mm::SIZE_CLASS_NONE;
  for (int ipt : ipts) if (256ull * (unsigned long long)ipt >= count) return ipt;      // (ascending: the first that holds it is the smallest)
  return mm::SIZE_CLASS_SEGMENTED;
}

int main(int argc, char** argv) {
  const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  const std::vector<int> k2 = {4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64}, k4 = {1, 2, 3, 4, 6, 8, 12, 16};   // the lists of the issue, not the header's
  if (mm::N_SKETCH_CLASSES != (int)k2.size() || mm::N_HIT_SORT_CLASSES != (int)k4.size()) FAIL("class counts %d %d", mm::N_SKETCH_CLASSES, mm::N_HIT_SORT_CLASSES);
  for (size_t i = 0; i < k2.size(); ++i) if (mm::SKETCH_IPTS[i] != k2[i]) FAIL("SKETCH_IPTS[%zu] = %d", i, mm::SKETCH_IPTS[i]);
  for (size_t i = 0; i < k4.size(); ++i) if (mm::HIT_SORT_IPTS[i] != k4[i]) FAIL("HIT_SORT_IPTS[%zu] = %d", i, mm::HIT_SORT_IPTS[i]);
  if (mm::SKETCH_LDS_MAX != 16384 || mm::HIT_SORT_LDS_MAX != 4096) FAIL("LDS sort limits %llu %llu", (unsigned long long)mm::SKETCH_LDS_MAX, (unsigned long long)mm::HIT_SORT_LDS_MAX);
  std::vector<unsigned long long> counts;
  for (unsigned long long c = 0; c <= n; ++c) counts.push_back(c);
  for (int lg = 15; lg < 64; ++lg) for (int d = -1; d <= 1; ++d) counts.push_back((1ull << lg) + d);   // far beyond: no wrap of (count + 255) / 256
  counts.push_back(~0ull); counts.push_back(~0ull - 255); counts.push_back(~0ull - 256);
  int seen2[65] = {0}, seen4[17] = {0}, seg2 = 0, seg4 = 0;
  for (unsigned long long c : counts) {
    const int a = mm::sketch_class(c), b = mm::hit_sort_class(c), ia = mm::sketch_class_index(c), ib = mm::hit_sort_class_index(c);
    if (a != ref_class(k2, c, 0)) FAIL("sketch_class(%llu) = %d, rule %d", c, a, ref_class(k2, c, 0));
    if (b != ref_class(k4, c, 1)) FAIL("hit_sort_class(%llu) = %d, rule %d", c, b, ref_class(k4, c, 1));
    // the index form that bins the reads names the same kernel, and leaves out exactly the reads without one
    if (ia < 0 || ia > mm::N_SKETCH_CLASSES || (ia < mm::N_SKETCH_CLASSES ? mm::SKETCH_IPTS[ia] != a : a > 0)) FAIL("sketch_class_index(%llu) = %d beside class %d", c, ia, a);
    if (ib < 0 || ib > mm::N_HIT_SORT_CLASSES || (ib < mm::N_HIT_SORT_CLASSES ? mm::HIT_SORT_IPTS[ib] != b : b > 0)) FAIL("hit_sort_class_index(%llu) = %d beside class %d", c, ib, b);
    if (a > 0) { if (256ull * a < c) FAIL("sketch_class(%llu) = %d does not hold the read", c, a); seen2[a] = 1; } else seg2 += a == mm::SIZE_CLASS_SEGMENTED;
    if (b > 0) { if (256ull * b < c) FAIL("hit_sort_class(%llu) = %d does not hold the read", c, b); seen4[b] = 1; } else seg4 += b == mm::SIZE_CLASS_SEGMENTED;
  }
  if (n >= 16385) {
    for (int ipt : k2) if (!seen2[ipt]) FAIL("no count took sketch class %d", ipt);
    for (int ipt : k4) if (!seen4[ipt]) FAIL("no count took hit sort class %d", ipt);
    if (!seg2 || !seg4) FAIL("no count took the segmented path");
  }
  static_assert(mm::sketch_class(0) == mm::SIZE_CLASS_NONE && mm::sketch_class(1) == 4 && mm::sketch_class(1024) == 4 && mm::sketch_class(1025) == 6, "K2 edges");
  static_assert(mm::sketch_class(16384) == 64 && mm::sketch_class(16385) == mm::SIZE_CLASS_SEGMENTED, "K2 last class");
  static_assert(mm::hit_sort_class(1) == mm::SIZE_CLASS_NONE && mm::hit_sort_class(2) == 1 && mm::hit_sort_class(256) == 1 && mm::hit_sort_class(257) == 2, "K4 edges");
  static_assert(mm::hit_sort_class(4096) == 16 && mm::hit_sort_class(4097) == mm::SIZE_CLASS_SEGMENTED, "K4 last class");
  printf("ok %zu counts\n", counts.size());
  return 0;
}
