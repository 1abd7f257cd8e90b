// Size classes of the per-read LDS radix sorts (K2: a read's minimizers, K4: its seed hits): which kernel instance a read of `count`
// elements takes.  A workgroup of 256 threads sorts 256 * IPT elements; a read takes the smallest listed IPT with 256 * IPT >= count,
// nothing where there is nothing to sort, and the device's segmented sort beyond the last class.  Arithmetic only, no device types:
// mm_map.hip bins the reads of a batch with it, tests/test_size_classes.cpp holds it against the rule restated.
#pragma once
#include <cstdint>

namespace mm {

constexpr int SIZE_CLASS_NONE = 0;                                // nothing to do for this read
constexpr int SIZE_CLASS_SEGMENTED = -1;                          // beyond the LDS sort: the segmented device sort

constexpr int SKETCH_IPTS[] = {4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64};
constexpr int HIT_SORT_IPTS[] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int N_SKETCH_CLASSES = (int)(sizeof(SKETCH_IPTS) / sizeof(int));
constexpr int N_HIT_SORT_CLASSES = (int)(sizeof(HIT_SORT_IPTS) / sizeof(int));
constexpr uint64_t SKETCH_LDS_MAX = 256 * (uint64_t)SKETCH_IPTS[N_SKETCH_CLASSES - 1];        // 16 384 minimizers
constexpr uint64_t HIT_SORT_LDS_MAX = 256 * (uint64_t)HIT_SORT_IPTS[N_HIT_SORT_CLASSES - 1];  //  4 096 seed hits

// elements per thread needed -> index into the IPT list, as a table built at compile time: one look-up per read in the host loops that
// bin a batch (mm_map.hip, bin_reads).  [MAX_IPT + 1]: beyond the LDS sort.
template <int N, int MAX_IPT>
struct IptClassTable {
  uint8_t of_need[MAX_IPT + 2];
  constexpr explicit IptClassTable(const int (&ipts)[N]) : of_need{} {
    for (int need = 0, i = 0; need <= MAX_IPT; ++need) { while (ipts[i] < need) ++i; of_need[need] = (uint8_t)i; }
    of_need[MAX_IPT + 1] = (uint8_t)N;
  }
  constexpr int index(uint64_t count) const {
    const uint64_t need = count / 256 + (count % 256 != 0);       // ceil(count / 256) that does not wrap at the top of 64 bits
    return of_need[need < (uint64_t)MAX_IPT + 1 ? need : (uint64_t)MAX_IPT + 1];
  }
};
constexpr IptClassTable<N_SKETCH_CLASSES, 64> SKETCH_CLASS_TABLE(SKETCH_IPTS);
constexpr IptClassTable<N_HIT_SORT_CLASSES, 16> HIT_SORT_CLASS_TABLE(HIT_SORT_IPTS);

// index into SKETCH_IPTS of a read of `count` minimizers; N_SKETCH_CLASSES: not for sketch_radix_kernel (no minimizer, or more than 16 384)
constexpr int sketch_class_index(uint64_t count) { return count == 0 ? N_SKETCH_CLASSES : SKETCH_CLASS_TABLE.index(count); }
// index into HIT_SORT_IPTS of a read of `count` seed hits; N_HIT_SORT_CLASSES: not for sort_hits_radix_kernel (zero or one hit: sorted
// already; more than 4 096)
constexpr int hit_sort_class_index(uint64_t count) { return count <= 1 ? N_HIT_SORT_CLASSES : HIT_SORT_CLASS_TABLE.index(count); }

// the same as elements per thread: an IPT of the list, SIZE_CLASS_NONE or SIZE_CLASS_SEGMENTED
constexpr int sketch_class(uint64_t count) {
  const int i = sketch_class_index(count);
  return i < N_SKETCH_CLASSES ? SKETCH_IPTS[i] : count > SKETCH_LDS_MAX ? SIZE_CLASS_SEGMENTED : SIZE_CLASS_NONE;
}
constexpr int hit_sort_class(uint64_t count) {
  const int i = hit_sort_class_index(count);
  return i < N_HIT_SORT_CLASSES ? HIT_SORT_IPTS[i] : count > HIT_SORT_LDS_MAX ? SIZE_CLASS_SEGMENTED : SIZE_CLASS_NONE;
}

// the template argument list of a dispatch<...> is the IPT list it serves
template <int... V>
constexpr bool ipt_list_is(const int (&ipts)[sizeof...(V)]) {
  const int v[] = {V...};
  for (unsigned i = 0; i < sizeof...(V); ++i) if (v[i] != ipts[i]) return false;
  return true;
}

}  // namespace mm
