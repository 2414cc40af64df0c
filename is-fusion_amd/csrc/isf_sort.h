// isf_sort.h -- the pass plan of the stable LSD radix sort (isf_sort.hip): pure host code, no HIP call, so that
// tests/test_sort_plan.py can ask it for every key width without a GPU.
#pragma once

namespace isf {

constexpr int kSortMaxPassBits = 10;   // digits per pass <= 1024: the pass kernel's LDS counters
constexpr int kSortMaxPasses = 4;      // 32 key bits

// key_bits (1 .. 32) in ceil(key_bits / 10) passes of equal width, the LAST pass taking the remainder: the widths sum to
// key_bits exactly, so no bit above key_bits ever decides the order.  Pass p starts at bit p * bits[0].
struct SortPlan {
  int passes;
  int bits[kSortMaxPasses];
};
inline SortPlan stable_sort_plan(int key_bits) {
  SortPlan pl = {};
  pl.passes = (key_bits + kSortMaxPassBits - 1) / kSortMaxPassBits;
  const int bits = (key_bits + pl.passes - 1) / pl.passes;
  for (int p = 0; p < pl.passes; ++p) pl.bits[p] = p + 1 < pl.passes ? bits : key_bits - (pl.passes - 1) * bits;
  return pl;
}

}  // namespace isf
