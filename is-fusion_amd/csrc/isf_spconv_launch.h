// isf_spconv_launch.h -- the host side the launchers of the f16x3 sparse-conv family share (isf_spconv16.hip,
// isf_spconv_dma.hip, isf_spconv_deep.hip, isf_spconv_stage.hip): the problem checks, the slots of a kernel instantiation
// and the plan of one launch.
#pragma once
#include "isf_spconv16.h"

#include <atomic>

namespace isf {

// what the tile-family kernels ask of their problem, in the order the exported entries' codes depend on
static inline int conv_check_problem(const char* who, int c_in, int c_out, bool channels_built, int K, int nbr_stride, int n_out) {
  ISF_REQUIRE(K >= 1 && K <= kMaxTaps, ISF_ERR_UNSUPPORTED, "%s: %d taps (max 27)", who, K);
  ISF_REQUIRE(channels_built, ISF_ERR_UNSUPPORTED, "%s: (Cin,Cout)=(%d,%d) not built", who, c_in, c_out);
  ISF_REQUIRE(nbr_stride % 128 == 0 && nbr_stride >= n_out, ISF_ERR_ARG, "%s: bad nbr_stride", who);
  return ISF_OK;
}

// what a launch's `order` holds
enum { kOrderPerm = 0, kOrderTable = 1, kOrderParts = 2 };
static inline int order_mode_bit(int kind) { return kind == kOrderTable ? kConvModeTileTable : (kind == kOrderParts ? kConvModePartTable : 0); }
static inline int conv_order_kind(const ConvCall& c) {
  if (!c.order) return kOrderPerm;
  return (c.mode & kConvModeTileTable) ? kOrderTable : (c.mode & kConvModePartTable) ? kOrderParts : kOrderPerm;
}

// The slots of ONE kernel instantiation on this device family: resident workgroups per CU and CUs per XCD.  Every
// launcher keeps one as a function-local static; the first launch (or launch-info query) fills it.
struct ConvSlots {
  std::atomic<int> wgs_per_cu{0}, cus_per_xcd{0};
};
// lds_bytes: the dynamic LDS of the launch the occupancy is asked for; lds_limit: what the kernel is allowed from now on
static inline int conv_kernel_slots(ConvSlots& s, const void* kern, int threads, size_t lds_bytes, size_t lds_limit) {
  if (s.wgs_per_cu.load(std::memory_order_acquire) != 0) return ISF_OK;
  if (lds_limit > 48 * 1024)
    ISF_HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
  int dev = 0, cus = 0, occ = 0;
  ISF_HIP_TRY(hipGetDevice(&dev));
  ISF_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  ISF_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, lds_bytes));
  s.cus_per_xcd.store(cus >= 8 ? cus / 8 : 1, std::memory_order_relaxed);
  s.wgs_per_cu.store(occ > 0 ? occ : 1, std::memory_order_release);
  return ISF_OK;
}

// How the launch `c` is cut on a kernel with TM-row tiles, ncb column blocks and these slots.  *info (when asked for): the
// plan of its rows -- what conv16_launch_info reports and the order / table builders work on; the return value: what the
// kernel is handed, which for a launch on a tile table or a part table is the table's slots instead.  can_balance: the
// kernel has half tiles.
static inline Conv16Plan conv16_launch_plan(const ConvCall& c, int TM, int ncb, const ConvSlots& s, bool can_balance,
                                            Conv16LaunchInfo* info) {
  const int wgs_per_cu = s.wgs_per_cu.load(std::memory_order_relaxed), cus_per_xcd = s.cus_per_xcd.load(std::memory_order_relaxed);
  const int kind = conv_order_kind(c);
  Conv16Plan plan = conv16_plan(c.n_out, TM, ncb, wgs_per_cu, cus_per_xcd,
                                can_balance && (c.mode & ISF_CONV_MODE_UNIFORM_TILES) == 0 && kind != kOrderParts);
  if (info) *info = Conv16LaunchInfo{plan.full, plan.half, plan.part_rows, TM, ncb, wgs_per_cu, cus_per_xcd};
  if (kind == kOrderParts) {   // equal-work parts of the uniform plan (no half tiles: not balanced): conv16_parts_cap slots per part
    const int parts = ncb == 2 ? 4 : 8;
    plan = Conv16Plan{conv16_parts_cap(conv16_parts_tiles(plan.full, parts), parts), kPlanParts, plan.part_rows};
  }
  if (kind == kOrderTable) plan = Conv16Plan{wgs_per_cu * cus_per_xcd, -1, plan.part_rows};
  return plan;
}

}  // namespace isf
