// isf_spconv16.h -- what the f16x3 sparse-conv kernel (isf_spconv16.hip) and its siblings share: the mode bits and the
// instantiation choice of a launch (host), fragment types, LDS-DMA, the split format, the XCD-aware tile mapping, the
// plans and the epilogue.
#pragma once
#include "isf_common.h"

namespace isf {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

static constexpr int kMaxTaps = 27;

// CONV MODE bits that are hand-overs between the library's translation units.  They occupy the same int as the public
// ISF_CONV_MODE_* bits (include/isf_hip.h), which therefore never take these values.
static constexpr int kConvModeNarrowTiles = 64;   // the 128-column layers of the large levels on the 4-wave 128-row tile
                                                  // instead of the 8-wave 256-row one (A/B; the encoder's ISF_ENC_DIAG_NARROW_TILES)
static constexpr int kConvModeTileTable = 1024;   // `order` is a tile table (isf_sparse_conv_tile_table), not a tile order
static constexpr int kConvModePartTable = 16384;  // `order` is a part table (conv16_part_table_impl): equal-work parts of a launch of several rounds
// what conv16_choose ignores when it compares `mode` with one of the launch variants
static constexpr int kConvModeTileBits = ISF_CONV_MODE_UNIFORM_TILES | kConvModeTileTable | kConvModePartTable;

// Modes the exported entry points accept: a BASE mode (one of the values below) | any of the entry point's option bits.
static constexpr bool conv_mode_is_production(int m) {   // valid results on the production workgroup shapes
  return m == 0 || m == ISF_CONV_MODE_F16 || m == ISF_CONV_MODE_NO_SHARING || m == ISF_CONV_MODE_F16_STORAGE;
}
static constexpr bool conv_mode_is_knockout(int m) {     // timing diagnostics: results are garbage
  return m == ISF_CONV_MODE_NO_GATHER || m == ISF_CONV_MODE_NO_WEIGHTS || m == (ISF_CONV_MODE_NO_GATHER | ISF_CONV_MODE_NO_WEIGHTS) ||
         m == ISF_CONV_MODE_NO_LOOP;
}
static constexpr int kConvIssueOpts = ISF_CONV_MODE_STAGGER | ISF_CONV_MODE_R4_ISSUE | ISF_CONV_MODE_TWO_AHEAD | ISF_CONV_MODE_CHUNK_SPLIT;
static constexpr int kConvOptsForward = ISF_CONV_MODE_UNIFORM_TILES | kConvIssueOpts | kConvModeNarrowTiles | ISF_CONV_MODE_ONE_BLOCK_4W |
                                        ISF_CONV_MODE_ONE_BLOCK_8W | ISF_CONV_MODE_DEEP;   // isf_sparse_conv_forward_f16x3 (+ knock-outs)
static constexpr int kConvOptsOrdered = ISF_CONV_MODE_UNIFORM_TILES | kConvIssueOpts;      // isf_sparse_conv_forward_f16x3_ordered
static constexpr int kConvOptsTiled = 0;                                // isf_sparse_conv_tile_table / _forward_f16x3_tiled
static constexpr int kConvOptsDma = ISF_CONV_MODE_UNIFORM_TILES;        // isf_sparse_conv_forward_dma / _lines: base 0 | F16 | F16_STORAGE
static constexpr int kConvOptsStaged = ISF_CONV_MODE_UNIFORM_TILES;     // isf_sparse_conv_forward_staged: base 0 | F16

// The kernels' template parameter MODE is a THIRD number space (after the runtime `mode` and the encoder's `diagnostic`).
// These bits mean what the runtime bit of the same value means: conv_kern_bits hands them over unchanged ...
static constexpr int kKernF16 = ISF_CONV_MODE_F16, kKernNoGather = ISF_CONV_MODE_NO_GATHER, kKernNoWeights = ISF_CONV_MODE_NO_WEIGHTS,
                     kKernNoLoop = ISF_CONV_MODE_NO_LOOP, kKernNoSharing = ISF_CONV_MODE_NO_SHARING, kKernF16Rows = ISF_CONV_MODE_F16_ROWS,
                     kKernStagger = ISF_CONV_MODE_STAGGER, kKernR4Issue = ISF_CONV_MODE_R4_ISSUE, kKernTwoAhead = ISF_CONV_MODE_TWO_AHEAD,
                     kKernChunkSplit = ISF_CONV_MODE_CHUNK_SPLIT;
// ... and these two do NOT: as runtime bits 2048 is ISF_CONV_MODE_DMA_PLAN, and 512 is the encoder's ISF_ENC_DIAG_CU_KERNEL.
// Every other runtime bit (tiles, workgroup shape, kernel choice) is resolved on the host and never reaches a kernel.
static constexpr int kKernTrace = 512;         // per-workgroup trace (isf_sparse_conv_trace, isf_sparse_conv_dma_trace)
static constexpr int kKernPhaseTrace = 2048;   // with kKernTrace: per-wave phase trace (isf_sparse_conv_phase_trace)
// the kernels' MODE bits of a BASE mode: the mode itself (F16_STORAGE = kKernF16Rows | kKernF16); -1: not a base mode
static constexpr int conv_kern_bits(int base) { return conv_mode_is_production(base) || conv_mode_is_knockout(base) ? base : -1; }

// ------------------------------------------------------------------------------------------------------------------
// THE INSTANTIATION CHOICE of the tile kernel: pure host arithmetic (tests/test_conv_choice.py walks it without a GPU).
// The channel shapes each kernel of the family is built for:
inline bool sparse_conv_f16x3_supported(int c_in, int c_out) {
  return (c_in == 32 || c_in == 64 || c_in == 128 || c_in == 256) &&
         (c_out == 32 || c_out == 64 || c_out == 128 || c_out == 256);
}
inline bool sparse_conv_dma_supported(int c_in, int c_out) { return (c_in == 32 || c_in == 64) && (c_out == 32 || c_out == 64); }
inline bool sparse_conv_deep_supported(int c_in, int c_out) { return (c_in == 128 || c_in == 256) && (c_out == 128 || c_out == 256); }

// Workgroup shape per layer, from the measured sweep (profiles/r02_call1_knockout_variants.txt, B=4 x 300 k points):
// 8 waves x 32 rows (256-row tiles, two workgroups per CU) for the layers with exactly 128 output columns
// (128 -> 128: 1.13 (4 waves) / 1.02 (16 waves) -> 0.94 ms per 4 launches; 64 -> 128: 0.142 -> 0.130 ms); everything
// else on 4 waves x 32 rows: the narrow layers lose with wider workgroups (fewer independent workgroups to hide the
// gather latency) and the 256-column layers of the small deep levels do not have enough tiles (8 waves: 1.41 -> 1.67 ms;
// 12 waves = one 384-row workgroup per CU: 1.42 -> 1.55 ms, profiles/r02_call3_sharing.txt).
static constexpr int kConv16NW = 4, kConv16RG = 2;   // the default shape: 4 waves x two 16-row groups (the deep kernel's only one)
inline bool conv16_wide_shape(int c_out, int n_out) { return c_out == 128 && n_out >= 8 * 256; }   // -> 8 waves
// SMALL LAUNCHES (round 5, profiles/r05_small_launch_ab.txt).  Below these row counts conv16_plan cuts a launch into HALF
// tiles only (every compute unit still gets a workgroup): on the two-group kernel a half tile leaves half of each wave's
// accumulators and of its prefetch registers idle.  The one-group instantiation (RG = 1: the same 16 rows per wave, the
// same tiles, the same order of operations per output element -- bit-identical) runs them 16-19 % faster: 256 -> 256 at
// 20 k rows 0.908 -> 0.764 ms per five launches, 128 -> 256 0.106 -> 0.088, 128 -> 128 at 30 k rows 0.434 -> 0.382 ms per four;
// single-sweep line 454 -> 507 frames/s, two sweeps 706 -> 765.  Above the bound full tiles win by as much (40 k rows:
// 1.22 -> 1.48 ms; 128 -> 128 at 119 k rows 0.835 -> 0.98 ms), so the bound is exactly where the plan stops being all-half:
// rows <= 3 workgroups x 4 groups x 16 rows x CUs / 2 column blocks (24 576 on 256 CUs) for the 256-column layers,
// rows <= 2 x 8 x 16 x CUs (65 536) for the 8-wave 128-column shape.
inline int conv16_small_rows_256(int cus) { return 96 * cus; }
inline int conv16_small_rows_wide(int cus) { return 256 * cus; }

enum { kConv16Tile = 0, kConv16Deep = 1 };   // Conv16Choice::backend: spconv_f16x3_kernel | isf_spconv_deep.hip
struct Conv16Choice {
  int backend;
  int nt, rg, nw;       // 16-column tiles per column block, 16-row groups per wave, waves: spconv_f16x3_kernel<c_in, nt, rg, nw, kern>
  int kern;             // kKern* bits
  bool uniform_tiles;   // the launch runs with ISF_CONV_MODE_UNIFORM_TILES whatever the caller's mode says
  bool drop_order;      // ... and without the caller's tile order / table
};
// ISF_CONV_MODE_* bits that only pick a shape or a variant: peeled off `mode` one after the other, in this order.  A variant
// takes the launch when what is left of the mode (tile bits aside) is EXACTLY its bit(s) and the layer is one it is built
// for; otherwise its bit is ignored.  What remains at the end is a base mode.
static constexpr int kConvModeOneBlock = ISF_CONV_MODE_ONE_BLOCK_4W | ISF_CONV_MODE_ONE_BLOCK_8W;
static constexpr int kConvModeShapeBits = kConvModeNarrowTiles | ISF_CONV_MODE_DEEP | kConvIssueOpts | kConvModeOneBlock;
// -> ISF_OK | ISF_ERR_UNSUPPORTED (channels) | ISF_ERR_ARG (the base mode left in mode & ~kConvModeShapeBits is none:
// single-pass precision and the knock-outs do not combine).  cus: the device's compute units.
inline int conv16_choose(int c_in, int c_out, int n_out, int mode, bool has_rowmap, int cus, Conv16Choice* out) {
  if (!sparse_conv_f16x3_supported(c_in, c_out)) return ISF_ERR_UNSUPPORTED;
  const bool deep = sparse_conv_deep_supported(c_in, c_out), nt8 = c_out >= 128;   // column blocks of 128, or the whole narrow layer
  const bool wide = conv16_wide_shape(c_out, n_out), small256 = deep && c_out == 256 && n_out <= conv16_small_rows_256(cus);
  *out = Conv16Choice{kConv16Tile, nt8 ? 8 : c_out / 16, kConv16RG, kConv16NW, 0, false, false};
  int m = mode & ~(kConvModeNarrowTiles | ISF_CONV_MODE_DEEP);
  const auto left = [&m](int bits) { return (m & ~kConvModeTileBits) == bits; };
  const auto variant = [out](int nw, int kern) { out->nw = nw; out->kern = kern; return ISF_OK; };
  // CHUNK_SPLIT (256-column layers; two workgroups per tile): the workgroup shape follows the small-launch rule
  if (deep && c_out == 256 && left(ISF_CONV_MODE_CHUNK_SPLIT)) { out->rg = small256 ? 1 : 2; return variant(4, kKernChunkSplit); }
  m &= ~ISF_CONV_MODE_CHUNK_SPLIT;
  // ONE_BLOCK_4W / _8W (round 5 experiment, valid results, bit-identical): the 256-COLUMN layers as ONE column block -- a
  // workgroup owns all 256 output columns of its rows, so a row is gathered ONCE per tap and chunk instead of once per
  // column block.  The phase trace (profiles/r05_att_256.txt) shows the step bound by the vector-memory issue path (a
  // gather in the MFMA operand layout costs 64 address cycles, 12 resident waves x (3 gathers + 4 weight DMA pieces) =
  // the step time): per MFMA this halves the gather instructions.  _4W: 4 waves x 32 rows (two workgroups per CU:
  // 64 KiB weight stage); _8W: 8 waves x 16 rows (one group per wave: no half tiles).  Tile-order tables belong to the
  // two-block launch plan: ignored.
  if (deep && c_out == 256 && !has_rowmap && (m & kConvModeOneBlock) && left(m & kConvModeOneBlock)) {
    const bool w8 = (m & ISF_CONV_MODE_ONE_BLOCK_8W) != 0;
    *out = Conv16Choice{kConv16Tile, 16, w8 ? 1 : 2, w8 ? 8 : 4, 0, w8, true};
    return ISF_OK;
  }
  m &= ~kConvModeOneBlock;
  // TWO_AHEAD: gathered rows two steps ahead (A2 loop; 4-wave shapes only)
  if (deep && !wide && left(ISF_CONV_MODE_TWO_AHEAD)) return variant(4, kKernTwoAhead);
  m &= ~ISF_CONV_MODE_TWO_AHEAD;
  // R4_ISSUE: round 4's issue phase (index reads in the step, four separate DMA pieces): A/B
  if (nt8 && left(ISF_CONV_MODE_R4_ISSUE)) return variant(wide ? 8 : 4, kKernR4Issue);
  m &= ~ISF_CONV_MODE_R4_ISSUE;
  // STAGGER: staggered issue phases (deep layers; valid results, bit-identical)
  if (nt8 && left(ISF_CONV_MODE_STAGGER)) return variant(wide ? 8 : 4, kKernStagger);
  m &= ~ISF_CONV_MODE_STAGGER;
  // a base mode other than 0: f16 storage and no-sharing on the production workgroup shapes, single-pass f16 (opt-in) and
  // the timing knock-outs on the 4-wave shape
  if (const int base = m & ~kConvModeTileBits) {
    if (conv_kern_bits(base) < 0) return ISF_ERR_ARG;
    const bool production = base == ISF_CONV_MODE_F16_STORAGE || base == ISF_CONV_MODE_NO_SHARING;
    return variant(production && wide ? 8 : 4, conv_kern_bits(base));
  }
  // mode 0.  kConvModeNarrowTiles (A/B): the wide layers on the 4-wave 128-row tile -- but not their small launches
  const bool small_wide = wide && n_out <= conv16_small_rows_wide(cus);
  if (small_wide || small256) out->rg = 1;   // small launches: one 16-row group per wave
  if (small_wide || (wide && !(mode & kConvModeNarrowTiles))) return variant(8, 0);
  // ISF_CONV_MODE_DEEP (opt-in, bit-identical, measured 8 % slower: profiles/r06_deep.txt): what is left on the default
  // shape of the deep layers, on isf_spconv_deep.hip (LDS-DMA gathers + one instruction stream per step; it reads no row
  // map and no part table)
  const bool use_deep = deep && !small256 && (mode & ISF_CONV_MODE_DEEP) && !has_rowmap && !(m & kConvModePartTable);
  if (use_deep) out->backend = kConv16Deep;
  return ISF_OK;
}
// The trace instantiations (mode: kKernTrace, + kKernPhaseTrace for the per-wave phase records) exist on the production
// workgroup shape of the two deep input widths: c_in 256, and 128 (which any other width is answered with).
inline Conv16Choice conv16_choose_trace(int c_in, int c_out, int n_out, int mode) {
  return Conv16Choice{kConv16Tile, 8, kConv16RG, c_in != 256 && conv16_wide_shape(c_out, n_out) ? 8 : kConv16NW,
                      kKernTrace | (mode & kKernPhaseTrace), false, false};
}

// narrow layers (CIN <= 64, <= 64 output columns) run all their 32-channel chunks in one step: half / the same
// number of barriers for twice the MFMAs per barrier
template <int CIN, int NT>
struct Conv16Step {
  static constexpr int KCH = (CIN <= 64 && NT <= 4) ? CIN / 32 : 1;      // 32-channel chunks per step
};

// LDS-DMA of 16 B per lane: LDS[lds_base + lane*16] = *gsrc.  Issued through inline asm on purpose: when hipcc
// sees a global_load_lds it drains vmcnt(0) before every later ds_read (it cannot prove the buffers differ),
// which would serialise the next step's weight/activation prefetch behind the current step's MFMAs.  Hidden
// here, the DMA stays in flight during the compute; the loops wait for it explicitly (s_waitcnt vmcnt(N) +
// barrier) right before the buffer is read.  M0 carries the wave-uniform LDS base and is restored.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_base_bytes /* wave-uniform */) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_base_bytes)
      : "memory");
}

// N consecutive KiB in one go: LDS[lds_base + i * 1024 + lane * 16] = gsrc[i * 64] for i < N -- ONE M0 set-up and N loads with
// immediate offsets (the offset field moves the global AND the LDS address).  The phase trace put the four separate
// glds16 of a wave's weight share at 410 cycles per step, 12 % of it (profiles/r05_att_256_v2.txt): each carried its own
// m0 save / set / nop / restore and address arithmetic.
template <int N>
__device__ __forceinline__ void glds16_run(const void* gsrc, unsigned lds_base_bytes /* wave-uniform */) {
  static_assert(N == 1 || N == 2 || N == 4, "1, 2 or 4 KiB");
  unsigned keep;
  if constexpr (N == 1)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_base_bytes) : "memory");
  else if constexpr (N == 2)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:1024\n\t"
                 "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_base_bytes) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:1024\n\t"
                 "global_load_lds_dwordx4 %1, off offset:2048\n\t"
                 "global_load_lds_dwordx4 %1, off offset:3072\n\t"
                 "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_base_bytes) : "memory");
}

// the hi halves only (single-pass f16 modes): of the N KiB of a run, the even ones -- N / 2 loads at offsets 0, 2048
template <int N>
__device__ __forceinline__ void glds16_run_hi(const void* gsrc, unsigned lds_base_bytes /* wave-uniform */) {
  static_assert(N == 2 || N == 4, "2 or 4 KiB");
  unsigned keep;
  if constexpr (N == 2)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_base_bytes) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:2048\n\t"
                 "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_base_bytes) : "memory");
}

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}

__device__ __forceinline__ void split8(const f32x8 v, uint4& hi, uint4& lo) {
  const h8 h = __builtin_convertvector(v, h8);
  const f32x8 r = v - __builtin_convertvector(h, f32x8);
  const h8 l = __builtin_convertvector(r, h8);
  hi = *reinterpret_cast<const uint4*>(&h);
  lo = *reinterpret_cast<const uint4*>(&l);
}

__device__ __forceinline__ f32x8 join8(const uint4 hi, const uint4 lo) {
  const h8 h = *reinterpret_cast<const h8*>(&hi);
  const h8 l = *reinterpret_cast<const h8*>(&lo);
  return __builtin_convertvector(h, f32x8) + __builtin_convertvector(l, f32x8);
}

// XCD-aware tile mapping: workgroups are dealt round-robin to the 8 XCDs (each with its own 4 MB L2) in
// linear-id order.  XCD x works through ONE CONTIGUOUS range of rows (rows are (b,z,y,x)-sorted, so the y / z
// neighbours a tile gathers are rows of tiles the same XCD touches a little earlier or later: its L2 holds that
// sliding window instead of every XCD fetching every row), and with two column blocks only ever on column block
// x & 1, so that the weights it streams are half of the layer's.
// A row range ("part": 4 with two column blocks, 8 with one) is cut into `full` tiles of TM rows followed by `half`
// tiles of TM / 2 rows (every wave of a half tile owns ONE 16-row group instead of two) -- see conv16_plan.
// -> false when this workgroup has no tile.
struct Conv16Plan {
  int full, half;   // tiles per part.  half < 0: TABLE mode -- `full` slots per part, slot j of a part works on the tile
                    // (first 16-row group, groups) the launch's tile table names (conv16_table_part)
  int part_rows;    // rows per part (a multiple of 16; the parts split the rows evenly whatever the tile mix)
};

static constexpr int kPlanParts = -2;   // Conv16Plan::half of a launch that reads a PART TABLE (equal-work parts, below):
                                        // `full` slots per part, slot j names one tile of the uniform plan or -1

// tile j of part `part` -> its first row, the first row past its share (the part's end or n_out, whichever comes
// first) and whether it is a half tile; false when the tile is empty.  Host and device: tests/test_tile_plan.py walks
// the same arithmetic the kernel uses.
__host__ __device__ inline bool conv16_tile_rows(Conv16Plan plan, int TM, int n_out, int part, int j, int& row0,
                                                 int& row_end, bool& half) {
  if (j >= plan.full + plan.half) return false;
  half = j >= plan.full;
  const int off = half ? plan.full * TM + (j - plan.full) * (TM / 2) : j * TM;
  row0 = part * plan.part_rows + off;
  const int part_end = (part + 1) * plan.part_rows;
  row_end = part_end < n_out ? part_end : n_out;
  return off < plan.part_rows && row0 < n_out;
}

// slot j of part `part` of a launch on a PART TABLE (plan.half == kPlanParts, plan.full = slots per part; the table:
// first [parts + 1] | class bounds [3] | slots [parts][plan.full]) -> the rows of the uniform tile the slot names; false for a
// slot without a tile.  Host and device (tests/test_part_plan.py walks a whole grid through it).
__host__ __device__ inline bool conv16_part_tile_rows(Conv16Plan plan, int TM, int n_out, int parts, const int32_t* table,
                                                      int part, int j, int& row0, int& row_end, bool& half) {
  const int t = table[parts + 1 + 3 + part * plan.full + j];
  if (t < 0) return false;
  const int per = (plan.part_rows + TM - 1) / TM;           // tiles per part of the uniform plan
  return conv16_tile_rows(Conv16Plan{per, 0, plan.part_rows}, TM, n_out, t / per, t - (t / per) * per, row0, row_end, half);
}

// order (optional): [parts][full + half] -- the tile workgroup slot j of a part works on (a permutation per part, built
// by conv16_tile_order_impl so that the tiles sharing a CU add up to about the same work).
__device__ __forceinline__ bool conv16_tile_of_block(int ncb, Conv16Plan plan, int TM, int n_out, int& cb, int& row0,
                                                     int& row_end, bool& half,
                                                     const int32_t* __restrict__ order = nullptr, int bid = -1) {
  if (bid < 0) bid = (int)blockIdx.x;     // (chunk-split launches: the workgroup's id within its half of the grid)
  const int xcd = bid & 7;
  int j = bid >> 3;
  cb = ncb == 2 ? xcd & 1 : 0;
  const int part = ncb == 2 ? xcd >> 1 : xcd;
  if (plan.half == kPlanParts) return conv16_part_tile_rows(plan, TM, n_out, ncb == 2 ? 4 : 8, order, part, j, row0, row_end, half);
  if (plan.half < 0) {   // tile table: (first group, groups) per slot; a tile of <= TM / 32 groups runs as a half tile
    const int g0 = order[2 * (part * plan.full + j)], ng = order[2 * (part * plan.full + j) + 1];
    row0 = g0 * 16;
    row_end = row0 + ng * 16 < n_out ? row0 + ng * 16 : n_out;
    half = ng * 32 <= TM;
    return ng > 0 && row0 < n_out;
  }
  if (order) j = order[part * (plan.full + plan.half) + j];
  return conv16_tile_rows(plan, TM, n_out, part, j, row0, row_end, half);
}
static inline int conv16_grid_blocks(Conv16Plan plan) { return 8 * (plan.half < 0 ? plan.full : plan.full + plan.half); }

// TILE TABLE of a launch that is resident in one round of workgroups: instead of cutting a part's rows into equal tiles
// (whose matrix work varies 3x with the density of the scene, so that the launch ends with its densest compute unit),
// the part's 16-row groups are dealt to the XCD's compute units as contiguous runs of about EQUAL WORK (work of a group =
// taps through which one of its rows has a neighbour, + a constant for its fixed cost), at most wgs_per_cu * gt groups
// per CU, and a CU's run is cut into full tiles of gt groups plus one tile with the remainder; tile k of CU c goes to
// workgroup slot c + cus * k, which is where the dispatcher puts it (round-robin over the XCD's CUs,
// tools/probes/wg_placement.hip).  Dense CUs get fewer rows, sparse ones more.  Host and device walk the same code
// (tests/test_tile_plan.py).  -> false when the part does not fit one round (the caller keeps the uniform plan).
static constexpr int kTableGroupBias = 2;
__host__ __device__ inline bool conv16_table_part(const int32_t* work, int G0, int G1, int cus, int wgs_per_cu, int gt,
                                                  int32_t* tiles /* [wgs_per_cu * cus][2] */) {
  const int slots = wgs_per_cu * cus, cap = wgs_per_cu * gt;
  for (int j = 0; j < 2 * slots; ++j) tiles[j] = 0;
  if (G1 - G0 > cus * cap) return false;
  long long rem = 0;
  for (int g = G0; g < G1; ++g) rem += work[g] + kTableGroupBias;
  int g = G0;
  for (int c = 0; c < cus && g < G1; ++c) {
    const int left_cus = cus - c, left_groups = G1 - g;
    const long long target = (rem + left_cus - 1) / left_cus;
    int must = left_groups - (left_cus - 1) * cap;     // what the others cannot hold
    if (must < 0) must = 0;
    int take = 0;
    long long acc = 0;
    while (g + take < G1 && take < cap) {
      const long long w = work[g + take] + kTableGroupBias;
      if (take >= must && (acc >= target || (take > 0 && acc + w - target > target - acc))) break;
      acc += w;
      ++take;
    }
    for (int k = 0, off = 0; off < take; ++k) {
      const int ng = take - off < gt ? take - off : gt;
      tiles[2 * (c + cus * k)] = g + off;
      tiles[2 * (c + cus * k) + 1] = ng;
      off += ng;
    }
    g += take;
    rem -= acc;
  }
  return g == G1;
}

// How a launch is cut into tiles.  The matrix pipe is per SIMD and a workgroup puts one wave (NW = 4) on each SIMD of
// its CU, so what bounds a launch that fits the chip in ONE round of workgroups is the largest number of 16-row groups
// any SIMD ends up with.  With uniform TM-row tiles that is wgs_per_cu * RG on the CUs that get a full set of
// workgroups while the others idle: 636 workgroups on 256 CUs x 3 slots = 6 groups per SIMD on 124 CUs, 4 on 132, for
// an average need of 4.97.  Mixing full and half tiles -- per CU f full + (wgs_per_cu - f) half, dealt in that order:
// the dispatcher places workgroups round-robin over the CUs of an XCD, every CU gets the same set
// (tools/probes/wg_placement.hip, profiles/r02_call13_tile_mix.txt) -- brings the maximum down to ceil(need).
// Launches of several rounds keep uniform tiles (the dispatcher refills slots as they drain).
// align_groups: every tile starts at a multiple of 16 * align_groups rows (the LDS-staged kernel works on 64-row units
// of the rulebook's staging tables: align_groups = 4; TM / 2 must be a multiple of it too).
static inline Conv16Plan conv16_plan(int n_out, int TM, int ncb, int wgs_per_cu, int cus_per_xcd, bool balance,
                                     int align_groups = 1) {
  const int parts = ncb == 2 ? 4 : 8;
  const int gt = TM / 16;                                       // 16-row groups per full tile
  const int groups = ceil_div(ceil_div(ceil_div(n_out, 16), parts), align_groups) * align_groups;   // per part = per XCD
  Conv16Plan plan{ceil_div(groups, gt), 0, groups * 16};
  if (!balance || (gt & 1) || plan.full > wgs_per_cu * cus_per_xcd) return plan;
  const int per_cu = ceil_div(groups, cus_per_xcd);
  int f = ceil_div(per_cu - wgs_per_cu * (gt / 2), gt / 2);
  f = f < 0 ? 0 : (f > wgs_per_cu ? wgs_per_cu : f);
  plan.full = min(f * cus_per_xcd, ceil_div(groups, gt));
  const int rest = groups - plan.full * gt;
  plan.half = rest > 0 ? ceil_div(rest, gt / 2) : 0;
  return plan;
}

// ------------------------------------------------------------------------------------------------------------------
// EQUAL-WORK PARTS of a launch of several rounds.  conv16_plan gives every XCD the same number of
// ROWS; the steps a tile walks (popcount of the OR of its rows' tap masks, x 32-channel chunks) vary 4x with the density
// of the scene, an XCD cannot give work away, and the launch ends with the XCD that was dealt the most steps (1.10 x the
// mean on the benchmark geometry).  Here the launch's uniform tiles -- the SAME tiles, tile t = tile t % full of the plan's
// part t / full -- are dealt to the XCDs as contiguous runs of about equal WEIGHT (steps + a constant for the tile's fixed
// cost), and inside a run the heavy tiles go to the first workgroup slots, so that what drains last is light.  Every XCD
// still owns one contiguous row range; every row is computed by the same tile: bit-identical.
// PART TABLE (device, built behind the neighbour table): first[parts + 1] | class bounds [3] | slots [parts][cap], slot j of
// part p = the tile it works on, -1 for none.  The launch passes Conv16Plan{cap, kPlanParts, part_rows} and the table as
// `order`; its grid is 8 * cap, sized from n_out alone.
static constexpr int kPartClasses = 4;         // work classes of the order inside a part
// Fixed cost of a tile in steps = (intercept b of the fit loop_us = a * steps + b, + prologue + epilogue) / a, from the
// per-workgroup trace of the launch shape on the benchmark geometry (tools/conv_trace.py --level 0 | 1,
// profiles/r06_dma_trace.txt and profiles/r07_launch_balance.txt):
//   32 -> 32 (level 0): (2.5 + 3.3 + 2.0) us / 0.925 us per step =  8 steps
//   64 -> 64 (level 1): (16.1 + 2.8 + 5.6) us / 0.929 us per step = 26 steps
// A shape without a trace of its own gets 0: its tiles are weighed by their steps alone.
__host__ __device__ inline int conv16_tile_fixed_steps(int c_in, int c_out) {
  if (c_in == 32 && c_out == 32) return 8;
  if (c_in == 64 && c_out == 64) return 26;
  return 0;
}
// tiles of the plan a part table deals out (plans without half tiles only)
__host__ __device__ inline int conv16_parts_tiles(int full, int parts) { return full * parts; }
// slots per part: the even share of the tiles + 1/8 + 1.  The census of the benchmark geometry needs +-7 % (the heaviest
// part's tiles are 0.93 x, the lightest's 1.07 x the even share); 12.5 % covers it with room for denser scenes, and what
// exceeds it is clamped (conv16_part_firsts), never lost.  An idle slot costs one workgroup that reads one word and exits.
__host__ __device__ inline int conv16_parts_cap(int T, int parts) {
  const int even = (T + parts - 1) / parts;
  return even + (even + 7) / 8 + 1;
}
__host__ __device__ inline int conv16_part_table_ints(int parts, int cap) { return parts + 1 + 3 + parts * cap; }
// W: inclusive prefix of the tile weights.  Unclamped cut k (0 < k < parts): behind the first tile whose prefix reaches
// k / parts of the total
__host__ __device__ inline int conv16_part_cut(const int32_t* W, int T, int parts, int k) {
  if (k <= 0) return 0;
  if (k >= parts) return T;
  const long long target = (long long)k * (long long)W[T - 1];
  int lo = 0, hi = T;                          // first t with W[t] * parts >= target
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)W[mid] * parts >= target) hi = mid; else lo = mid + 1;
  }
  return lo < T ? lo + 1 : T;
}
// first[parts + 1]: the cuts, every part clamped to `cap` tiles -- what a part cannot hold goes to the next, and a part
// takes at least what the parts behind it cannot hold (parts * cap >= T)
__host__ __device__ inline void conv16_part_firsts(const int32_t* W, int T, int parts, int cap, int32_t* first) {
  first[0] = 0;
  for (int k = 1; k < parts; ++k) {
    int c = conv16_part_cut(W, T, parts, k);
    const int hi = first[k - 1] + cap, lo = T - (parts - k) * cap;
    c = c < first[k - 1] ? first[k - 1] : c;
    c = c > hi ? hi : c;
    c = c < lo ? lo : c;
    first[k] = c;
  }
  first[parts] = T;
}
// class bounds from the histogram of the tile weights (hist[w], w < nbins): bound[q] = the smallest weight with at least
// (q + 1) / 4 of the tiles at or below it, so the classes hold about a quarter of the tiles each
__host__ __device__ inline void conv16_class_bounds(const int32_t* hist, int nbins, int32_t bound[3]) {
  int total = 0, acc = 0, q = 0;               // (weight 0 = a tile without rows: not counted)
  for (int w = 1; w < nbins; ++w) total += hist[w];
  for (int w = 1; w < nbins && q < 3; ++w) {
    acc += hist[w];
    while (q < 3 && (long long)acc * kPartClasses >= (long long)(q + 1) * total) bound[q++] = w;
  }
  while (q < 3) bound[q++] = nbins - 1;
}
// 0 = the heaviest class (runs first) .. 3 = the lightest
__host__ __device__ inline int conv16_work_class(int w, const int32_t bound[3]) {
  return (w <= bound[2]) + (w <= bound[1]) + (w <= bound[0]);
}
// slots of part k: its tiles by class, raster order inside a class (a stable counting sort: x / y-adjacent tiles stay
// resident together), -1 behind them.  (The device builds the same table a wave per part: conv16_part_table_kernel.)
__host__ __device__ inline void conv16_part_slots(const int32_t* w /* [T] tile weights */, const int32_t* first, int k, int cap,
                                                  const int32_t bound[3], bool raster, int32_t* slots /* [cap] */) {
  int n = 0;
  for (int c = 0; c < (raster ? 1 : kPartClasses); ++c)
    for (int t = first[k]; t < first[k + 1]; ++t)
      if (raster || conv16_work_class(w[t], bound) == c) slots[n++] = t;
  for (; n < cap; ++n) slots[n] = -1;
}

// ------------------------------------------------------------------------------------------------------------------
// Unit plan of the one-workgroup-per-CU kernel (isf_spconv_cu.hip).  The rows of a launch are cut into UNITS of whole
// 16-row groups, every unit carrying about the same matrix work -- work of a group = the taps through which at least one
// of its rows has a neighbour = what it issues MFMAs for -- so that each compute unit gets one unit (or r of them) and
// they all finish together, whatever the density of the scene under them.  Host and device walk the same arithmetic
// (tests/test_tile_plan.py): cut u of U0 = first group whose inclusive work prefix exceeds u * total / U0; a unit longer
// than kCuCapGroups groups (what one workgroup's accumulators hold) is split evenly.
static constexpr int kCuCapGroups = 16;       // 256 rows x 256 columns of fp32 accumulators in 8 waves x 128 registers
static constexpr int kCuAvgGroups = 12;       // a launch gets cus * r balanced units with n_groups / (cus * r) <= this

// Two shapes (round 6): cap 16 = one 8-wave workgroup per compute unit (the unit's 256 x 256 accumulator tile is the CU's
// register file); cap 8 = two 4-wave workgroups per compute unit, each over a unit of <= 8 groups (128 rows x 256 columns,
// a wave = 8 groups x 64 columns): the two workgroups of a CU run unsynchronised, one's load-issue phase under the other's
// multiply phase.  `slots` = compute units x workgroups per compute unit.
static constexpr int kCuCapGroups8 = 8;
static constexpr int kCuAvgGroups8 = 6;
__host__ __device__ inline int conv_cu_avg_of_cap(int cap) { return cap == kCuCapGroups8 ? kCuAvgGroups8 : kCuAvgGroups; }
__host__ __device__ inline int conv_cu_balanced_units(int n_groups, int slots, int cap = kCuCapGroups) {
  const int per = slots * conv_cu_avg_of_cap(cap);
  const int r = n_groups > per ? (n_groups + per - 1) / per : 1;
  return slots * r;
}
// upper bound of the final unit count (splitting adds at most one unit per `cap` groups)
__host__ __device__ inline int conv_cu_max_units(int n_groups, int slots, int cap = kCuCapGroups) {
  return conv_cu_balanced_units(n_groups, slots, cap) + (n_groups + cap - 1) / cap;
}
// first group of balanced unit u (0 <= u <= U0): W = inclusive prefix of the per-group work
__host__ __device__ inline int conv_cu_cut(const int32_t* W, int n_groups, int U0, int u) {
  if (u <= 0) return 0;
  if (u >= U0) return n_groups;
  const long long target = (long long)u * (long long)W[n_groups - 1] / U0;
  int lo = 0, hi = n_groups;                 // first i with W[i] > target
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)W[mid] > target) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__host__ __device__ inline int conv_cu_pieces(int len, int cap = kCuCapGroups) { return len <= 0 ? 0 : (len + cap - 1) / cap; }
// piece p of a balanced unit of `len` groups starting at group c -> (first group, groups)
__host__ __device__ inline void conv_cu_piece(int c, int len, int p, int& g0, int& ng, int cap = kCuCapGroups) {
  const int P = conv_cu_pieces(len, cap);
  const int a = (int)((long long)p * len / P), b = (int)((long long)(p + 1) * len / P);
  g0 = c + a;
  ng = b - a;
}

// Epilogue shared by both kernels: per 16-row group, accumulator (col = lane&15, row = 4*(lane>>4)+t) -> LDS row-major
// (wave-private transpose tile) -> one lane per (row, 8-channel unit): BN fold (incl. the weight scale), residual,
// ReLU, split, store.  The 8 BN scales / shifts of an item are fetched with two 32-byte loads issued together (the
// scalar form compiled to a load-wait pair per channel: 128 dependent round trips per wave and tile; measured
// 4.49 -> 4.09 ms per step over the 21 convs, profiles/r02_call1_knockout_variants.txt).
// tile_l: this wave's 16 x (16*EPN+4) fp32 LDS tile.  All rows of the wave: row0w .. row0w + 16*RG.
template <int NT, int RG>
struct Conv16Epi {
  static constexpr int EPN = NT > 4 ? 4 : NT;            // column tiles per pass (keeps the transpose tile small)
  static constexpr int RS = 16 * EPN + 4;
  static constexpr int wave_bytes = 16 * RS * 4;
};

// F16IO: residual and output rows are plain f16 ([N][C] halves, 2 bytes per element: the "half format" of the f16
// storage mode) instead of split rows: one 16-byte piece per 8-channel unit at row * (C / 8) + unit.
template <int NT, int RG, bool F16IO = false>
__device__ __forceinline__ void conv16_epilogue(const f32x4 (&acc)[RG][NT], float* tile_l, int lane, int row0w,
                                                int col0 /* first output channel of this workgroup */, int cout,
                                                float winv, const float* __restrict__ scale,
                                                const float* __restrict__ shift, const uint4* __restrict__ residual,
                                                uint4* __restrict__ ys, int n_out, int relu, int groups = RG,
                                                const int32_t* __restrict__ rowmap = nullptr /* position -> row */) {
  using E = Conv16Epi<NT, RG>;
  constexpr int EPN = E::EPN, RS = E::RS;
  const int col = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    if (rg >= groups) continue;                        // half tiles / short units: the upper row groups do not exist
                                                       // (continue, not break: a break keeps hipcc from unrolling RG = 16
                                                       // and the accumulators would be indexed through scratch memory)
#pragma unroll
    for (int ps = 0; ps < NT / EPN; ++ps) {
      constexpr int UNITS = (16 * EPN) / 8;           // 8-channel units per row in this pass
      constexpr int ITEMS = (16 * UNITS + 63) / 64;   // (row, unit) items per lane
      // the residual rows of this pass are requested before the LDS transpose, so their latency hides behind it
      uint4 res_hi[ITEMS], res_lo[ITEMS];
      if (residual) {
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
          const int i = lane + 64 * it;
          const int grow = row0w + rg * 16 + i / UNITS;
          res_hi[it] = make_uint4(0, 0, 0, 0);
          res_lo[it] = make_uint4(0, 0, 0, 0);
          if (i < 16 * UNITS && grow < n_out) {
            const int unit = (col0 + ps * (16 * EPN)) / 8 + i % UNITS;
            const int gm = rowmap ? rowmap[grow] : grow;      // the row this position of the (sorted) launch computes
            if (F16IO) {
              res_hi[it] = residual[(size_t)gm * (cout >> 3) + unit];
            } else {
              const size_t o = split_hi_index((size_t)gm, cout >> 3, unit);
              res_hi[it] = residual[o];
              res_lo[it] = residual[o + 4];
            }
          }
        }
      }
#pragma unroll
      for (int nt = 0; nt < EPN; ++nt)
#pragma unroll
        for (int t = 0; t < 4; ++t) tile_l[(4 * kg + t) * RS + nt * 16 + col] = acc[rg][ps * EPN + nt][t];
      // wave-private tile: a wave-level fence is enough (LDS ops of one wave complete in order)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      for (int it = 0; it < ITEMS; ++it) {
        const int i = lane + 64 * it;
        const int r = i / UNITS, u = i % UNITS;
        const int grow = row0w + rg * 16 + r;
        if (i < 16 * UNITS && grow < n_out) {
          const float* tp = tile_l + r * RS + u * 8;
          f32x8 v;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = tp[j];
          const int gc = col0 + ps * (16 * EPN) + u * 8;
          f32x8 sc8, sh8;
#pragma unroll
          for (int j = 0; j < 8; ++j) { sc8[j] = 1.f; sh8[j] = 0.f; }
          if (scale) sc8 = *reinterpret_cast<const f32x8*>(scale + gc);
          if (shift) sh8 = *reinterpret_cast<const f32x8*>(shift + gc);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = fmaf(v[j], scale ? sc8[j] * winv : winv, sh8[j]);
          if (residual) v += join8(res_hi[it], res_lo[it]);   // F16IO: res_lo is zero
          if (relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
          }
          uint4 hi, lo;
          split8(v, hi, lo);
          const int gm = rowmap ? rowmap[grow] : grow;
          if (F16IO) {
            ys[(size_t)gm * (cout >> 3) + (gc >> 3)] = hi;   // round-to-nearest f16 of the fp32 result
          } else {
            const size_t o = split_hi_index((size_t)gm, cout >> 3, gc >> 3);
            ys[o] = hi;
            ys[o + 4] = lo;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
  }
}

}  // namespace isf
