// isf_sort.hip -- the library's one stable sort: 32-bit keys, LSD radix, hand-written (stable_sort_u32_impl).  Its callers:
// the pillar voxelization (isf_voxelize.hip), the row sorts of the sparse convolutions (isf_spconv16.hip), the evaluator's
// order (isf_eval.hip) and isf_ingroup_indices (isf_boundary.hip).
#include "isf_common.h"
#include "isf_sort.h"

namespace isf {

// ---------------------------------------------------------------------------------------------------------------------
// The stable sort itself (round 6; hand-written, replaces rocprim::radix_sort_pairs -- 8 launches, 270 us per two-sample
// forward, one of them 214 us: a library tuned for arrays a thousand times larger).  LSD radix sort, `bits` (<= 10) key
// bits per pass, WAVE MULTI-SPLIT ranking: a wave owns a tile of kRsTile consecutive elements and walks it in order, 64 at
// a time; `bits` ballots tell every lane which lanes hold the same digit (mask &= my bit ? ballot : ~ballot), so its rank
// among them is a popcount and the group's first lane keeps the wave's running count of the digit in LDS -- no atomics,
// no sorting network, stable by construction (lanes, sub-tiles and tiles are all taken in index order).
//   count pass   per (digit, tile) counts                -> hist [digits][tiles]   (digit-major: the order of the output)
//   row scan     per digit: exclusive prefix over its tiles, and its total
//   scatter pass out[first position of the digit + hist[digit][tile] + running count in the tile + rank in the sub-tile]
constexpr int kRsTile = 1024;     // elements per wave (16 sub-tiles): 293 waves for 300 k points
constexpr int kRsWaves = 4;       // waves (tiles) per workgroup

template <bool SCATTER>
__global__ __launch_bounds__(64 * kRsWaves) void hv_radix_pass_kernel(const uint32_t* __restrict__ keys_in,
                                                                      const int* __restrict__ vals_in /* nullptr: identity */,
                                                                      int n, int shift, int bits, int tiles,
                                                                      uint32_t* __restrict__ hist,
                                                                      const uint32_t* __restrict__ totals /* [digits] */,
                                                                      uint32_t* __restrict__ keys_out, int* __restrict__ vals_out) {
  __shared__ uint32_t cnt_s[kRsWaves][1024];
  __shared__ uint32_t dbase_s[1024];                 // SCATTER: first output position of every digit
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * kRsWaves + wave;
  const int nd = 1 << bits;
  if (SCATTER) {                                     // exclusive prefix of the digit totals (<= 1024 values: one wave)
    if (wave == 0) {
      uint32_t run = 0u;
      for (int b0 = 0; b0 < nd; b0 += 64) {
        const uint32_t v = totals[b0 + lane];
        uint32_t x = v;
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
          const uint32_t o = __shfl_up(x, dlt, 64);
          if (lane >= dlt) x += o;
        }
        dbase_s[b0 + lane] = run + x - v;
        run += __shfl(x, 63, 64);
      }
    }
    __syncthreads();
  }
  if (tile >= tiles) return;
  volatile uint32_t* cnt = cnt_s[wave];
  for (int d = lane; d < nd; d += 64) cnt[d] = 0u;
  __builtin_amdgcn_wave_barrier();
  const unsigned long long lt = (1ull << lane) - 1ull;
  // the tile's keys (and values) are requested up front: kRsTile / 64 independent loads in flight per lane instead of one
  // exposed round trip per sub-tile (147 waves walking 32 dependent round trips each made a pass 50 us)
  constexpr int NSUB = kRsTile / 64;
  uint32_t kreg[NSUB];
  int vreg[NSUB];
#pragma unroll
  for (int sub = 0; sub < NSUB; ++sub) {
    const int i = tile * kRsTile + sub * 64 + lane;
    kreg[sub] = i < n ? keys_in[i] : 0u;
    vreg[sub] = (SCATTER && i < n) ? (vals_in ? vals_in[i] : i) : 0;
  }
#pragma unroll
  for (int sub = 0; sub < NSUB; ++sub) {
    const int i = tile * kRsTile + sub * 64 + lane;
    const bool valid = i < n;
    const uint32_t key = kreg[sub];
    const uint32_t d = (key >> shift) & (uint32_t)(nd - 1);
    unsigned long long m = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const int rank = __popcll(m & lt), group = __popcll(m);
    uint32_t base = 0u;
    if (valid) base = cnt[d];                       // every lane of a digit group reads the count before ...
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) cnt[d] = base + (uint32_t)group;   // ... its first lane advances it (one address per group)
    __builtin_amdgcn_wave_barrier();
    if (SCATTER && valid) {
      const uint32_t pos = dbase_s[d] + hist[(size_t)d * tiles + tile] + base + (uint32_t)rank;
      keys_out[pos] = key;
      vals_out[pos] = vreg[sub];
    }
  }
  if (!SCATTER)
    for (int d = lane; d < nd; d += 64) hist[(size_t)d * tiles + tile] = cnt[d];
}

// per digit (one wave each): exclusive prefix of its row of per-tile counts in place (coalesced, ceil(tiles / 64) rounds)
// and the digit's total; the scatter pass turns the totals into the digits' first output positions itself.  (A single
// workgroup scanning all digits x tiles entries with a chunk per thread was 100 us of dependent, uncoalesced loads.)
__global__ __launch_bounds__(256) void hv_radix_rowscan_kernel(uint32_t* __restrict__ hist, int nd, int tiles,
                                                               uint32_t* __restrict__ totals) {
  const int lane = threadIdx.x & 63, d = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= nd) return;
  uint32_t* row = hist + (size_t)d * tiles;
  uint32_t run = 0u;
  for (int b0 = 0; b0 < tiles; b0 += 64) {
    const int t = b0 + lane;
    const uint32_t v = t < tiles ? row[t] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const uint32_t o = __shfl_up(x, dlt, 64);
      if (lane >= dlt) x += o;
    }
    if (t < tiles) row[t] = run + x - v;
    run += __shfl(x, 63, 64);
  }
  if (lane == 0) totals[d] = run;
}

// the keys in an earlier order: what a sort that continues `after` starts from (kept out of the pass kernel, whose loads
// stay direct)
__global__ void sort_gather_keys_kernel(const uint32_t* __restrict__ keys, const int* __restrict__ after, int n,
                                        uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = keys[after[i]];
}

// idx_sorted [n] = the stable order of keys [n] by their low `key_bits` bits (1 .. 32) and by NOTHING above them
// (stable_sort_plan, isf_sort.h); scratch from the arena.
//   keys_sorted  the caller's [n] buffer when it wants keys[idx_sorted[j]] as well, else nullptr
//   after        a permutation p of 0 .. n - 1 from an earlier sort: the result is the stable order of keys[p[0]],
//                keys[p[1]], ... expressed in original indices (idx_sorted[j] is an element of p) -- sorting the minor key
//                first and the major key `after` it gives the lexicographic order.  Must not be idx_sorted itself.
int stable_sort_u32_impl(Arena& a, const uint32_t* keys, int n, int key_bits, int* idx_sorted, hipStream_t st,
                         uint32_t* keys_sorted, const int* after) {
  ISF_REQUIRE(keys && idx_sorted && n > 0 && key_bits >= 1 && key_bits <= 32 && after != idx_sorted, ISF_ERR_ARG,
              "stable_sort: bad arguments");
  const int tiles = ceil_div(n, kRsTile), blocks = ceil_div(tiles, kRsWaves);
  uint32_t *keys_tmp = nullptr, *hist = nullptr;
  int* idx_tmp = nullptr;
  ISF_TRY(a.alloc_n(&keys_tmp, (size_t)n));
  if (!keys_sorted) ISF_TRY(a.alloc_n(&keys_sorted, (size_t)n));
  ISF_TRY(a.alloc_n(&idx_tmp, (size_t)n));
  ISF_TRY(a.alloc_n(&hist, (size_t)1024 * (tiles + 1)));
  uint32_t* totals = hist + (size_t)1024 * tiles;
  const uint32_t* kin = keys;
  const int* vin = nullptr;
  if (after) {
    uint32_t* keys_after = nullptr;
    ISF_TRY(a.alloc_n(&keys_after, (size_t)n));
    hipLaunchKernelGGL(sort_gather_keys_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, keys, after, n, keys_after);
    kin = keys_after;
    vin = after;
  }
  const SortPlan pl = stable_sort_plan(key_bits);
  for (int p = 0; p < pl.passes; ++p) {
    // ping-pong so that the LAST pass writes the caller's output buffers
    const bool to_out = ((pl.passes - 1 - p) & 1) == 0;
    uint32_t* kout = to_out ? keys_sorted : keys_tmp;
    int* vout = to_out ? idx_sorted : idx_tmp;
    const int shift = p * pl.bits[0], bits = pl.bits[p];
    hipLaunchKernelGGL(hv_radix_pass_kernel<false>, dim3(blocks), dim3(64 * kRsWaves), 0, st, kin, vin, n, shift, bits, tiles,
                       hist, totals, kout, vout);
    hipLaunchKernelGGL(hv_radix_rowscan_kernel, dim3(ceil_div(1 << bits, 4)), dim3(256), 0, st, hist, 1 << bits, tiles, totals);
    hipLaunchKernelGGL(hv_radix_pass_kernel<true>, dim3(blocks), dim3(64 * kRsWaves), 0, st, kin, vin, n, shift, bits, tiles,
                       hist, totals, kout, vout);
    kin = kout;
    vin = vout;
  }
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // namespace isf

extern "C" {

int isf_debug_stable_sort(const uint32_t* keys, int num, int key_bits, const int32_t* after, int32_t* order,
                          uint32_t* keys_sorted, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num >= 0 && key_bits >= 1 && key_bits <= 32, ISF_ERR_ARG, "debug_stable_sort: bad arguments");
  if (num == 0) return ISF_OK;
  ISF_REQUIRE(keys && order, ISF_ERR_ARG, "debug_stable_sort: null pointer");
  hipStream_t st = as_stream(stream);
  Arena& a = arena_for_stream(st);
  ISF_TRY(a.reset());
  return stable_sort_u32_impl(a, keys, num, key_bits, order, st, keys_sorted, after);
}

}  // extern "C"
