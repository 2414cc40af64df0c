// isf_voxelize.hip -- A1 dynamic voxelization, A2 deterministic hard (pillar) voxelization.
//
// A2 design (replaces the reference's O(P^2) point_to_voxelidx_kernel + single-thread
// determin_voxel_num, voxelization_cuda.cu:105-180):
//   1. every point bubbles its index into a per-cell sorted list of the max_points smallest point
//      indices (one atomicMin per slot; order-independent, deterministic result);
//   2. a cell's voxel id in "first appearance" order is the rank of its smallest point index among
//      all cells' smallest indices -> one bitmap over point indices + the popcount-prefix scan;
//   3. one gather pass writes voxels / coors / num_points for ids < max_voxels.
// All of it is HBM/L2-bound integer work: O(P * max_points) atomics worst case, O(P) typical.
#include <cstring>


#include "isf_common.h"

namespace isf {

__global__ void dynamic_voxelize_kernel(const float* __restrict__ points, int P, int C, VoxGeom g,
                                        int32_t* __restrict__ coors, int stride, int col0,
                                        int batch_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  int cx, cy, cz;
  const bool ok = voxel_of_point(points + (size_t)i * C, g.vx, g.vy, g.vz, g.x0, g.y0, g.z0, g.gx, g.gy,
                                 g.gz, cx, cy, cz);
  int32_t* o = coors + (size_t)i * stride;
  if (col0) o[0] = batch_idx;
  o[col0 + 0] = ok ? cz : -1;
  o[col0 + 1] = ok ? cy : -1;
  o[col0 + 2] = ok ? cx : -1;
}

int dynamic_voxelize_impl(const float* points, int P, int C, const float vs[3], const float range[6],
                          int32_t* coors, int coors_stride, int coors_col0, int batch_idx,
                          hipStream_t st) {
  if (P <= 0) return ISF_OK;
  hipLaunchKernelGGL(dynamic_voxelize_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, points, P, C,
                     make_geom(vs, range), coors, coors_stride, coors_col0, batch_idx);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

// ------------------------------------------------------------------------------------------- A2
static constexpr int kEmpty = 0x7f7f7f7f;  // hipMemset byte pattern 0x7f; larger than any point index

// The samples of a batch voxelized in ONE pass (isf_hard_voxelize_batched_device): the points are concatenated, sample b owns
// the point indices [off[b], off[b + 1]) and the grid planes [b * gz, (b + 1) * gz) of a grid stacked along z.  Point indices
// ascend with the sample, so "rank of a cell's first point" numbers sample 0's voxels first, then sample 1's ...
static constexpr int kHvMaxBatch = 16;
struct HvBatch {
  int n;
  int off[kHvMaxBatch + 1];
};
__device__ __forceinline__ int hv_sample_of(const HvBatch& hb, int i) {
  int b = 0;
#pragma unroll
  for (int k = 1; k < kHvMaxBatch; ++k) b += (k < hb.n && i >= hb.off[k]) ? 1 : 0;
  return b;
}

__global__ void hv_mark_cells_kernel(const float* __restrict__ points, int P, int C, VoxGeom g, HvBatch hb,
                                     unsigned long long* __restrict__ cbits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  int cx, cy, cz;
  if (!voxel_of_point(points + (size_t)i * C, g.vx, g.vy, g.vz, g.x0, g.y0, g.z0, g.gx, g.gy, g.gz, cx,
                      cy, cz))
    return;
  cz += hv_sample_of(hb, i) * g.gz;
  const unsigned long long cell = ((unsigned long long)cz * g.gy + cy) * g.gx + cx;
  const unsigned long long bit = 1ull << (cell & 63);
  unsigned long long* p = cbits + (cell >> 6);
  if (!(*p & bit)) atomicOr(p, bit);
}

// byte-map marking for small grids (pillars: 32 k cells): plain byte stores instead of device-scope atomicOr on a few
// hundred hot words (memory-side atomics serialise per address: 257 us for 300 k points), then one pack pass
__global__ void hv_mark_bytes_kernel(const float* __restrict__ points, int P, int C, VoxGeom g, HvBatch hb,
                                     unsigned char* __restrict__ seen) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  int cx, cy, cz;
  if (!voxel_of_point(points + (size_t)i * C, g.vx, g.vy, g.vz, g.x0, g.y0, g.z0, g.gx, g.gy, g.gz, cx,
                      cy, cz))
    return;
  cz += hv_sample_of(hb, i) * g.gz;
  seen[((size_t)cz * g.gy + cy) * g.gx + cx] = 1;
}

__global__ void hv_pack_bytes_kernel(const unsigned char* __restrict__ seen, size_t ncells, size_t nwords,
                                     unsigned long long* __restrict__ bits) {
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  unsigned long long v = 0;
  for (int j = 0; j < 64; ++j) {
    const size_t c = w * 64 + j;
    if (c < ncells && seen[c]) v |= 1ull << j;
  }
  bits[w] = v;
}

// points of a cell = one segment of the point indices STABLY sorted by the cell's rank (radix sort over the rank's bits,
// stable_sort_u32_impl, isf_sort.hip): inside a segment the indices ascend, so a cell's T smallest point indices -- what the reference's
// sequential scan keeps (voxelization_cpu.cpp:54-69) -- are the first T of its segment.  Deterministic, no atomics.
// History: v1 atomicMin bubble insertion (720 us per 300 k points in pillars), v2 count -> scan -> fill -> select with
// one atomic per point per pass (90 + 16 + 90 + 55 us: the pillar grid's hot cells serialise the atomics).
__global__ void hv_keys_kernel(const float* __restrict__ points, int P, int C, VoxGeom g, HvBatch hb,
                               const unsigned long long* __restrict__ cbits, const uint32_t* __restrict__ cprefix,
                               uint32_t none, uint32_t* __restrict__ keys, int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  int cx, cy, cz;
  uint32_t key = none;   // points outside the grid sort behind every cell (none = row capacity > any rank)
  if (voxel_of_point(points + (size_t)i * C, g.vx, g.vy, g.vz, g.x0, g.y0, g.z0, g.gx, g.gy, g.gz, cx, cy, cz))
    key = (uint32_t)occ_lookup(cbits, cprefix,
                               ((unsigned long long)(cz + hv_sample_of(hb, i) * g.gz) * g.gy + cy) * g.gx + cx);
  keys[i] = key;
  if (idx) idx[i] = i;     // (the sort takes the identity permutation implicitly)
}

// first sorted position of every cell
__global__ void hv_segment_heads_kernel(const uint32_t* __restrict__ keys, int P, uint32_t none,
                                        uint32_t* __restrict__ start) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  const uint32_t k = keys[j];
  if (k != none && (j == 0 || keys[j - 1] != k)) start[k] = (uint32_t)j;
}

__global__ void hv_segment_slots_kernel(const uint32_t* __restrict__ keys, const int* __restrict__ idx, int P,
                                        const uint32_t* __restrict__ start, uint32_t none, int T,
                                        int* __restrict__ slots /*[rows][T], pre-filled kEmpty*/) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  const uint32_t k = keys[j];
  if (k == none) return;
  const uint32_t t = (uint32_t)j - start[k];
  if (t < (uint32_t)T) slots[(size_t)k * T + t] = idx[j];
}

__global__ void hv_mark_first_kernel(const int* __restrict__ slots, const int* __restrict__ nrows,
                                     int T, unsigned long long* __restrict__ pbits) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= *nrows) return;
  const int first = slots[(size_t)r * T];
  atomicOr(pbits + (first >> 6), 1ull << (first & 63));
}

// number of set bits before position x of an occupancy index over point indices (x <= number of positions)
__device__ __forceinline__ int hv_rank_before(const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ prefix,
                                              int x, int npos, const int* __restrict__ total) {
  if (x >= npos) return *total;
  const unsigned long long w = bits[x >> 6];
  return (int)prefix[x >> 6] + __popcll(w & ((1ull << (x & 63)) - 1ull));
}

// batched (hb.n > 1 or coors4 output): voxel ids are local to the sample (id among ALL first points - first points of the
// earlier samples), capped per sample, and the samples' voxels are written one behind the other (row = voxels kept by the
// earlier samples + local id) with (sample, z, y, x) coordinates -- what the reference's per-sample loop + cat + pad produce
__global__ void hv_gather_kernel(const float* __restrict__ points, int C, const int* __restrict__ slots,
                                 const int* __restrict__ nrows, const int32_t* __restrict__ cell_coors4,
                                 int T, const unsigned long long* __restrict__ pbits,
                                 const uint32_t* __restrict__ pprefix, int max_voxels,
                                 float* __restrict__ voxels, int32_t* __restrict__ coors,
                                 int32_t* __restrict__ num_points, int fill_empty, HvBatch hb, int gz, int batched,
                                 const int* __restrict__ ptotal) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long long)(*nrows) * T) return;
  const int r = (int)(tid / T), t = (int)(tid % T);
  const int* s = slots + (size_t)r * T;
  int vid = occ_lookup(pbits, pprefix, (unsigned long long)s[0]);
  int b = 0;
  if (batched) {
    b = hv_sample_of(hb, s[0]);
    const int npos = hb.off[hb.n];
    int row0 = 0, before = 0;   // voxels kept by the earlier samples; first points of the earlier samples
    for (int k = 0; k < b; ++k) {
      const int nxt = hv_rank_before(pbits, pprefix, hb.off[k + 1], npos, ptotal);
      const int cnt = nxt - before;
      row0 += cnt < max_voxels ? cnt : max_voxels;
      before = nxt;
    }
    vid -= before;
    if (vid < 0 || vid >= max_voxels) return;
    vid += row0;
  } else if (vid < 0 || vid >= max_voxels) {
    return;
  }
  const int pi = s[t];
  if (pi != kEmpty) {
    const float* p = points + (size_t)pi * C;
    float* o = voxels + ((size_t)vid * T + t) * C;
    for (int k = 0; k < C; ++k) o[k] = p[k];
  } else if (fill_empty) {                       // the caller did not zero the output: write the padding slots here
    float* o = voxels + ((size_t)vid * T + t) * C;
    for (int k = 0; k < C; ++k) o[k] = 0.f;
  }
  if (t == 0) {
    int n = 0;
    for (int k = 0; k < T; ++k) n += (s[k] != kEmpty);
    num_points[vid] = n;
    const int4 c = reinterpret_cast<const int4*>(cell_coors4)[r];  // (0, z, y, x); batched: z = sample * gz + z
    if (batched) {
      coors[(size_t)vid * 4 + 0] = b;
      coors[(size_t)vid * 4 + 1] = c.y - b * gz;
      coors[(size_t)vid * 4 + 2] = c.z;
      coors[(size_t)vid * 4 + 3] = c.w;
    } else {
      coors[(size_t)vid * 3 + 0] = c.y;
      coors[(size_t)vid * 3 + 1] = c.z;
      coors[(size_t)vid * 3 + 2] = c.w;
    }
  }
}

__global__ void hv_publish_count_kernel(const int* __restrict__ total, int max_voxels, int32_t* __restrict__ out) {
  *out = *total < max_voxels ? *total : max_voxels;
}

// batched: out[b] = voxels kept of sample b, out[n] = their sum (= rows written)
__global__ void hv_publish_counts_kernel(const unsigned long long* __restrict__ pbits, const uint32_t* __restrict__ pprefix,
                                         const int* __restrict__ total, HvBatch hb, int max_voxels,
                                         int32_t* __restrict__ out) {
  int before = 0, sum = 0;
  for (int b = 0; b < hb.n; ++b) {
    const int nxt = hv_rank_before(pbits, pprefix, hb.off[b + 1], hb.off[hb.n], total);
    const int cnt = nxt - before < max_voxels ? nxt - before : max_voxels;
    out[b] = cnt;
    sum += cnt;
    before = nxt;
  }
  out[hb.n] = sum;
}

// voxel_num_dev != nullptr: DEVICE-RESIDENT COUNT -- no host read-back (the caller sized the outputs for max_voxels and
// did not zero them: rows [0, *voxel_num_dev) are written completely, padding slots included; the rest is untouched)
// batch != nullptr (with voxel_num_dev): the samples of a batch in one pass -- `points` holds them one behind the other,
// coors is [rows, 4] = (sample, z, y, x), voxel_num_dev has n + 1 entries (per sample, then the sum); see HvBatch
int hard_voxelize_impl(Arena& a, const float* points, int P, int C, const float vs[3],
                       const float range[6], int max_points, int max_voxels, float* voxels,
                       int32_t* coors, int32_t* num_points, int* voxel_num_host, hipStream_t st,
                       int32_t* voxel_num_dev = nullptr, const HvBatch* batch = nullptr) {
  const VoxGeom g = make_geom(vs, range);
  ISF_REQUIRE(g.gx > 0 && g.gy > 0 && g.gz > 0, ISF_ERR_ARG, "hard_voxelize: empty grid");
  if (voxel_num_host) *voxel_num_host = 0;
  HvBatch hb;
  for (int k = 0; k <= kHvMaxBatch; ++k) hb.off[k] = P;
  hb.n = 1;
  hb.off[0] = 0;
  if (batch) hb = *batch;
  const int nb = hb.n;
  if (P <= 0) {
    if (voxel_num_dev) ISF_HIP_TRY(hipMemsetAsync(voxel_num_dev, 0, (batch ? nb + 1 : 1) * sizeof(int32_t), st));
    return ISF_OK;
  }
  const long long cells = (long long)g.gx * g.gy * g.gz * nb;
  const int row_cap = (int)(cells < P ? cells : P);
  OccIndex cocc;  // occupied cells of this sample
  OccIndex pocc;  // bitmap over POINT indices: rank of a cell's first point = its voxel id
  int* slots = nullptr;
  ISF_TRY(a.alloc_n(&slots, (size_t)row_cap * max_points));
  const bool bytes_path = cells <= (1ll << 22);
  if (bytes_path) {
    // the four fills of the pass -- cell index, byte map, point index (zero: incl. the padding words the scans read) and the
    // slot table (kEmpty) -- in one launch
    ISF_TRY(occ_create(a, &cocc, 1, g.gz * nb, g.gy, g.gx, st, false));
    ISF_TRY(occ_create(a, &pocc, 1, 1, 1, P, st, false));
    unsigned char* seen = nullptr;
    ISF_TRY(a.alloc_n(&seen, (size_t)cells));
    void* fp[4] = {cocc.bits, seen, pocc.bits, slots};
    const size_t fb[4] = {occ_bits_bytes(cocc), (size_t)cells, occ_bits_bytes(pocc), (size_t)row_cap * max_points * sizeof(int)};
    const unsigned char fv[4] = {0, 0, 0, 0x7f};
    ISF_TRY(fill_many(st, 4, fp, fb, fv));
    hipLaunchKernelGGL(hv_mark_bytes_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, points, P, C, g, hb, seen);
    hipLaunchKernelGGL(hv_pack_bytes_kernel, dim3(ceil_div((long long)cocc.nwords, 256)), dim3(256), 0, st, seen,
                       (size_t)cells, cocc.nwords, cocc.bits);
  } else {
    ISF_TRY(occ_create(a, &cocc, 1, g.gz * nb, g.gy, g.gx, st));
    hipLaunchKernelGGL(hv_mark_cells_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, points, P, C, g, hb,
                       cocc.bits);
  }
  ISF_LAUNCH_CHECK();
  ISF_TRY(occ_scan(a, cocc, st));
  int32_t* cell_coors = nullptr;
  ISF_TRY(a.alloc_n(&cell_coors, (size_t)row_cap * 4));
  if (!bytes_path) {
    ISF_HIP_TRY(hipMemsetAsync(slots, 0x7f, (size_t)row_cap * max_points * sizeof(int), st));
    ISF_TRY(occ_create(a, &pocc, 1, 1, 1, P, st));
  }
  ISF_TRY(occ_compact_coords4(cocc, cell_coors, st));
  {
    uint32_t *keys = nullptr, *keys_sorted = nullptr, *start = nullptr;
    int* idx_sorted = nullptr;
    ISF_TRY(a.alloc_n(&keys, (size_t)P));
    ISF_TRY(a.alloc_n(&keys_sorted, (size_t)P));
    ISF_TRY(a.alloc_n(&idx_sorted, (size_t)P));
    ISF_TRY(a.alloc_n(&start, (size_t)row_cap + 1));
    const uint32_t none = (uint32_t)row_cap;           // ranks are < row_cap
    int key_bits = 1;
    while ((1ull << key_bits) <= (unsigned long long)none) ++key_bits;
    hipLaunchKernelGGL(hv_keys_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, points, P, C, g, hb, cocc.bits,
                       cocc.prefix, none, keys, (int*)nullptr);
    ISF_LAUNCH_CHECK();
    ISF_TRY(stable_sort_u32_impl(a, keys, P, key_bits, idx_sorted, st, keys_sorted));
    hipLaunchKernelGGL(hv_segment_heads_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, keys_sorted, P, none, start);
    hipLaunchKernelGGL(hv_segment_slots_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, keys_sorted, idx_sorted, P,
                       start, none, max_points, slots);
  }
  hipLaunchKernelGGL(hv_mark_first_kernel, dim3(ceil_div(row_cap, 256)), dim3(256), 0, st, slots,
                     cocc.total, max_points, pocc.bits);
  ISF_LAUNCH_CHECK();
  ISF_TRY(occ_scan(a, pocc, st));
  hipLaunchKernelGGL(hv_gather_kernel, dim3(ceil_div((long long)row_cap * max_points, 256)), dim3(256),
                     0, st, points, C, slots, cocc.total, cell_coors, max_points, pocc.bits,
                     pocc.prefix, max_voxels, voxels, coors, num_points, voxel_num_dev ? 1 : 0, hb, g.gz, batch ? 1 : 0,
                     pocc.total);
  ISF_LAUNCH_CHECK();
  if (voxel_num_dev) {
    if (batch)
      hipLaunchKernelGGL(hv_publish_counts_kernel, dim3(1), dim3(1), 0, st, pocc.bits, pocc.prefix, pocc.total, hb,
                         max_voxels, voxel_num_dev);
    else
      hipLaunchKernelGGL(hv_publish_count_kernel, dim3(1), dim3(1), 0, st, pocc.total, max_voxels, voxel_num_dev);
    ISF_LAUNCH_CHECK();
    return ISF_OK;
  }
  int total = 0;
  ISF_TRY(read_int(pocc.total, &total, st));
  *voxel_num_host = total < max_voxels ? total : max_voxels;
  return ISF_OK;
}

}  // namespace isf

extern "C" {

int isf_dynamic_voxelize(const float* points, int num_points, int num_features,
                         const float voxel_size_host[3], const float coors_range_host[6],
                         int32_t* coors, isf_stream_t stream) {
  ISF_REQUIRE(num_points >= 0 && num_features >= 3 && voxel_size_host && coors_range_host,
              ISF_ERR_ARG, "dynamic_voxelize: bad arguments");
  ISF_REQUIRE(num_points == 0 || (points && coors), ISF_ERR_ARG, "dynamic_voxelize: null pointer");
  return isf::dynamic_voxelize_impl(points, num_points, num_features, voxel_size_host,
                                    coors_range_host, coors, 3, 0, 0, isf::as_stream(stream));
}

int isf_dynamic_voxelize_batched(const float* points, const int64_t* point_offsets_host,
                                 int batch_size, int num_features, const float voxel_size_host[3],
                                 const float coors_range_host[6], int32_t* coors4,
                                 isf_stream_t stream) {
  ISF_REQUIRE(point_offsets_host && batch_size >= 0 && num_features >= 3, ISF_ERR_ARG,
              "dynamic_voxelize_batched: bad arguments");
  for (int b = 0; b < batch_size; ++b) {
    const int64_t lo = point_offsets_host[b], hi = point_offsets_host[b + 1];
    ISF_REQUIRE(hi >= lo && hi - lo < (1ll << 31), ISF_ERR_ARG, "dynamic_voxelize_batched: bad offsets");
    ISF_TRY(isf::dynamic_voxelize_impl(points + lo * num_features, (int)(hi - lo), num_features,
                                       voxel_size_host, coors_range_host, coors4 + lo * 4, 4, 1, b,
                                       isf::as_stream(stream)));
  }
  return ISF_OK;
}

int isf_hard_voxelize(const float* points, int num_points, int num_features,
                      const float voxel_size_host[3], const float coors_range_host[6],
                      int max_points, int max_voxels, float* voxels, int32_t* coors,
                      int32_t* num_points_per_voxel, int* voxel_num_host, isf_stream_t stream) {
  ISF_REQUIRE(num_points >= 0 && num_features >= 3 && max_points > 0 && max_voxels > 0 &&
                  voxel_num_host && voxel_size_host && coors_range_host,
              ISF_ERR_ARG, "hard_voxelize: bad arguments");
  ISF_REQUIRE(num_points == 0 || (points && voxels && coors && num_points_per_voxel), ISF_ERR_ARG,
              "hard_voxelize: null pointer");
  isf::Arena& a = isf::arena_for_stream(isf::as_stream(stream));
  ISF_TRY(a.reset());
  return isf::hard_voxelize_impl(a, points, num_points, num_features, voxel_size_host,
                                 coors_range_host, max_points, max_voxels, voxels, coors,
                                 num_points_per_voxel, voxel_num_host, isf::as_stream(stream));
}

int isf_hard_voxelize_device(const float* points, int num_points, int num_features,
                             const float voxel_size_host[3], const float coors_range_host[6],
                             int max_points, int max_voxels, float* voxels, int32_t* coors,
                             int32_t* num_points_per_voxel, int32_t* voxel_num_device, isf_stream_t stream) {
  ISF_REQUIRE(num_points >= 0 && num_features >= 3 && max_points > 0 && max_voxels > 0 &&
                  voxel_num_device && voxel_size_host && coors_range_host,
              ISF_ERR_ARG, "hard_voxelize_device: bad arguments");
  ISF_REQUIRE(num_points == 0 || (points && voxels && coors && num_points_per_voxel), ISF_ERR_ARG,
              "hard_voxelize_device: null pointer");
  isf::Arena& a = isf::arena_for_stream(isf::as_stream(stream));
  ISF_TRY(a.reset());
  return isf::hard_voxelize_impl(a, points, num_points, num_features, voxel_size_host,
                                 coors_range_host, max_points, max_voxels, voxels, coors,
                                 num_points_per_voxel, nullptr, isf::as_stream(stream), voxel_num_device);
}

int isf_hard_voxelize_batched_device(const float* points, const int64_t* point_offsets_host, int batch_size,
                                     int num_features, const float voxel_size_host[3], const float coors_range_host[6],
                                     int max_points, int max_voxels, float* voxels, int32_t* coors4,
                                     int32_t* num_points_per_voxel, int32_t* voxel_num_device, isf_stream_t stream) {
  ISF_REQUIRE(point_offsets_host && batch_size >= 1 && batch_size <= isf::kHvMaxBatch && num_features >= 3 &&
                  max_points > 0 && max_voxels > 0 && voxel_num_device && voxel_size_host && coors_range_host,
              ISF_ERR_ARG, "hard_voxelize_batched_device: bad arguments (batch 1..%d)", isf::kHvMaxBatch);
  isf::HvBatch hb;
  hb.n = batch_size;
  ISF_REQUIRE(point_offsets_host[0] == 0, ISF_ERR_ARG, "hard_voxelize_batched_device: offsets start at 0");
  for (int b = 0; b <= isf::kHvMaxBatch; ++b) {
    const int64_t o = point_offsets_host[b < batch_size ? b : batch_size];
    ISF_REQUIRE(o >= 0 && o < (1ll << 31) && (b == 0 || b > batch_size || o >= point_offsets_host[b - 1]), ISF_ERR_ARG,
                "hard_voxelize_batched_device: bad offsets");
    hb.off[b] = (int)o;
  }
  const int P = hb.off[batch_size];
  ISF_REQUIRE(P == 0 || (points && voxels && coors4 && num_points_per_voxel), ISF_ERR_ARG,
              "hard_voxelize_batched_device: null pointer");
  isf::Arena& a = isf::arena_for_stream(isf::as_stream(stream));
  ISF_TRY(a.reset());
  return isf::hard_voxelize_impl(a, points, P, num_features, voxel_size_host, coors_range_host, max_points, max_voxels,
                                 voxels, coors4, num_points_per_voxel, nullptr, isf::as_stream(stream), voxel_num_device,
                                 &hb);
}

}  // extern "C"
