// isf_attention_plan.h -- which kernels a call of the attention cores runs on, and the workspace it takes: pure host
// arithmetic (no HIP call, no device state), shared by isf_attention.hip / isf_attention_bwd.hip and answered on the CPU
// by tests/test_attention_dropout_keys.py, so that a change of a shape's route shows up as a changed table row.
#pragma once
#include <algorithm>
#include <cstddef>

namespace isf {

static constexpr int kAttnKeysPerSplit = 512;   // keys of one workgroup's resident set (forward) / of one key split (backward)
static constexpr int kAttTile = 128;            // keys (rows_lanes, rows_keysplit) / queries (cols_lanes) per LDS tile
static constexpr int kAttnPartFloats = 2;       // (max, sum) in front of a partial row of head_dim floats

// the index fields of the dropout hash (attn_keep, isf_common.h): bh << 48 | query << 24 | key
static constexpr long long kAttnDropMaxIndex = 1ll << 24;   // queries and keys below this
static constexpr long long kAttnDropMaxBh = 1ll << 16;      // batch_size * num_heads below this

// the argument whose indices would alias in the hash (its name, *value and *limit set), or nullptr when all fit
inline const char* attention_dropout_out_of_range(int batch, int num_queries, int num_keys, int heads, long long* value,
                                                  long long* limit) {
  *limit = kAttnDropMaxIndex;
  if ((*value = num_queries) >= kAttnDropMaxIndex) return "num_queries";
  if ((*value = num_keys) >= kAttnDropMaxIndex) return "num_keys";
  *limit = kAttnDropMaxBh;
  if ((*value = (long long)batch * heads) >= kAttnDropMaxBh) return "batch_size * num_heads";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------------------ forward
// up to 512 keys: one resident set; more (the head's 32400): 512-key splits, each writing (max, sum, unnormalised O) per
// query [B][heads][nsplit][Lq][head_dim + 2], merged by merge_key_splits_kernel
struct AttnForwardPlan {
  int keys_per_split;
  int splits;
  size_t workspace_floats;
};

inline AttnForwardPlan attention_forward_plan(int batch, int num_queries, int num_keys, int heads, int head_dim) {
  AttnForwardPlan p;
  p.keys_per_split = num_keys > kAttnKeysPerSplit ? kAttnKeysPerSplit : num_keys;
  p.splits = (num_keys + p.keys_per_split - 1) / p.keys_per_split;
  p.workspace_floats = p.splits == 1 ? 0 : (size_t)batch * heads * p.splits * num_queries * (head_dim + kAttnPartFloats);
  return p;
}

// ----------------------------------------------------------------------------------------------------------- backward
enum AttnBwdRoute {
  kAttnBwdWave = 0,       // attention_bwd_rows_kernel + attention_bwd_cols_kernel: a wave per query / per key
  kAttnBwdLanes = 1,      // attention_bwd_rows_lanes_kernel + attention_bwd_cols_lanes_kernel: a lane per query / per key
  kAttnBwdKeySplit = 2,   // attention_bwd_rows_keysplit_kernel + merge, then attention_bwd_cols_lanes_kernel (one chunk)
};

struct AttnBackwardPlan {
  int route;
  int chunks;        // query chunks of the dK / dV kernel (> 1: partial buffers + the ordered reduce)
  int key_splits;    // key splits of the dQ kernel (kAttnBwdKeySplit only, else 1)
  size_t workspace_floats;
};

// head_dim 16.  ldgkv: the leading dimension of grad_k / grad_v (the partial buffers of chunks > 1 copy it); 0 = packed.
inline AttnBackwardPlan attention_backward_plan(int batch, int num_queries, int num_keys, int heads, bool dropout_on,
                                                int ldgkv = 0) {
  const int hd = 16;
  if (ldgkv == 0) ldgkv = hd * heads;
  AttnBackwardPlan p;
  p.key_splits = 1;
  p.workspace_floats = (size_t)batch * heads * num_queries * 2;   // stat (L, D) per (sample, head, query)
  const size_t rows = (size_t)batch * num_keys;
  // many keys under few queries with dropout (the head's 200 x 32400 cross-attention in training): a wave per query would
  // walk every key twice with per-lane row fetches and a hash per pair; cut the keys instead
  if (dropout_on && num_keys > kAttnKeysPerSplit && num_queries <= 256) {
    p.route = kAttnBwdKeySplit;
    p.chunks = 1;
    p.key_splits = (num_keys + kAttnKeysPerSplit - 1) / kAttnKeysPerSplit;
    p.workspace_floats += (size_t)batch * heads * p.key_splits * num_queries * (hd + kAttnPartFloats);
    return p;
  }
  if (num_queries >= 2048) {   // lanes own queries / keys (see attention_bwd_rows_lanes_kernel)
    p.route = kAttnBwdLanes;
    // enough (key block, chunk, head, sample) workgroups to fill the chip: ~2000 of them, at least 2 query tiles each
    const int kblocks = (num_keys + 255) / 256;
    int chunks = std::max(1, 2048 / std::max(1, kblocks * heads * batch));
    p.chunks = std::max(1, std::min(chunks, num_queries / (2 * kAttTile)));
    p.workspace_floats += 2 * (size_t)p.chunks * rows * ldgkv;   // always through the partial buffers
    return p;
  }
  p.route = kAttnBwdWave;
  p.chunks = std::max(1, std::min(64, num_queries / 1024));
  if (p.chunks > 1) p.workspace_floats += 2 * (size_t)p.chunks * rows * ldgkv;
  return p;
}

}  // namespace isf
