// Row partition for CDNA4: scatter each node segment's rows into
// [left | right] halves of a double buffer.
//
// Reference behavior: src/tree/gpu_hist/row_partitioner.cuh (cub
// DispatchScan partition + SortPositionCopyKernel).  MI355X re-design:
// wave-tiled, ballot-based block-aggregated scatter —
//   A) each wave walks tiles of 64 CONSECUTIVE ridx_in entries (one
//      coalesced load per tile), gathers the bin and takes the wave
//      ballot of the go-left decision; left counts are popcounts,
//   B) ONE atomicAdd/atomicSub PER BLOCK reserves the global left/right
//      windows (profiling showed per-wave atomics on the per-node
//      counters serialize: 273us/launch -> ~10us),
//   C) a lane's destination is window base + mbcnt(ballot), so each
//      side's stores are contiguous within the wave.
// Row ids and ballots stay in registers between A and C for tasks of up
// to kPartCacheRows rows; larger tasks re-load and re-gather in C.
// Order within a side is unspecified; histogram sums are
// order-independent anyway (int64 fixed point).
#include "gbt_kernels.h"

#ifndef GBT_PART_BLOCK
#define GBT_PART_BLOCK 256
#endif

namespace {
constexpr int kPartWaves = GBT_PART_BLOCK / 64;
// register-cached tiles per wave: 4 covers the 1024-row tasks, 16 the
// coarser task sizes (4096 rows per block)
constexpr int kPartTilesSmall = 4;
constexpr int kPartTilesLarge = 16;
constexpr int kPartCacheRows = kPartTilesLarge * 64 * kPartWaves;
}  // namespace

__device__ __forceinline__ bool DecideLeft(int local_bin, int fbins,
                                           int split_bin_local,
                                           bool default_left,
                                           const uint32_t* cat_bits,
                                           int cat_words) {
  if (local_bin >= fbins) {  // missing
    return default_left;
  }
  if (cat_words > 0) {       // categorical: stored set goes RIGHT
    const int w = local_bin >> 5;
    const bool in_set =
        (w < cat_words) && ((cat_bits[w] >> (local_bin & 31)) & 1u);
    return !in_set;
  }
  return local_bin <= split_bin_local;
}

// per-block split description, shared by the count and scatter phases
template <typename BinT>
struct PartSplit {
  const BinT* gidx;
  const BinT* col;  // the split feature's column, or null (row-major)
  int n_features, feature, fbins, sbin, cat_words;
  bool dleft;
  const uint32_t* cats;

  __device__ __forceinline__ bool Left(int row) const {
    const int local = col ? (int)col[row]
                          : (int)gidx[(size_t)row * n_features + feature];
    return DecideLeft(local, fbins, sbin, dleft, cats, cat_words);
  }
};

// number of set bits of a wave mask below this lane
__device__ __forceinline__ int LanesBelow(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi(
      (unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// phase B: one reservation per block on the node's counter pair;
// returns this wave's first left / right destination
__device__ __forceinline__ void ReserveWindows(int wave_left, int wave_right,
                                               int32_t* counters, int slot,
                                               int* dl, int* dr) {
  __shared__ int s_left[kPartWaves], s_right[kPartWaves];
  __shared__ int s_base_l, s_base_r;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_left[wave] = wave_left;
    s_right[wave] = wave_right;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot_l = 0, tot_r = 0;
    for (int w = 0; w < kPartWaves; ++w) {
      tot_l += s_left[w];
      tot_r += s_right[w];
    }
    s_base_l = tot_l ? atomicAdd(&counters[2 * slot], tot_l) : 0;
    s_base_r = tot_r ? atomicSub(&counters[2 * slot + 1], tot_r) - tot_r : 0;
  }
  __syncthreads();
  int l = s_base_l, r = s_base_r;
  for (int w = 0; w < wave; ++w) {
    l += s_left[w];
    r += s_right[w];
  }
  *dl = l;
  *dr = r;
}

// Tasks of up to TILES * 64 * kPartWaves rows: tile j of wave w covers
// entries [begin + (j * kPartWaves + w) * 64, +64).  Straight-line code
// (no per-tile branch) so the TILES loads and gathers issue back to back.
template <typename BinT, int TILES>
__device__ __forceinline__ void PartitionCached(
    const PartSplit<BinT>& sp, const int32_t* __restrict__ ridx_in,
    int32_t* __restrict__ ridx_out, int begin, int end, int slot,
    int32_t* counters) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  int rows[TILES];
  unsigned long long lmask[TILES];
  int wave_left = 0, wave_rows = 0;
#pragma unroll
  for (int j = 0; j < TILES; ++j) {
    const int i = begin + (j * kPartWaves + wave) * 64 + lane;
    const bool valid = i < end;
    // clamped: lanes past the task re-read its last entry (in bounds)
    rows[j] = ridx_in[min(i, end - 1)];
    lmask[j] = __ballot(sp.Left(rows[j]) && valid);
    wave_left += __popcll(lmask[j]);
    wave_rows += __popcll(__ballot(valid));
  }
  int dl, dr;
  ReserveWindows(wave_left, wave_rows - wave_left, counters, slot, &dl, &dr);
#pragma unroll
  for (int j = 0; j < TILES; ++j) {
    const int i = begin + (j * kPartWaves + wave) * 64 + lane;
    const bool valid = i < end;
    const unsigned long long lm = lmask[j];
    const unsigned long long rm = __ballot(valid) & ~lm;
    if (valid) {
      if ((lm >> lane) & 1ull) {
        ridx_out[dl + LanesBelow(lm)] = rows[j];
      } else {
        ridx_out[dr + LanesBelow(rm)] = rows[j];
      }
    }
    dl += __popcll(lm);
    dr += __popcll(rm);
  }
}

// Tasks beyond the register budget: count, then re-load and re-gather.
template <typename BinT>
__device__ __forceinline__ void PartitionRegather(
    const PartSplit<BinT>& sp, const int32_t* __restrict__ ridx_in,
    int32_t* __restrict__ ridx_out, int begin, int end, int slot,
    int32_t* counters) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  int wave_left = 0, wave_rows = 0;
  for (int t0 = begin + wave * 64; t0 < end; t0 += kPartWaves * 64) {
    const int i = t0 + lane;
    const bool valid = i < end;
    const int row = ridx_in[min(i, end - 1)];
    wave_left += __popcll(__ballot(sp.Left(row) && valid));
    wave_rows += __popcll(__ballot(valid));
  }
  int dl, dr;
  ReserveWindows(wave_left, wave_rows - wave_left, counters, slot, &dl, &dr);
  for (int t0 = begin + wave * 64; t0 < end; t0 += kPartWaves * 64) {
    const int i = t0 + lane;
    const bool valid = i < end;
    const int row = ridx_in[min(i, end - 1)];
    const bool left = sp.Left(row) && valid;
    const unsigned long long lm = __ballot(left);
    const unsigned long long rm = __ballot(valid) & ~lm;
    if (valid) {
      if (left) {
        ridx_out[dl + LanesBelow(lm)] = row;
      } else {
        ridx_out[dr + LanesBelow(rm)] = row;
      }
    }
    dl += __popcll(lm);
    dr += __popcll(rm);
  }
}

// gidx_col: optional FEATURE-MAJOR copy of the bin matrix ([F][ld]).
// The partition touches ONE feature per node, so the column layout
// turns its per-row gather from a random 64-byte line across the whole
// row-major matrix (LLC-bandwidth bound, ~4x the roofline) into
// accesses confined to a single n_rows-byte column that sits in cache.
template <typename BinT>
__global__ __launch_bounds__(GBT_PART_BLOCK) void PartitionKernel(
    const BinT* __restrict__ gidx, int n_features,
    const BinT* __restrict__ gidx_col, long long col_ld,
    const int32_t* __restrict__ ridx_in, int32_t* __restrict__ ridx_out,
    const BlockTask* __restrict__ tasks,
    const int32_t* __restrict__ split_feature,
    const int32_t* __restrict__ split_bin_local,
    const uint8_t* __restrict__ default_left,
    const uint32_t* __restrict__ cat_bits,
    const int32_t* __restrict__ cat_bits_offset,
    const int32_t* __restrict__ n_bins_feat,
    int32_t* __restrict__ counters) {
  const BlockTask task = tasks[blockIdx.x];
  if (task.row_begin >= task.row_end) return;  // padded empty task
  const int slot = task.out_slot;
  PartSplit<BinT> sp;
  sp.gidx = gidx;
  sp.n_features = n_features;
  sp.feature = split_feature[slot];
  sp.sbin = split_bin_local[slot];
  sp.dleft = default_left[slot] != 0;
  sp.fbins = n_bins_feat[sp.feature];
  sp.cats = nullptr;
  sp.cat_words = 0;
  if (cat_bits_offset != nullptr) {
    const int c0 = cat_bits_offset[slot];
    sp.cat_words = cat_bits_offset[slot + 1] - c0;
    if (sp.cat_words > 0) sp.cats = cat_bits + c0;
  }
  sp.col = gidx_col ? gidx_col + (size_t)sp.feature * col_ld : nullptr;

  // block-uniform dispatch on the task size
  const int n_rows = task.row_end - task.row_begin;
  if (n_rows <= kPartTilesSmall * 64 * kPartWaves) {
    PartitionCached<BinT, kPartTilesSmall>(sp, ridx_in, ridx_out,
                                           task.row_begin, task.row_end, slot,
                                           counters);
  } else if (n_rows <= kPartCacheRows) {
    PartitionCached<BinT, kPartTilesLarge>(sp, ridx_in, ridx_out,
                                           task.row_begin, task.row_end, slot,
                                           counters);
  } else {
    PartitionRegather<BinT>(sp, ridx_in, ridx_out, task.row_begin,
                            task.row_end, slot, counters);
  }
}

extern "C" void gbt_partition(
    const uint8_t* gidx8, const uint16_t* gidx16, int n_features,
    const uint8_t* gidx8_col, const uint16_t* gidx16_col, int64_t col_ld,
    const int32_t* ridx_in, int32_t* ridx_out, const BlockTask* tasks,
    int n_tasks, const int32_t* split_feature, const int32_t* split_bin_local,
    const uint8_t* default_left, const uint32_t* cat_bits,
    const int32_t* cat_bits_offset, const int32_t* n_bins_feat,
    int32_t* counters, hipStream_t stream) {
  if (gidx8 != nullptr) {
    hipLaunchKernelGGL((PartitionKernel<uint8_t>), dim3(n_tasks),
                       dim3(GBT_PART_BLOCK), 0, stream, gidx8, n_features,
                       gidx8_col, (long long)col_ld,
                       ridx_in, ridx_out, tasks, split_feature,
                       split_bin_local, default_left, cat_bits,
                       cat_bits_offset, n_bins_feat, counters);
  } else {
    hipLaunchKernelGGL((PartitionKernel<uint16_t>), dim3(n_tasks),
                       dim3(GBT_PART_BLOCK), 0, stream, gidx16, n_features,
                       gidx16_col, (long long)col_ld,
                       ridx_in, ridx_out, tasks, split_feature,
                       split_bin_local, default_left, cat_bits,
                       cat_bits_offset, n_bins_feat, counters);
  }
}

// Copy partitioned task ranges from the scratch buffer back into the
// primary ridx buffer — one launch replaces per-segment memcpys.
__global__ __launch_bounds__(GBT_PART_BLOCK) void CopyRangesKernel(
    const int32_t* __restrict__ src, int32_t* __restrict__ dst,
    const BlockTask* __restrict__ tasks) {
  const BlockTask task = tasks[blockIdx.x];
  for (int i = task.row_begin + (int)threadIdx.x; i < task.row_end;
       i += blockDim.x) {
    dst[i] = src[i];
  }
}

extern "C" void gbt_copy_ranges(const int32_t* src, int32_t* dst,
                                const BlockTask* tasks, int n_tasks,
                                hipStream_t stream) {
  hipLaunchKernelGGL(CopyRangesKernel, dim3(n_tasks), dim3(GBT_PART_BLOCK), 0,
                     stream, src, dst, tasks);
}

__global__ __launch_bounds__(GBT_PART_BLOCK) void LeafPartitionKernel(
    const int32_t* __restrict__ ridx, const BlockTask* __restrict__ tasks,
    const int32_t* __restrict__ leaf_ids, int32_t* __restrict__ out_pos) {
  const BlockTask task = tasks[blockIdx.x];
  const int leaf = leaf_ids[task.out_slot];
  for (int i = task.row_begin + (int)threadIdx.x; i < task.row_end;
       i += blockDim.x) {
    out_pos[ridx[i]] = leaf;
  }
}

template <typename BinT>
__global__ __launch_bounds__(GBT_PART_BLOCK) void LeafDecideKernel(
    const BinT* __restrict__ gidx, int n_features,
    const BinT* __restrict__ gidx_col, long long col_ld,
    const int32_t* __restrict__ ridx, const BlockTask* __restrict__ tasks,
    const int32_t* __restrict__ split_feature,
    const int32_t* __restrict__ split_bin_local,
    const uint8_t* __restrict__ default_left,
    const int32_t* __restrict__ kids /* [k][2] = (left nid, right nid) */,
    const int32_t* __restrict__ n_bins_feat, int32_t* __restrict__ out_pos) {
  const BlockTask task = tasks[blockIdx.x];
  if (task.row_begin >= task.row_end) return;
  const int slot = task.out_slot;
  const int feature = split_feature[slot];
  const int sbin = split_bin_local[slot];
  const bool dleft = default_left[slot] != 0;
  const int fbins = n_bins_feat[feature];
  const int lnid = kids[2 * slot], rnid = kids[2 * slot + 1];
  const BinT* col = gidx_col ? gidx_col + (size_t)feature * col_ld
                             : nullptr;
  for (int i = task.row_begin + (int)threadIdx.x; i < task.row_end;
       i += blockDim.x) {
    const int row = ridx[i];
    const int local = col ? (int)col[row]
                          : (int)gidx[(size_t)row * n_features + feature];
    const bool left = DecideLeft(local, fbins, sbin, dleft, nullptr, 0);
    out_pos[row] = left ? lnid : rnid;
  }
}

extern "C" void gbt_leaf_decide(const uint8_t* gidx8, const uint16_t* gidx16,
                                int n_features,
                                const uint8_t* gidx8_col,
                                const uint16_t* gidx16_col, int64_t col_ld,
                                const int32_t* ridx,
                                const BlockTask* tasks, int n_tasks,
                                const int32_t* split_feature,
                                const int32_t* split_bin_local,
                                const uint8_t* default_left,
                                const int32_t* kids,
                                const int32_t* n_bins_feat, int32_t* out_pos,
                                hipStream_t stream) {
  if (gidx8 != nullptr) {
    hipLaunchKernelGGL((LeafDecideKernel<uint8_t>), dim3(n_tasks),
                       dim3(GBT_PART_BLOCK), 0, stream, gidx8, n_features,
                       gidx8_col, (long long)col_ld,
                       ridx, tasks, split_feature, split_bin_local,
                       default_left, kids, n_bins_feat, out_pos);
  } else {
    hipLaunchKernelGGL((LeafDecideKernel<uint16_t>), dim3(n_tasks),
                       dim3(GBT_PART_BLOCK), 0, stream, gidx16, n_features,
                       gidx16_col, (long long)col_ld,
                       ridx, tasks, split_feature, split_bin_local,
                       default_left, kids, n_bins_feat, out_pos);
  }
}

extern "C" void gbt_leaf_partition(const int32_t* ridx, const BlockTask* tasks,
                                   int n_tasks, const int32_t* leaf_ids,
                                   int32_t* out_pos, hipStream_t stream) {
  hipLaunchKernelGGL(LeafPartitionKernel, dim3(n_tasks),
                     dim3(GBT_PART_BLOCK), 0, stream, ridx, tasks, leaf_ids,
                     out_pos);
}
