// Ranking metrics ndcg, map and pre on device predictions by counting,
// not sorting.
//
// Specification: metrics.ndcg / map_metric / precision_at (metrics.py).
// None of them needs the sorted list; each needs, per document d of a
// group, at most two counts over the documents e of the same group:
//
//   rank_d = #{e : (score_e desc, e asc) before (score_d, d)}, the position
//            a stable descending argsort gives d
//   hits_d = #{e relevant : rank_e <= rank_d}                    (map only)
//
// and contributes one term if rank_d < min(k, n):
//
//   ndcg  (2^y_d - 1) / log2(rank_d + 2)
//   map   [y_d > 0] * hits_d / (rank_d + 1)
//   pre   [y_d > 0]
//
// Work split: a work item is one slab of one group, kThreads * kPer
// documents that its threads own: thread t keeps the 64-bit keys
//   (DescKey(score) << 32) | (doc << 1 | relevant)
// of documents slab + t, slab + t + kThreads, ... in registers with their
// counters.  The keys of the WHOLE group are streamed through an LDS tile
// of kTile keys; every thread reads every staged key (a broadcast read, no
// bank conflict) and does one 64-bit compare per counter per owned
// document.  Nothing is scattered by rank and nothing is scanned, so LDS
// holds the tile only and does not bound the group size; a group longer
// than a slab is covered by several work items in separate blocks.
//
// Each work item sums its terms in fp64 in a fixed order (owned documents
// in order, wave butterfly, waves in order) into its own slot of the
// partial buffer; the finish kernel adds a group's slots in slab order.
// No atomics, so the result is bit-reproducible.
//
// Tiers: groups of <= 64 documents take one wave each, four per block, no
// block barrier; every other group takes one block per slab.
#include "gbt_kernels.h"
#include "rank_common.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kPre = 2;

struct RankMetricArgs {
  const float* scores;
  const float* labels;
  const long long* group_ptr;
  const int32_t* work;      // wave tier: group; block tier: {group, slab start}
  const int32_t* part_off;  // [G+1] first partial slot of each group
  int n_work;
  int k;
  double* partial;
};

// NaN takes the last key, where a stable descending argsort puts it
__device__ inline unsigned int NanLastKey(float s) {
  if (s != s) return 0xFFFFFFFFu;
  return DescKey(s);
}

template <int kKind>
__device__ inline unsigned long long DocKey(const RankMetricArgs& a,
                                            long long base, int d) {
  unsigned int lo = (unsigned int)d << 1;
  if constexpr (kKind == kMap) lo |= a.labels[base + d] > 0.0f ? 1u : 0u;
  return RankKey(NanLastKey(a.scores[base + d]), lo);
}

// One pass of `len` staged keys over the first kAct owned documents.
template <int kKind, int kAct, int kPer>
__device__ __forceinline__ void CountTile(const unsigned long long* tile,
                                          int len,
                                          const unsigned long long (&key)[kPer],
                                          int (&rank)[kPer],
                                          int (&hits)[kPer]) {
  static_assert(kAct <= kPer, "active documents");
#pragma unroll 4
  for (int j = 0; j < len; ++j) {
    const unsigned long long ke = tile[j];
#pragma unroll
    for (int m = 0; m < kAct; ++m) {
      rank[m] += ke < key[m] ? 1 : 0;
      if constexpr (kKind == kMap) {
        hits[m] += (ke <= key[m] ? 1 : 0) & (int)(ke & 1ull);
      }
    }
  }
}

template <int kKind, int kThreads, int kPer, int kTile, int kGroups>
__global__ __launch_bounds__(kThreads* kGroups) void RankMetricKernel(
    const RankMetricArgs a) {
  constexpr int kWaves = kThreads / kWave;
  constexpr int kSlab = kThreads * kPer;
  static_assert(kThreads % kWave == 0, "whole waves");
  static_assert(kGroups == 1 || (kWaves == 1 && kPer == 1 && kTile == kWave),
                "shared blocks: one wave, one tile, one document per lane");
  static_assert(kPer == 1 || kPer == 2 || kPer == 4 || kPer == 8, "kPer");
  __shared__ unsigned long long tile_all[kGroups][kTile];
  __shared__ double wsum[kWaves];

  const int slot = (int)threadIdx.x / kThreads;
  const int t = (int)threadIdx.x % kThreads;
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  const int w_idx = (int)blockIdx.x * kGroups + slot;
  if (w_idx >= a.n_work) return;  // whole waves, one-wave tier only
  unsigned long long* tile = tile_all[slot];
  int gidx, start = 0;
  if constexpr (kGroups > 1) {
    gidx = a.work[w_idx];
  } else {
    gidx = a.work[2 * w_idx];
    start = a.work[2 * w_idx + 1];
  }
  const long long base = a.group_ptr[gidx];
  const int n = (int)(a.group_ptr[gidx + 1] - base);
  // the host schedules none of these; uniform over the item's threads
  if (n < 1 || start < 0 || start >= n) return;
  if (kGroups > 1 && n > kTile) return;

  // ---- owned documents -----------------------------------------------------
  unsigned long long my_key[kPer];
  int rank[kPer], hits[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int d = start + t + m * kThreads;
    my_key[m] = d < n ? DocKey<kKind>(a, base, d) : ~0ull;
    rank[m] = 0;
    hits[m] = 0;
  }
  const int owned = n - start < kSlab ? n - start : kSlab;
  const int act = (owned + kThreads - 1) / kThreads;  // 1..kPer, uniform

  // ---- stream the group's keys through the tile ------------------------------
  for (int t0 = 0; t0 < n; t0 += kTile) {
    const int len = n - t0 < kTile ? n - t0 : kTile;
    if (t0 > 0) GroupSync<kWaves>();  // the last tile has been read
    for (int j = t; j < len; j += kThreads) {
      tile[j] = DocKey<kKind>(a, base, t0 + j);
    }
    GroupSync<kWaves>();
    if (kPer >= 8 && act > 4) {
      CountTile<kKind, kPer >= 8 ? 8 : kPer>(tile, len, my_key, rank, hits);
    } else if (kPer >= 4 && act > 2) {
      CountTile<kKind, kPer >= 4 ? 4 : kPer>(tile, len, my_key, rank, hits);
    } else if (kPer >= 2 && act > 1) {
      CountTile<kKind, kPer >= 2 ? 2 : kPer>(tile, len, my_key, rank, hits);
    } else {
      CountTile<kKind, 1>(tile, len, my_key, rank, hits);
    }
  }

  // ---- terms, fixed-order sum ------------------------------------------------
  const int kk = a.k < n ? a.k : n;
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int d = start + t + m * kThreads;
    if (d < n && rank[m] < kk) {
      const double y = (double)a.labels[base + d];
      if constexpr (kKind == kNdcg) {
        // a division, not NdcgDiscount's reciprocal: metrics.ndcg divides
        sum += NdcgGain(y, true) / log2((double)(rank[m] + 2));
      } else if constexpr (kKind == kMap) {
        if (y > 0.0) sum += (double)hits[m] / (double)(rank[m] + 1);
      } else {
        if (y > 0.0) sum += 1.0;
      }
    }
  }
  sum = WaveSum(sum);
  const int out = a.part_off[gidx] + start / kSlab;
  if constexpr (kWaves == 1) {
    if (lane == 0) a.partial[out] = sum;
  } else {
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int w = 0; w < kWaves; ++w) s += wsum[w];
      a.partial[out] = s;
    }
  }
}

// One thread per group: slab partials in slab order, then the group's
// normaliser.  scale[g] <= 0 marks a group that takes the default value
// (empty, no relevant document, IDCG == 0); scale == null leaves the sum.
__global__ void RankMetricFinishKernel(const double* partial,
                                       const int32_t* part_off,
                                       const double* scale, double dflt,
                                       double* out, int n_groups) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= n_groups) return;
  double sum = 0.0;
  for (int i = part_off[g]; i < part_off[g + 1]; ++i) sum += partial[i];
  if (scale != nullptr) {
    const double s = scale[g];
    sum = s > 0.0 ? sum * s : dflt;
  }
  out[g] = sum;
}

template <int kKind, int kThreads, int kPer, int kTile, int kGroups>
void Launch(const RankMetricArgs& a, hipStream_t stream) {
  const int blocks = (a.n_work + kGroups - 1) / kGroups;
  hipLaunchKernelGGL(
      (RankMetricKernel<kKind, kThreads, kPer, kTile, kGroups>), dim3(blocks),
      dim3(kThreads * kGroups), 0, stream, a);
}

template <int kKind>
void LaunchTier(int tier, const RankMetricArgs& a, hipStream_t stream) {
  switch (tier) {
    case 0: Launch<kKind, 64, 1, 64, 4>(a, stream); break;
    case 1: Launch<kKind, 256, 8, 1024, 1>(a, stream); break;
    case 2: Launch<kKind, 256, 4, 1024, 1>(a, stream); break;
    case 3: Launch<kKind, 512, 4, 1024, 1>(a, stream); break;
    case 4: Launch<kKind, 256, 8, 256, 1>(a, stream); break;
    default: break;
  }
}

}  // namespace

extern "C" {

int gbt_rank_metric_slab(int tier) {
  switch (tier) {
    case 0: return 64;
    case 1:
    case 3:
    case 4: return 2048;
    case 2: return 1024;
    default: return 0;
  }
}

void gbt_rank_metric(int kind, int tier, const float* scores,
                     const float* labels, const long long* group_ptr,
                     const int32_t* work, int n_work, int k,
                     const int32_t* part_off, double* partial,
                     hipStream_t stream) {
  if (n_work <= 0) return;
  const RankMetricArgs a{scores, labels, group_ptr, work, part_off, n_work,
                         k, partial};
  switch (kind) {
    case kNdcg: LaunchTier<kNdcg>(tier, a, stream); break;
    case kMap: LaunchTier<kMap>(tier, a, stream); break;
    case kPre: LaunchTier<kPre>(tier, a, stream); break;
    default: break;
  }
}

void gbt_rank_metric_finish(const double* partial, const int32_t* part_off,
                            const double* scale, double dflt, double* out,
                            int n_groups, hipStream_t stream) {
  if (n_groups <= 0) return;
  hipLaunchKernelGGL(RankMetricFinishKernel, dim3((n_groups + 255) / 256),
                     dim3(256), 0, stream, partial, part_off, scale, dflt,
                     out, n_groups);
}

}  // extern "C"
