// LambdaMART gradients for query groups too long for lambdarank.hip's LDS
// tiers (above 2048 documents): the slab tier.
//
// Specification: the same as lambdarank.hip, _LambdaRankBase.get_gradient
// (objectives.py), top-k pair method, through the same definitions
// (rank_common.h): rank key, statistics' terms, pair gradient, group
// normaliser and final write.
//
// A work item is one slab of one group: kThreads * kPer consecutive
// positions (documents in launch 1, ranks afterwards) that the threads of
// one block own, thread t taking start + t, start + t + kThreads, ...  The
// ranked list lives in global scratch, so LDS does not bound the group.
// At most four launches, all over the same item list:
//
//  1. rank     every thread keeps its documents' 64-bit keys
//              (DescKey(score) << 32) | doc in registers and counts the
//              smaller keys of the WHOLE group, streamed through an LDS
//              tile.  The tile holds the 32-bit score keys only: the low
//              half of a staged key is its position in the group, which is
//              uniform over the wave, so the compare takes it from a
//              scalar register and the tile is half the size and half the
//              LDS traffic of rank_metric.hip's.  Unique keys make the
//              ranks a permutation; each document scatters score, label
//              and in-group index (int32) to its rank slot.
//  2. stats    rank:map only.  The first item of a group scans the by-rank
//              labels in fp64 into n_rel and acc = cumsum(y / (r + 1)):
//              tiles of 1024 ranks, thread-contiguous, wave scan, waves in
//              order, a running carry between tiles.  ndcg needs no table
//              (discount from the rank, gain from the label) and pairwise
//              none at all.
//  3. pairs    one block per (group, column slab).  A thread keeps its
//              columns' score, label, two statistics and g/h sums in
//              registers; the head rows i < min(k, n) pass through LDS
//              kRowChunk at a time (score, label, two fp64 statistics: 24
//              bytes a row), so k is not bounded.  Pair (i, j), j > i, is
//              evaluated once: the column share stays in the register, the
//              row share is summed over the wave by a butterfly, over the
//              block's waves in order, and written to row_part[item][i].
//              An item only visits rows above its last column, so with
//              the default k = 32 every item does one chunk; its share of
//              sum(-2 lambda) goes to s_part[item].
//  4. finish   one block per slab: s_part of the group in slab order and
//              the normaliser; for each owned rank the column sum, plus
//              for a head rank the row shares of the items that have a
//              column above it, in slab order; StoreGpair through the
//              rank -> document map.
//
// No atomics and every sum in a fixed order: the output is
// bit-reproducible.  Every scratch entry that is read has been written by
// an earlier launch of the same call, so the scratch is never cleared.
//
// Shapes: 256 threads with kPer = 1, 2, 4 or 8 positions each.  kPer = 1,
// a slab of 256, is the measured choice up to the tier's cap of 2^16
// documents: the most blocks for a lone long group and the fewest
// registers in the pair kernel (profiles/lambdarank_mi355x.md).
#include "gbt_kernels.h"
#include "rank_common.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kRowChunk = 64;  // head rows in LDS at a time
constexpr int kTile = 2048;    // score keys per LDS tile of the rank pass
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPairwise = 2;

struct SlabArgs {
  const float* scores;
  const float* labels;
  const long long* group_ptr;
  const double* inv_idcg;     // [G], ndcg only
  const double* weight;       // [N] or null
  const int32_t* items;       // [n_items] {group, slab start}
  const int32_t* item_off;    // [G+1] first item slot of each group
  const long long* doc_off;   // [G+1] first by-rank slot of each group
  const long long* row_off;   // [G+1] first row_part entry of each group
  int n_items;
  int k;
  int score_norm;
  int normalize;
  int exp_gain;
  // scratch, by rank: [n_docs] each
  float* r_score;
  float* r_label;
  int32_t* r_doc;
  double* st0;    // map: n_rel
  double* st1;    // map: acc
  double* col_g;
  double* col_h;
  double* row_g;  // [n_rows] row_part
  double* row_h;
  double* s_part;  // [n_items]
  float* out_g;
  float* out_h;
};

struct Item {
  int gidx, start, n;
  long long base;
  bool ok;
};

// The host schedules no item outside its group; uniform over the block.
__device__ inline Item LoadItem(const SlabArgs& a) {
  Item it;
  it.gidx = a.items[2 * (int)blockIdx.x];
  it.start = a.items[2 * (int)blockIdx.x + 1];
  it.base = a.group_ptr[it.gidx];
  it.n = (int)(a.group_ptr[it.gidx + 1] - it.base);
  it.ok = it.n >= 1 && it.start >= 0 && it.start < it.n;
  return it;
}

// ---- 1. rank and scatter ----------------------------------------------------

// One pass of `len` staged score keys, group positions t0.., over the
// first kAct owned documents.
template <int kAct, int kPer>
__device__ __forceinline__ void CountTile(const unsigned int* tile, int t0,
                                          int len,
                                          const unsigned long long (&key)[kPer],
                                          int (&rank)[kPer]) {
  static_assert(kAct <= kPer, "active documents");
#pragma unroll 4
  for (int j = 0; j < len; ++j) {
    const unsigned long long ke = RankKey(tile[j], t0 + j);
#pragma unroll
    for (int m = 0; m < kAct; ++m) rank[m] += ke < key[m] ? 1 : 0;
  }
}

template <int kPer>
__global__ __launch_bounds__(kThreads) void SlabRankKernel(const SlabArgs a) {
  constexpr int kSlab = kThreads * kPer;
  static_assert(kPer == 1 || kPer == 2 || kPer == 4 || kPer == 8, "kPer");
  __shared__ unsigned int tile[kTile];
  const Item it = LoadItem(a);
  if (!it.ok) return;
  const int t = (int)threadIdx.x;
  const int n = it.n;

  float my_s[kPer];
  unsigned long long my_key[kPer];
  int rank[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int d = it.start + t + m * kThreads;
    my_s[m] = 0.0f;
    my_key[m] = 0;  // nothing is below it: the counter of an empty slot rests
    rank[m] = 0;
    if (d < n) {
      my_s[m] = a.scores[it.base + d] + 0.0f;
      my_key[m] = RankKey(DescKey(my_s[m]), d);
    }
  }
  const int owned = n - it.start < kSlab ? n - it.start : kSlab;
  const int act = (owned + kThreads - 1) / kThreads;  // 1..kPer, uniform

  for (int t0 = 0; t0 < n; t0 += kTile) {
    const int len = n - t0 < kTile ? n - t0 : kTile;
    if (t0 > 0) __syncthreads();  // the last tile has been read
    for (int j = t; j < len; j += kThreads) {
      tile[j] = DescKey(a.scores[it.base + t0 + j]);
    }
    __syncthreads();
    if (kPer >= 8 && act > 4) {
      CountTile<kPer >= 8 ? 8 : kPer>(tile, t0, len, my_key, rank);
    } else if (kPer >= 4 && act > 2) {
      CountTile<kPer >= 4 ? 4 : kPer>(tile, t0, len, my_key, rank);
    } else if (kPer >= 2 && act > 1) {
      CountTile<kPer >= 2 ? 2 : kPer>(tile, t0, len, my_key, rank);
    } else {
      CountTile<1>(tile, t0, len, my_key, rank);
    }
  }

  const long long off = a.doc_off[it.gidx];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int d = it.start + t + m * kThreads;
    if (d < n && rank[m] < n) {  // rank < n always; keeps a bad key in bounds
      a.r_score[off + rank[m]] = my_s[m];
      a.r_label[off + rank[m]] = a.labels[it.base + d];
      a.r_doc[off + rank[m]] = d;
    }
  }
}

// ---- 2. rank:map statistics -------------------------------------------------

__global__ __launch_bounds__(kThreads) void SlabMapScanKernel(const SlabArgs a) {
  constexpr int kPer = 4;
  constexpr int kSpan = kThreads * kPer;
  __shared__ double scan_c[kWaves], scan_a[kWaves];
  const Item it = LoadItem(a);
  if (!it.ok || it.start != 0) return;  // the group's first item scans it
  const int t = (int)threadIdx.x;
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  const int n = it.n;
  const long long off = a.doc_off[it.gidx];
  const float* ry = a.r_label + off;
  double carry_c = 0.0, carry_a = 0.0;
  for (int t0 = 0; t0 < n; t0 += kSpan) {
    // thread t scans the contiguous ranks [lo, lo + kPer)
    const int lo = t0 + t * kPer;
    double y[kPer];
    double c = 0.0, ac = 0.0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = lo + q;
      y[q] = e < n ? (double)ry[e] : 0.0;
      c += y[q];
      ac += y[q] / (double)(e + 1);
    }
    double run_c, run_a;
    MapWaveScan(lane, c, ac, run_c, run_a);
    if (t0 > 0) __syncthreads();  // the last span's totals have been read
    if (lane == kWave - 1) {
      scan_c[wave] = c;
      scan_a[wave] = ac;
    }
    __syncthreads();
    double pc = carry_c, pa = carry_a;
    for (int w = 0; w < wave; ++w) {
      pc += scan_c[w];
      pa += scan_a[w];
    }
    run_c += pc;
    run_a += pa;
    // the same order in every thread, so the carry is uniform
    for (int w = 0; w < kWaves; ++w) {
      carry_c += scan_c[w];
      carry_a += scan_a[w];
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = lo + q;
      if (e < n) {
        run_c += y[q];
        run_a += y[q] / (double)(e + 1);
        a.st0[off + e] = run_c;
        a.st1[off + e] = run_a;
      }
    }
  }
}

// ---- 3. pairs ---------------------------------------------------------------

template <int kMetric, int kPer>
__global__ __launch_bounds__(kThreads) void SlabPairsKernel(const SlabArgs a) {
  constexpr int kSlab = kThreads * kPer;
  __shared__ float row_s[kRowChunk], row_y[kRowChunk];
  __shared__ double row_a[kRowChunk], row_b[kRowChunk];
  __shared__ double part_g[kRowChunk * kWaves], part_h[kRowChunk * kWaves];
  __shared__ double wsum[kWaves];
  const Item it = LoadItem(a);
  if (!it.ok) return;
  const int t = (int)threadIdx.x;
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  const int n = it.n;
  const long long off = a.doc_off[it.gidx];
  const float* rs = a.r_score + off;
  const float* ry = a.r_label + off;
  const double* st0 = a.st0 + off;
  const double* st1 = a.st1 + off;
  const int end = it.start + kSlab < n ? it.start + kSlab : n;
  const int kk = a.k < n ? a.k : n;
  // rows with a column of this slab above them
  const int rlim = kk < end - 1 ? kk : end - 1;

  double inv_idcg = 0.0, n_total = 1.0;
  if constexpr (kMetric == kNdcg) inv_idcg = a.inv_idcg[it.gidx];
  if constexpr (kMetric == kMap) n_total = fmax(st0[n - 1], 1e-300);
  // LambdaGrad's degenerate-group check: no score normalisation when the
  // best score equals the worst (every group at round 0)
  const bool do_norm = a.score_norm && rs[0] != rs[n - 1];

  // columns: ndcg {discount, gain}, map {n_rel / rank, acc of the rank above}
  float col_y[kPer];
  double col_s[kPer], col_a[kPer], col_b[kPer], acc_g[kPer], acc_h[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int j = it.start + t + m * kThreads;
    col_y[m] = 0.0f;
    col_s[m] = col_a[m] = col_b[m] = acc_g[m] = acc_h[m] = 0.0;
    if (j < n) {
      col_y[m] = ry[j];
      col_s[m] = (double)rs[j];
      if constexpr (kMetric == kNdcg) {
        col_a[m] = NdcgDiscount(j);
        col_b[m] = NdcgGain((double)col_y[m], a.exp_gain);
      } else if constexpr (kMetric == kMap) {
        col_a[m] = st0[j] / (double)(j + 1);
        col_b[m] = j > 0 ? st1[j - 1] : 0.0;
      }
    }
  }

  const long long rbase =
      a.row_off[it.gidx] + (long long)(it.start / kSlab) * kk;
  double s_loc = 0.0;  // this thread's share of sum(-2 lambda)
  for (int c0 = 0; c0 < rlim; c0 += kRowChunk) {
    const int c1 = c0 + kRowChunk < rlim ? c0 + kRowChunk : rlim;
    if (t < c1 - c0) {
      const int i = c0 + t;
      const float y = ry[i];
      row_s[t] = rs[i];
      row_y[t] = y;
      if constexpr (kMetric == kNdcg) {
        row_a[t] = NdcgDiscount(i);
        row_b[t] = NdcgGain((double)y, a.exp_gain);
      } else if constexpr (kMetric == kMap) {
        row_a[t] = st0[i] / (double)(i + 1);
        row_b[t] = st1[i];
      }
    }
    __syncthreads();
    for (int i = c0; i < c1; ++i) {
      const float yi = row_y[i - c0];
      const double si = (double)row_s[i - c0];
      double a_i = 0.0, b_i = 0.0;
      if constexpr (kMetric != kPairwise) {
        a_i = row_a[i - c0];
        b_i = row_b[i - c0];
      }
      double pg = 0.0, ph = 0.0;
#pragma unroll
      for (int m = 0; m < kPer; ++m) {
        const int j = it.start + t + m * kThreads;
        if (j > i && j < n && col_y[m] != yi) {
          const auto col = [&](double& a_j, double& b_j) {
            a_j = col_a[m];
            b_j = col_b[m];
          };
          const PairTerms p = PairGrad<kMetric>(yi, si, a_i, b_i, col_y[m],
                                                col_s[m], col, inv_idcg,
                                                n_total, do_norm);
          acc_g[m] -= p.va;
          acc_h[m] += p.hess;
          pg += p.va;
          ph += p.hess;
          s_loc += -2.0 * p.lam;
        }
      }
      pg = WaveSum(pg);
      ph = WaveSum(ph);
      if (lane == 0) {
        part_g[(i - c0) * kWaves + wave] = pg;
        part_h[(i - c0) * kWaves + wave] = ph;
      }
    }
    __syncthreads();  // part[] complete; the rows are free for the next chunk
    if (t < c1 - c0) {
      double g = 0.0, h = 0.0;
      for (int w = 0; w < kWaves; ++w) {
        g += part_g[t * kWaves + w];
        h += part_h[t * kWaves + w];
      }
      a.row_g[rbase + c0 + t] = g;
      a.row_h[rbase + c0 + t] = h;
    }
    // the next chunk rewrites part[] only after its own first barrier
  }

  s_loc = WaveSum(s_loc);
  if (lane == 0) wsum[wave] = s_loc;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += wsum[w];
    a.s_part[a.item_off[it.gidx] + it.start / kSlab] = s;
  }
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int j = it.start + t + m * kThreads;
    if (j < n) {
      a.col_g[off + j] = acc_g[m];
      a.col_h[off + j] = acc_h[m];
    }
  }
}

// ---- 4. finish --------------------------------------------------------------

template <int kPer>
__global__ __launch_bounds__(kThreads) void SlabFinishKernel(const SlabArgs a) {
  constexpr int kSlab = kThreads * kPer;
  const Item it = LoadItem(a);
  if (!it.ok) return;
  const int t = (int)threadIdx.x;
  const int n = it.n;
  const long long off = a.doc_off[it.gidx];
  const int kk = a.k < n ? a.k : n;
  const int first = a.item_off[it.gidx];
  const int n_slabs = (n + kSlab - 1) / kSlab;
  const long long rbase = a.row_off[it.gidx];

  double norm = 1.0;
  if (a.normalize) {
    double sum = 0.0;
    for (int s = 0; s < n_slabs; ++s) sum += a.s_part[first + s];
    norm = GroupNorm(sum);
  }
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int j = it.start + t + m * kThreads;
    if (j < n) {
      double g = a.col_g[off + j];
      double h = a.col_h[off + j];
      if (j < kk) {
        // the slabs that have a column above rank j wrote its row share
        for (int s = (j + 1) / kSlab; s < n_slabs; ++s) {
          const int end = (s + 1) * kSlab < n ? (s + 1) * kSlab : n;
          if (end - 1 > j) {
            g += a.row_g[rbase + (long long)s * kk + j];
            h += a.row_h[rbase + (long long)s * kk + j];
          }
        }
      }
      const int doc = a.r_doc[off + j];
      if (doc < 0 || doc >= n) continue;  // never: the ranks are a permutation
      StoreGpair(a.out_g, a.out_h, it.base + doc, g, h, norm, a.weight);
    }
  }
}

template <int kMetric, int kPer>
void LaunchChain(const SlabArgs& a, hipStream_t stream) {
  const dim3 grid(a.n_items), block(kThreads);
  hipLaunchKernelGGL(SlabRankKernel<kPer>, grid, block, 0, stream, a);
  if constexpr (kMetric == kMap) {
    hipLaunchKernelGGL(SlabMapScanKernel, grid, block, 0, stream, a);
  }
  hipLaunchKernelGGL((SlabPairsKernel<kMetric, kPer>), grid, block, 0, stream,
                     a);
  hipLaunchKernelGGL(SlabFinishKernel<kPer>, grid, block, 0, stream, a);
}

template <int kMetric>
void LaunchShape(int shape, const SlabArgs& a, hipStream_t stream) {
  switch (shape) {
    case 0: LaunchChain<kMetric, 1>(a, stream); break;
    case 1: LaunchChain<kMetric, 2>(a, stream); break;
    case 2: LaunchChain<kMetric, 4>(a, stream); break;
    case 3: LaunchChain<kMetric, 8>(a, stream); break;
    default: break;
  }
}

}  // namespace

extern "C" {

int gbt_lambdarank_slab_size(int shape) {
  return shape >= 0 && shape <= 3 ? kThreads << shape : 0;
}

void gbt_lambdarank_slab(int metric, int shape, const float* scores,
                         const float* labels, const long long* group_ptr,
                         const double* inv_idcg, const double* weight,
                         const int32_t* items, int n_items,
                         const int32_t* item_off, const long long* doc_off,
                         const long long* row_off, int k, int score_norm,
                         int normalize, int exp_gain, long long n_docs,
                         long long n_rows, float* scratch_f32,
                         int32_t* scratch_i32, double* scratch_f64,
                         float* out_g, float* out_h, hipStream_t stream) {
  if (n_items <= 0) return;
  SlabArgs a;
  a.scores = scores;
  a.labels = labels;
  a.group_ptr = group_ptr;
  a.inv_idcg = inv_idcg;
  a.weight = weight;
  a.items = items;
  a.item_off = item_off;
  a.doc_off = doc_off;
  a.row_off = row_off;
  a.n_items = n_items;
  a.k = k;
  a.score_norm = score_norm;
  a.normalize = normalize;
  a.exp_gain = exp_gain;
  a.r_score = scratch_f32;
  a.r_label = scratch_f32 + n_docs;
  a.r_doc = scratch_i32;
  a.st0 = scratch_f64;
  a.st1 = a.st0 + n_docs;
  a.col_g = a.st1 + n_docs;
  a.col_h = a.col_g + n_docs;
  a.row_g = a.col_h + n_docs;
  a.row_h = a.row_g + n_rows;
  a.s_part = a.row_h + n_rows;
  a.out_g = out_g;
  a.out_h = out_h;
  switch (metric) {
    case kNdcg: LaunchShape<kNdcg>(shape, a, stream); break;
    case kMap: LaunchShape<kMap>(shape, a, stream); break;
    case kPairwise: LaunchShape<kPairwise>(shape, a, stream); break;
    default: break;
  }
}

}  // extern "C"
