// LambdaMART gradients (rank:ndcg, rank:map, rank:pairwise), one query
// group per workgroup, everything between the score read and the
// gradient write in LDS and registers.
//
// Specification: _LambdaRankBase.get_gradient (objectives.py), top-k pair
// method, which follows the reference's LambdaGrad / MakePairs
// (src/objective/lambdarank_obj.h); the pair gradient, the rank key, the
// statistics' terms, the normaliser and the final write are rank_common.h's,
// shared with the slab tier.  The reference's device path is one
// thread per pair with global atomics; fp64 atomics CAS-loop here and the
// head documents are ~n-way contended, so this kernel has no atomics:
//
//  1. stage   each thread loads its documents (doc d = t, t + T, ...),
//             writes a 32-bit order-preserving key of the score to LDS
//  2. rank    rank-by-counting on the composite key (score desc, doc
//             asc) -- unique keys, so the ranks are a permutation and
//             equal scores come out in document order -- then scatter
//             score, label, doc index to their rank slot
//  3. stats   ndcg: discount and gain per rank; map: fp64 block scan of
//             n_rel and acc = cumsum(y/(r+1)) down the list
//  4. pairs   rows i < min(k, n); each thread owns the columns
//             j = t, t + T, ... and keeps their g/h sums in registers.
//             Pair (i, j) is evaluated once: the column share goes to the
//             thread's register, the row share is summed over the wave
//             with a shuffle butterfly and parked in part[i][wave].  One
//             barrier per kRowChunk rows (one in all for k <= 64), then
//             the owner of column i folds part[i][*] in wave order.
//  5. write   StoreGpair through the rank -> document map.
//
// Every sum has a fixed order, so a tier's output is bit-reproducible.
// Tiers: groups of <= 64 documents take one wave each (four per block,
// no block barrier anywhere); larger groups take one block each.
#include "gbt_kernels.h"
#include "rank_common.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kRowChunk = 64;  // rows between two barriers of the pair loop
constexpr int kPairwise = 2;

struct LambdaRankArgs {
  const float* scores;
  const float* labels;
  const long long* group_ptr;
  const double* inv_idcg;  // [G], ndcg only
  const double* weight;    // [N] or null
  const int32_t* work;     // group ids of this tier
  int n_work;
  int k;
  int score_norm;
  int normalize;
  int exp_gain;
  float* out_g;
  float* out_h;
};

template <int kCap, int kWaves>
struct GroupLds {
  // by-rank statistics: ndcg {discount, gain}, map {n_rel, acc}.  The
  // staging keys (by document) are dead before the statistics are built
  // and share st0's storage.
  union {
    unsigned int key[kCap];
    double st0[kCap];
  };
  double st1[kCap];
  float score[kCap];  // by rank
  float label[kCap];  // by rank
  unsigned short doc[kCap];  // rank -> document index within the group
  double part_g[kWaves > 1 ? kRowChunk * kWaves : 1];
  double part_h[kWaves > 1 ? kRowChunk * kWaves : 1];
  double wsum[kWaves];
  double scan_c[kWaves];
  double scan_a[kWaves];
};

template <int kMetric, int kCap, int kThreads, int kGroups>
__global__ __launch_bounds__(kThreads* kGroups) void LambdaRankKernel(
    const LambdaRankArgs a) {
  constexpr int kWaves = kThreads / kWave;
  constexpr int kPer = kCap / kThreads;  // columns per thread
  static_assert(kThreads % kWave == 0 && kCap % kThreads == 0, "tier shape");
  static_assert(kGroups == 1 || kWaves == 1, "shared blocks: one wave each");
  static_assert(kCap <= 65536, "doc index is 16 bit");
  __shared__ GroupLds<kCap, kWaves> lds_all[kGroups];

  const int slot = (int)threadIdx.x / kThreads;
  const int t = (int)threadIdx.x % kThreads;
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  const int w_idx = (int)blockIdx.x * kGroups + slot;
  if (w_idx >= a.n_work) return;  // whole waves, one-wave tier only
  GroupLds<kCap, kWaves>& s = lds_all[slot];
  const int gidx = a.work[w_idx];
  const long long base = a.group_ptr[gidx];
  const int n = (int)(a.group_ptr[gidx + 1] - base);
  // the host schedules neither; uniform over the threads of the group
  if (n < 1 || n > kCap) return;

  // ---- 1. stage ---------------------------------------------------------
  float my_s[kPer], my_y[kPer];
  unsigned long long my_key[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int d = t + m * kThreads;
    my_s[m] = 0.0f;
    my_y[m] = 0.0f;
    my_key[m] = 0;
    if (d < n) {
      my_s[m] = a.scores[base + d] + 0.0f;
      my_y[m] = a.labels[base + d];
      const unsigned int key = DescKey(my_s[m]);
      s.key[d] = key;
      my_key[m] = RankKey(key, d);
    }
  }
  GroupSync<kWaves>();

  // ---- 2. rank ----------------------------------------------------------
  int rank[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) rank[m] = 0;
  for (int e = 0; e < n; ++e) {
    const unsigned long long ke = RankKey(s.key[e], e);
#pragma unroll
    for (int m = 0; m < kPer; ++m) rank[m] += ke < my_key[m] ? 1 : 0;
  }
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int d = t + m * kThreads;
    if (d < n) {
      s.score[rank[m]] = my_s[m];
      s.label[rank[m]] = my_y[m];
      s.doc[rank[m]] = (unsigned short)d;
    }
  }
  GroupSync<kWaves>();  // ranked list complete; keys dead from here

  // ---- 3. statistics ----------------------------------------------------
  double inv_idcg = 0.0, n_total = 1.0;
  if constexpr (kMetric == kNdcg) {
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int r = t + m * kThreads;
      if (r < n) {
        s.st0[r] = NdcgDiscount(r);
        s.st1[r] = NdcgGain((double)s.label[r], a.exp_gain);
      }
    }
    inv_idcg = a.inv_idcg[gidx];
  } else if constexpr (kMetric == kMap) {
    // thread t scans the contiguous ranks [t*kPer, (t+1)*kPer)
    const int lo = t * kPer;
    double c = 0.0, ac = 0.0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = lo + q;
      if (e < n) {
        const double y = (double)s.label[e];
        c += y;
        ac += y / (double)(e + 1);
      }
    }
    double run_c, run_a;  // exclusive prefix of this thread's chunk
    MapWaveScan(lane, c, ac, run_c, run_a);
    if constexpr (kWaves > 1) {
      if (lane == kWave - 1) {
        s.scan_c[wave] = c;
        s.scan_a[wave] = ac;
      }
      __syncthreads();
      double pc = 0.0, pa = 0.0;
      for (int w = 0; w < wave; ++w) {
        pc += s.scan_c[w];
        pa += s.scan_a[w];
      }
      run_c = pc + run_c;
      run_a = pa + run_a;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = lo + q;
      if (e < n) {
        const double y = (double)s.label[e];
        run_c += y;
        run_a += y / (double)(e + 1);
        s.st0[e] = run_c;
        s.st1[e] = run_a;
      }
    }
  }
  GroupSync<kWaves>();
  if constexpr (kMetric == kMap) n_total = fmax(s.st0[n - 1], 1e-300);

  // ---- 4. pairs ---------------------------------------------------------
  // LambdaGrad's degenerate-group check: no score normalisation when the
  // best score equals the worst (every group at round 0)
  const bool do_norm = a.score_norm && s.score[0] != s.score[n - 1];
  const int kk = a.k < n ? a.k : n;
  const int n_waves = (n + kWave - 1) / kWave < kWaves
                          ? (n + kWave - 1) / kWave : kWaves;
  const bool wave_on = wave < n_waves;  // else no column of this wave < n
  double acc_g[kPer], acc_h[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    acc_g[m] = 0.0;
    acc_h[m] = 0.0;
  }
  double s_loc = 0.0;  // this thread's share of sum(-2 lambda)
  int c0 = 0;
  do {
    const int c1 = c0 + kRowChunk < kk ? c0 + kRowChunk : kk;
    if (wave_on) {
      for (int i = c0; i < c1; ++i) {
        const float yi = s.label[i];
        const double si = (double)s.score[i];
        double a_i = 0.0, b_i = 0.0;
        if constexpr (kMetric == kNdcg) {
          a_i = s.st0[i];  // discount
          b_i = s.st1[i];  // gain
        } else if constexpr (kMetric == kMap) {
          a_i = s.st0[i] / (double)(i + 1);  // n_rel / rank
          b_i = s.st1[i];                    // acc
        }
        double pg = 0.0, ph = 0.0;
#pragma unroll
        for (int m = 0; m < kPer; ++m) {
          const int j = t + m * kThreads;
          if (j > i && j < n) {
            const float yj = s.label[j];
            if (yj != yi) {
              const double sj = (double)s.score[j];
              const auto col = [&s, j](double& a_j, double& b_j) {
                if constexpr (kMetric == kNdcg) {
                  b_j = s.st1[j];
                  a_j = s.st0[j];
                } else if constexpr (kMetric == kMap) {
                  a_j = s.st0[j] / (double)(j + 1);
                  b_j = s.st1[j - 1];  // acc of the rank above
                }
              };
              const PairTerms p = PairGrad<kMetric>(
                  yi, si, a_i, b_i, yj, sj, col, inv_idcg, n_total, do_norm);
              acc_g[m] -= p.va;
              acc_h[m] += p.hess;
              pg += p.va;
              ph += p.hess;
              s_loc += -2.0 * p.lam;
            }
          }
        }
        pg = WaveSum(pg);
        ph = WaveSum(ph);
        if constexpr (kWaves == 1) {
          // the butterfly leaves the row sum in every lane: its owner
          // takes it, no table
          if (lane == i) {
            acc_g[0] += pg;
            acc_h[0] += ph;
          }
        } else {
          if (lane == 0) {
            s.part_g[(i - c0) * kWaves + wave] = pg;
            s.part_h[(i - c0) * kWaves + wave] = ph;
          }
        }
      }
    }
    const bool last = c1 >= kk;
    if (last) {
      s_loc = WaveSum(s_loc);
      if (lane == 0) s.wsum[wave] = s_loc;
    }
    if constexpr (kWaves > 1) {
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kPer; ++m) {
        const int j = t + m * kThreads;
        if (j >= c0 && j < c1) {
          for (int w = 0; w < n_waves; ++w) {
            acc_g[m] += s.part_g[(j - c0) * kWaves + w];
            acc_h[m] += s.part_h[(j - c0) * kWaves + w];
          }
        }
      }
      if (!last) __syncthreads();  // part[] is rewritten by the next chunk
    }
    c0 = c1;
  } while (c0 < kk);

  // ---- 5. normalise and write --------------------------------------------
  double norm = 1.0;
  if (a.normalize) {
    double sum = 0.0;
    if constexpr (kWaves == 1) {
      sum = s_loc;
    } else {
      for (int w = 0; w < kWaves; ++w) sum += s.wsum[w];
    }
    norm = GroupNorm(sum);
  }
#pragma unroll
  for (int m = 0; m < kPer; ++m) {
    const int j = t + m * kThreads;
    if (j < n) {
      StoreGpair(a.out_g, a.out_h, base + s.doc[j], acc_g[m], acc_h[m], norm,
                 a.weight);
    }
  }
}

template <int kMetric, int kCap, int kThreads, int kGroups>
void Launch(const LambdaRankArgs& a, hipStream_t stream) {
  const int blocks = (a.n_work + kGroups - 1) / kGroups;
  hipLaunchKernelGGL((LambdaRankKernel<kMetric, kCap, kThreads, kGroups>),
                     dim3(blocks), dim3(kThreads * kGroups), 0, stream, a);
}

template <int kMetric>
void LaunchTier(int tier, const LambdaRankArgs& a, hipStream_t stream) {
  switch (tier) {
    case 0: Launch<kMetric, 64, 64, 4>(a, stream); break;
    case 1: Launch<kMetric, 256, 128, 1>(a, stream); break;
    case 2: Launch<kMetric, 256, 256, 1>(a, stream); break;
    case 3: Launch<kMetric, 2048, 256, 1>(a, stream); break;
    case 4: Launch<kMetric, 2048, 512, 1>(a, stream); break;
    default: break;
  }
}

}  // namespace

extern "C" {

int gbt_lambdarank_tier_cap(int tier) {
  switch (tier) {
    case 0: return 64;
    case 1:
    case 2: return 256;
    case 3:
    case 4: return 2048;
    default: return 0;
  }
}

void gbt_lambdarank(int metric, int tier, const float* scores,
                    const float* labels, const long long* group_ptr,
                    const double* inv_idcg, const double* weight,
                    const int32_t* work, int n_work, int k, int score_norm,
                    int normalize, int exp_gain, float* out_g, float* out_h,
                    hipStream_t stream) {
  if (n_work <= 0) return;
  const LambdaRankArgs a{scores, labels, group_ptr, inv_idcg, weight, work,
                         n_work, k, score_norm, normalize, exp_gain, out_g,
                         out_h};
  switch (metric) {
    case kNdcg: LaunchTier<kNdcg>(tier, a, stream); break;
    case kMap: LaunchTier<kMap>(tier, a, stream); break;
    case kPairwise: LaunchTier<kPairwise>(tier, a, stream); break;
    default: break;
  }
}

}  // extern "C"
