// The one definition of the ranking kernels' maths, shared by the LambdaMART
// gradient kernels (lambdarank.hip, lambdarank_slab.hip) and the ranking
// metrics (rank_metric.hip): the rank order, the ndcg gain and discount,
// the rank:map scan step, the pair gradient, the group normaliser and the
// final write.  The gradient pieces are the specification of
// _LambdaRankBase.get_gradient (objectives.py), which follows the
// reference's LambdaGrad (src/objective/lambdarank_obj.h); every tier
// evaluates these fp64 expressions in this operation order, which is what
// keeps the tiers one formula.  Device only.
#pragma once
#include <hip/hip_runtime.h>

constexpr int kWave = 64;

// Metric ids shared by the gradient objectives and the metric kinds; id 2
// is rank:pairwise in the gradient files and pre in rank_metric.hip.
enum : int { kNdcg = 0, kMap = 1 };

// Barrier over the threads that share one group or work item: the block,
// or for a one-wave tier only the wave (the waves of a block run different
// groups of different sizes there, so a block barrier would be wrong as
// well as slow).
template <int kWaves>
__device__ __forceinline__ void GroupSync() {
  if constexpr (kWaves > 1) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

__device__ __forceinline__ double WaveSum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// Ascending float order -> descending unsigned order.  -0 folds into +0,
// so equal floats have equal keys.
__device__ __forceinline__ unsigned int DescKey(float s) {
  const unsigned int u = __float_as_uint(s + 0.0f);
  const unsigned int asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// Score key above, position (or any tie-break) below: unique per document,
// so counting the smaller keys of a group gives a permutation with equal
// scores in position order.
__device__ __forceinline__ unsigned long long RankKey(unsigned int key,
                                                      unsigned int low) {
  return ((unsigned long long)key << 32) | low;
}

__device__ __forceinline__ double NdcgGain(double y, bool exp_gain) {
  return exp_gain ? exp2(y) - 1.0 : y;
}

__device__ __forceinline__ double NdcgDiscount(int rank) {
  return 1.0 / log2((double)(rank + 2));
}

// One wave's step of the rank:map scan over thread-contiguous ranks.  In:
// the sums (c, ac) of this thread's chunk.  Out: the same sums inclusive
// over the lanes up to this one, and in (run_c, run_a) the sums of the
// lanes below it.  The caller adds the totals of the waves (and tiles)
// before this one, in order.
__device__ __forceinline__ void MapWaveScan(int lane, double& c, double& ac,
                                            double& run_c, double& run_a) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double tc = __shfl_up(c, off, kWave);
    const double ta = __shfl_up(ac, off, kWave);
    if (lane >= off) {
      c += tc;
      ac += ta;
    }
  }
  run_c = __shfl_up(c, 1, kWave);
  run_a = __shfl_up(ac, 1, kWave);
  if (lane == 0) {
    run_c = 0.0;
    run_a = 0.0;
  }
}

struct PairTerms {
  double va;    // gradient at the upper row i; the column j takes -va
  double hess;  // both take it
  double lam;   // the pair's lambda; -2 lam goes to the group normaliser
};

// One pair, i ranked above j, labels yi != yj.  (a, b) are a rank's
// statistics: ndcg {discount, gain}; map, with n_rel and acc the running
// sums of y and y / (r + 1) down the list, a_i = n_rel[i] / (i + 1),
// b_i = acc[i] for the upper rank and a_j = n_rel[j] / (j + 1),
// b_j = acc[j - 1] for the lower; pairwise none.  `col(a_j, b_j)` fetches the
// lower rank's pair and is called after the sigmoid: the LDS tier loads and
// divides there, and doing that ahead of the call keeps four more VGPRs
// live across the exp, which costs its rank:map wave tier a wave of
// occupancy.  `do_norm` is LambdaGrad's score normalisation, off for a
// degenerate group.
template <int kMetric, class ColStats>
__device__ __forceinline__ PairTerms PairGrad(float yi, double si, double a_i,
                                              double b_i, float yj, double sj,
                                              ColStats col, double inv_idcg,
                                              double n_total, bool do_norm) {
  const bool swap = yi < yj;  // the lower-ranked doc is better
  const double ds = swap ? sj - si : si - sj;  // high - low
  const double sig = 1.0 / (1.0 + exp(-ds));
  double delta = 1.0, a_j = 0.0, b_j = 0.0;
  col(a_j, b_j);
  if constexpr (kMetric == kNdcg) {
    // (gain_h - gain_l)(disc_h - disc_l): both factors flip sign together
    // under swap
    delta = fabs((b_i - b_j) * (a_i - a_j) * inv_idcg);
  } else if constexpr (kMetric == kMap) {
    // DeltaMAP with positions ordered (i above j)
    delta = fabs((a_i - a_j + (b_j - b_i)) / n_total);
  }
  if (do_norm) delta = delta / (fabs(ds) + 0.01);
  const double lam = (sig - 1.0) * delta;
  const double hess = fmax(sig * (1.0 - sig), 1e-16) * delta * 2.0;
  return {swap ? -lam : lam, hess, lam};
}

// The group normaliser for sum = sum(-2 lambda) over the group's pairs.
__device__ __forceinline__ double GroupNorm(double sum) {
  double norm = 1.0;
  if (sum > 0.0) norm = log2(1.0 + sum) / sum;
  return norm;
}

// Normaliser, weight (null: none), hessian floor, one fp64 -> fp32 cast.
__device__ __forceinline__ void StoreGpair(float* out_g, float* out_h,
                                           long long d, double g, double h,
                                           double norm, const double* weight) {
  g *= norm;
  h *= norm;
  if (weight != nullptr) {
    const double w = weight[d];
    g *= w;
    h *= w;
  }
  out_g[d] = (float)g;
  out_h[d] = (float)fmax(h, 1e-16);
}
