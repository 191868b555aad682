// Split evaluation for CDNA4: one 256-thread block (four wave64s) per
// (feature, node), one thread per bin.
//
// Reference behavior: src/tree/gpu_hist/evaluate_splits.cu
// EvaluateSplitsKernel — which hard-codes 32-thread warps; this is a
// wave64 re-design: an int64 shuffle-based inclusive scan (exact:
// quantized sums) per wave, the wave totals joined through LDS, then
// gains in float64 with the exact operation order of the numpy oracle
// (xgboost_amd/splits.py) so results match bit-for-bit.  The first form,
// one wave64 walking a feature in 64-bin chunks, remains as the
// reference entry point and for features wider than the block.  The gain
// arithmetic itself (TryCandidate) lives in split_gain.h.
#include "gbt_kernels.h"
#include "split_gain.h"

#include <algorithm>

namespace {

__device__ __forceinline__ long long ShflUpLL(long long v, int delta) {
  return __shfl_up(v, delta, 64);
}

// wave argmax reduce with the full tie key; lane 0 holds the result
__device__ __forceinline__ void WaveArgmax(Best* best) {
  for (int off = 32; off > 0; off >>= 1) {
    Best other;
    other.gain = __shfl_down(best->gain, off, 64);
    other.bin = __shfl_down(best->bin, off, 64);
    other.dir = __shfl_down(best->dir, off, 64);
    other.lg = __shfl_down(best->lg, off, 64);
    other.lh = __shfl_down(best->lh, off, 64);
    if (other.bin >= 0 && (best->bin < 0 || Better(other, *best)))
      *best = other;
  }
}

// the launch arguments shared by the three evaluate kernels
struct EvalArgs {
  const int64_t* hist;
  int n_nodes, n_bins, n_features;
  const int32_t* cut_ptrs;
  const int64_t* parent_sums;
  const float* maxabs;   // null, or [2]: derive scales on device so no
                         // host sync is needed before the root evaluation
  const int32_t* k_dev;  // null, or the live node count: whole-tree mode
                         // launches a worst-case grid
  int narrow_max;  // >0: skip numeric features with <= this many bins
                   // (EvaluateNarrowKernel owns them — a wave per 2-bin
                   // one-hot feature wastes 97% of the machine on sparse
                   // data)
  double g_scale, h_scale;
  double reg_lambda, reg_alpha, max_delta_step, min_child_weight;
  const int8_t* monotone;
  const double* node_bounds;
  int mask_stride;  // n_features = per-node mask rows; 0 = one per-tree
                    // row broadcast to every node
  const uint8_t* feature_mask;
  const uint8_t* cat_feature;
  double* out_gain;
  int32_t* out_bin;
  uint8_t* out_dir;
  int64_t* out_lsum;
};

// everything one (node, feature) evaluation needs besides the bins
struct FeatCtx {
  SplitParams p;
  int mono;
  bool is_cat;
  int fb0, fb1;
  long long pg, ph;
  double inv_g, inv_h, parent_gain;
  const int64_t* nh;  // the node's histogram
  size_t out_idx;
};

// Who writes a (node, feature) slot: the narrow kernel takes the numeric
// features of at most narrow_max bins, the block kernel the rest.
__device__ __forceinline__ bool NarrowOwns(const EvalArgs& a, int width,
                                           bool is_cat) {
  return a.narrow_max > 0 && width <= a.narrow_max && !is_cat;
}

// the dequantisation factors, from host scales or the device max-abs pair
__device__ __forceinline__ void SetScales(const EvalArgs& a, FeatCtx* c) {
  double g_scale = a.g_scale, h_scale = a.h_scale;
  if (a.maxabs != nullptr) {
    // identical derivation to the host/QuantizeKernel formula
    g_scale = a.maxabs[0] > 0.f ? 1073741824.0 / (double)a.maxabs[0] : 1.0;
    h_scale = a.maxabs[1] > 0.f ? 1073741824.0 / (double)a.maxabs[1] : 1.0;
  }
  c->inv_g = 1.0 / g_scale;
  c->inv_h = 1.0 / h_scale;
}

// two fp64 divisions: only for a slot that has candidates to compare
__device__ __forceinline__ void SetParentGain(FeatCtx* c) {
  const double pw = CalcWeight(c->pg * c->inv_g, c->ph * c->inv_h, c->p);
  c->parent_gain =
      GainGivenWeight(c->pg * c->inv_g, c->ph * c->inv_h, pw, c->p);
}

// Claims the slot (node, f) for the narrow kernel (kNarrow) or a block
// kernel and fills *c.  False = this kernel writes nothing more to the
// slot: the other kernel owns it, or the feature is masked (then `writer`
// stores gain and bin of the no-split record).  Uniform over the threads
// that share a slot.  The narrow kernel sets its scales once per thread
// and the parent gain only for a feature the node's rows have, so for it
// both stay out of here.
template <bool kNarrow>
__device__ __forceinline__ bool SetupFeature(const EvalArgs& a, int node,
                                             int f, bool writer,
                                             FeatCtx* c) {
  c->out_idx = (size_t)node * a.n_features + f;
  c->fb0 = a.cut_ptrs[f];
  c->fb1 = a.cut_ptrs[f + 1];
  c->is_cat = a.cat_feature && a.cat_feature[f];
  if (NarrowOwns(a, c->fb1 - c->fb0, c->is_cat) != kNarrow) return false;
  if (a.feature_mask != nullptr &&
      a.feature_mask[(size_t)node * a.mask_stride + f] == 0) {
    if (writer) {
      a.out_gain[c->out_idx] = -INFINITY;
      a.out_bin[c->out_idx] = -1;
    }
    return false;
  }
  c->p.lam = a.reg_lambda;
  c->p.alpha = a.reg_alpha;
  c->p.mds = a.max_delta_step;
  c->p.mcw = a.min_child_weight;
  c->p.lo = a.node_bounds ? a.node_bounds[2 * node] : -INFINITY;
  c->p.hi = a.node_bounds ? a.node_bounds[2 * node + 1] : INFINITY;
  c->mono = a.monotone ? (int)a.monotone[f] : 0;
  c->pg = a.parent_sums[2 * node];
  c->ph = a.parent_sums[2 * node + 1];
  c->nh = a.hist + (size_t)node * a.n_bins * 2;
  if (!kNarrow) {
    SetScales(a, c);
    SetParentGain(c);
  }
  return true;
}

__device__ __forceinline__ void WriteBest(const EvalArgs& a, size_t out_idx,
                                          const Best& best) {
  a.out_gain[out_idx] = best.gain;
  a.out_bin[out_idx] = best.bin;
  a.out_dir[out_idx] = (uint8_t)best.dir;
  a.out_lsum[2 * out_idx] = best.lg;
  a.out_lsum[2 * out_idx + 1] = best.lh;
}

// One wave64 evaluates one (node, feature) of any width: a totals pass,
// then per missing direction a walk over the bins in 64-wide chunks with
// an int64 shuffle scan.  This is the original evaluator; it serves the
// reference entry point and features wider than EvaluateKernel's block.
__device__ void EvaluateFeatureWave(const EvalArgs& a, const FeatCtx& c,
                                    int lane) {
  const int64_t* nh = c.nh;
  const int fb0 = c.fb0, fb1 = c.fb1;
  const long long pg = c.pg, ph = c.ph;

  // pass 1: feature totals (wave reduce)
  long long fg = 0, fh = 0;
  for (int b = fb0 + lane; b < fb1; b += 64) {
    fg += nh[2 * b];
    fh += nh[2 * b + 1];
  }
  for (int off = 32; off > 0; off >>= 1) {
    fg += __shfl_down(fg, off, 64);
    fh += __shfl_down(fh, off, 64);
  }
  fg = __shfl(fg, 0, 64);
  fh = __shfl(fh, 0, 64);
  const long long miss_g = pg - fg;
  const long long miss_h = ph - fh;

  Best best{-INFINITY, -1, 0, 0, 0};

  for (int dir = 0; dir < 2; ++dir) {
    const long long add_g = dir ? miss_g : 0;
    const long long add_h = dir ? miss_h : 0;
    long long run_g = 0, run_h = 0;
    for (int b0 = fb0; b0 < fb1; b0 += 64) {
      const int b = b0 + lane;
      const bool valid = b < fb1;
      long long sg = valid ? (long long)nh[2 * b] : 0;
      long long sh = valid ? (long long)nh[2 * b + 1] : 0;
      long long glq, hlq;
      if (c.is_cat) {
        // one-vs-rest: category bin goes RIGHT
        glq = pg - sg - (dir ? 0 : miss_g);
        hlq = ph - sh - (dir ? 0 : miss_h);
      } else {
        // inclusive wave scan (int64: exact)
        for (int off = 1; off < 64; off <<= 1) {
          const long long tg = ShflUpLL(sg, off);
          const long long th = ShflUpLL(sh, off);
          if (lane >= off) {
            sg += tg;
            sh += th;
          }
        }
        sg += run_g;
        sh += run_h;
        glq = sg + add_g;
        hlq = sh + add_h;
      }
      if (valid) {
        TryCandidate(glq, hlq, pg, ph, c.inv_g, c.inv_h, c.p, c.mono,
                     c.parent_gain, b, dir, &best);
      }
      if (!c.is_cat) {
        run_g = __shfl(sg, 63, 64);
        run_h = __shfl(sh, 63, 64);
      }
    }
  }

  WaveArgmax(&best);
  if (lane == 0) WriteBest(a, c.out_idx, best);
}

}  // namespace

// Reference evaluator: one wave64 per (feature, node).
__global__ __launch_bounds__(64) void EvaluateRefKernel(EvalArgs a) {
  const int node = blockIdx.y;
  if (a.k_dev != nullptr && node >= *a.k_dev) return;
  const int lane = threadIdx.x;
  for (int f = blockIdx.x; f < a.n_features; f += gridDim.x) {
    FeatCtx c;
    if (!SetupFeature<false>(a, node, f, lane == 0, &c)) continue;
    EvaluateFeatureWave(a, c, lane);
  }
}

// Single-pass evaluator: one 256-thread block per (feature, node), one
// thread per bin.  Each thread loads its bin once; an int64 wave scan
// plus the four wave totals through LDS give its inclusive prefix, and
// the sum of the four totals is the feature total, so the missing-value
// remainder needs no pass of its own.  Both missing directions are
// evaluated from that one prefix and reduced with the total order of
// `Better` (gain, then dir ascending, then bin ascending), so the result
// does not depend on the reduction order.
constexpr int kEvalBlock = 256;
constexpr int kEvalWaves = kEvalBlock / 64;

__global__ __launch_bounds__(kEvalBlock) void EvaluateKernel(EvalArgs a) {
  __shared__ long long s_tg[kEvalWaves], s_th[kEvalWaves];
  __shared__ double s_gain[kEvalWaves];
  __shared__ int s_key[kEvalWaves];
  const int node = blockIdx.y;
  // block-uniform exits: this return and the `continue`s below stay ahead
  // of every barrier in the loop body
  if (a.k_dev != nullptr && node >= *a.k_dev) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  for (int f = blockIdx.x; f < a.n_features; f += gridDim.x) {
    FeatCtx c;
    if (!SetupFeature<false>(a, node, f, tid == 0, &c)) continue;
    const int width = c.fb1 - c.fb0;
    if (width > kEvalBlock) {
      // max_bin 512 / 1024: wider than the block, wave 0 walks it
      if (wave == 0) EvaluateFeatureWave(a, c, lane);
      continue;
    }
    const int b = c.fb0 + tid;
    const bool valid = tid < width;
    const long long own_g = valid ? (long long)c.nh[2 * b] : 0;
    const long long own_h = valid ? (long long)c.nh[2 * b + 1] : 0;
    // inclusive wave scan (int64: exact), then the totals of the waves
    // before this one
    long long sg = own_g, sh = own_h;
    for (int off = 1; off < 64; off <<= 1) {
      const long long tg = ShflUpLL(sg, off);
      const long long th = ShflUpLL(sh, off);
      if (lane >= off) {
        sg += tg;
        sh += th;
      }
    }
    if (lane == 63) {
      s_tg[wave] = sg;
      s_th[wave] = sh;
    }
    __syncthreads();
    long long fg = 0, fh = 0;
    for (int w = 0; w < kEvalWaves; ++w) {
      const long long tg = s_tg[w], th = s_th[w];
      if (w < wave) {
        sg += tg;
        sh += th;
      }
      fg += tg;
      fh += th;
    }
    const long long miss_g = c.pg - fg;
    const long long miss_h = c.ph - fh;

    Best best{-INFINITY, -1, 0, 0, 0};
    if (valid) {
      // With no missing remainder both directions give the same sums and
      // the same gain; dir 0 wins that tie, so dir 1 is not evaluated.
      const int n_dir = (miss_g != 0 || miss_h != 0) ? 2 : 1;
      for (int dir = 0; dir < n_dir; ++dir) {
        long long glq, hlq;
        if (c.is_cat) {
          // one-vs-rest: category bin goes RIGHT
          glq = c.pg - own_g - (dir ? 0 : miss_g);
          hlq = c.ph - own_h - (dir ? 0 : miss_h);
        } else {
          glq = sg + (dir ? miss_g : 0);
          hlq = sh + (dir ? miss_h : 0);
        }
        TryCandidate(glq, hlq, c.pg, c.ph, c.inv_g, c.inv_h, c.p, c.mono,
                     c.parent_gain, b, dir, &best);
      }
    }
    // Block argmax over the tie key alone: (gain, dir, bin) with dir and
    // bin packed so that a smaller word is the better tie.  A thread's
    // key names its bin, so the winner is one thread, and that thread
    // writes its own left sums: no payload travels through shuffles.
    const int none = 0x7fffffff;
    const int my_key = best.bin < 0 ? none : ((best.dir << 30) | best.bin);
    double win_gain = best.gain;
    int win_key = my_key;
    for (int off = 32; off > 0; off >>= 1) {
      const double og = __shfl_down(win_gain, off, 64);
      const int ok = __shfl_down(win_key, off, 64);
      const bool take = og > win_gain || (og == win_gain && ok < win_key);
      win_gain = take ? og : win_gain;
      win_key = take ? ok : win_key;
    }
    if (lane == 0) {
      s_gain[wave] = win_gain;
      s_key[wave] = win_key;
    }
    __syncthreads();
    win_gain = s_gain[0];
    win_key = s_key[0];
    for (int w = 1; w < kEvalWaves; ++w) {
      const double og = s_gain[w];
      const int ok = s_key[w];
      const bool take = og > win_gain || (og == win_gain && ok < win_key);
      win_gain = take ? og : win_gain;
      win_key = take ? ok : win_key;
    }
    if (win_key == none) {
      if (tid == 0) WriteBest(a, c.out_idx, best);  // the no-split record
    } else if (my_key == win_key) {
      WriteBest(a, c.out_idx, best);
    }
    // the next iteration's LDS writes each sit behind one of its own
    // barriers, which a thread reaches only after these reads
  }
}

// Scalar evaluation for NARROW numeric features (one-hot scale sparse
// data: millions of 2-bin features).  One THREAD per (node, feature);
// the same TryCandidate and tie rule as the block kernel, so results are
// bit-identical — only the parallelization differs.
__global__ __launch_bounds__(256) void EvaluateNarrowKernel(EvalArgs a) {
  FeatCtx c;
  SetScales(a, &c);
  const int kn = (a.k_dev != nullptr) ? *a.k_dev : a.n_nodes;
  const long long total = (long long)kn * a.n_features;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += stride) {
    const int node = (int)(idx / a.n_features);
    const int f = (int)(idx % a.n_features);
    if (!SetupFeature<true>(a, node, f, true, &c)) continue;
    long long fg = 0, fh = 0;
    for (int b = c.fb0; b < c.fb1; ++b) {
      fg += c.nh[2 * b];
      fh += c.nh[2 * b + 1];
    }
    Best best{-INFINITY, -1, 0, 0, 0};
    if (fh == 0 && fg == 0) {
      // feature absent from this node's rows: every candidate split is
      // empty-vs-all and fails the exact hessian-count validity — the
      // common case for one-hot features in deep nodes, so it leaves
      // before the parent gain's divisions
      WriteBest(a, c.out_idx, best);
      continue;
    }
    const long long miss_g = c.pg - fg;
    const long long miss_h = c.ph - fh;
    SetParentGain(&c);
    for (int dir = 0; dir < 2; ++dir) {
      long long sg = dir ? miss_g : 0, sh = dir ? miss_h : 0;
      for (int b = c.fb0; b < c.fb1; ++b) {
        sg += c.nh[2 * b];
        sh += c.nh[2 * b + 1];
        TryCandidate(sg, sh, c.pg, c.ph, c.inv_g, c.inv_h, c.p, c.mono,
                     c.parent_gain, b, dir, &best);
      }
    }
    WriteBest(a, c.out_idx, best);
  }
}

// Second stage: per-node argmax over features -> packed [n_nodes, 6]
// (gain bits, bin, dir, left_gq, left_hq, feature).  One block per node;
// tie rule matches numpy flat argmax: higher gain wins, ties -> lower
// feature index (the per-feature stage already resolved bin/dir ties).
// kBlock = 64 is one wave per node; kBlock = 1024 adds an LDS reduction
// across its 16 waves for wide feature counts (one 64-thread wave over
// 1e6 one-hot features was 5.4 ms/launch on the Criteo shape).
template <int kBlock>
__global__ __launch_bounds__(kBlock) void SelectBestKernel(
    const double* __restrict__ gain, const int32_t* __restrict__ bins,
    const uint8_t* __restrict__ dirs, const int64_t* __restrict__ lsum,
    int n_features, int64_t* __restrict__ out_best,
    const int32_t* __restrict__ k_dev) {
  const int node = blockIdx.x;
  if (k_dev != nullptr && node >= *k_dev) return;
  const size_t base = (size_t)node * n_features;
  double best_gain = -INFINITY;
  int best_f = -1;
  for (int f = (int)threadIdx.x; f < n_features; f += kBlock) {
    const double gv = gain[base + f];
    if (gv > best_gain) {
      best_gain = gv;
      best_f = f;
    }
  }
  auto take = [&](double og, int of) {
    if (of >= 0 && (best_f < 0 || og > best_gain ||
                    (og == best_gain && of < best_f))) {
      best_gain = og;
      best_f = of;
    }
  };
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_down(best_gain, off, 64);
    const int of = __shfl_down(best_f, off, 64);
    take(og, of);
  }
  if constexpr (kBlock > 64) {
    __shared__ double s_g[kBlock / 64];
    __shared__ int s_f[kBlock / 64];
    if ((threadIdx.x & 63) == 0) {
      s_g[threadIdx.x >> 6] = best_gain;
      s_f[threadIdx.x >> 6] = best_f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < kBlock / 64; ++w) take(s_g[w], s_f[w]);
    }
  }
  if (threadIdx.x == 0) {
    int64_t* out = out_best + (size_t)node * 6;
    if (best_f < 0 || !isfinite(best_gain)) {
      out[0] = 0;
      out[1] = -1;
      out[2] = 0;
      out[3] = 0;
      out[4] = 0;
      out[5] = -1;
    } else {
      const size_t idx = base + best_f;
      out[0] = __double_as_longlong(best_gain);
      out[1] = bins[idx];
      out[2] = dirs[idx];
      out[3] = lsum[2 * idx];
      out[4] = lsum[2 * idx + 1];
      out[5] = best_f;
    }
  }
}

extern "C" void gbt_select_best(const double* gain, const int32_t* bins,
                                const uint8_t* dirs, const int64_t* lsum,
                                int n_nodes, int n_features,
                                int64_t* out_best, const int32_t* k_dev,
                                hipStream_t stream) {
  if (n_features > 4096) {
    hipLaunchKernelGGL(SelectBestKernel<1024>, dim3(n_nodes), dim3(1024), 0,
                       stream, gain, bins, dirs, lsum, n_features, out_best,
                       k_dev);
    return;
  }
  hipLaunchKernelGGL(SelectBestKernel<64>, dim3(n_nodes), dim3(64), 0, stream,
                     gain, bins, dirs, lsum, n_features, out_best, k_dev);
}

namespace {

// ref: launch the single-wave reference kernel instead of the
// one-thread-per-bin kernel; everything else is the same.
void LaunchEvaluate(
    bool ref, const int64_t* hist, int n_nodes, int n_bins, int n_features,
    const int32_t* cut_ptrs, const int64_t* parent_sums,
    const float* maxabs, double g_scale,
    double h_scale, double reg_lambda, double reg_alpha,
    double max_delta_step, double min_child_weight, const int8_t* monotone,
    const double* node_bounds, int mask_stride,
    const uint8_t* feature_mask,
    const uint8_t* cat_feature, double* out_gain, int32_t* out_bin,
    uint8_t* out_dir, int64_t* out_lsum, const int32_t* k_dev,
    int narrow_max, hipStream_t stream) {
  const EvalArgs ea{hist, n_nodes, n_bins, n_features, cut_ptrs, parent_sums,
                    maxabs, k_dev, narrow_max, g_scale, h_scale, reg_lambda,
                    reg_alpha, max_delta_step, min_child_weight, monotone,
                    node_bounds, mask_stride, feature_mask, cat_feature,
                    out_gain, out_bin, out_dir, out_lsum};
  dim3 grid(n_features > 65535 ? 65535 : n_features, n_nodes);
  if (ref) {
    hipLaunchKernelGGL(EvaluateRefKernel, grid, dim3(64), 0, stream, ea);
  } else {
    hipLaunchKernelGGL(EvaluateKernel, grid, dim3(kEvalBlock), 0, stream, ea);
  }
  if (narrow_max > 0) {
    const long long total = (long long)n_nodes * n_features;
    const int blocks =
        (int)std::min<long long>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(EvaluateNarrowKernel, dim3(blocks), dim3(256), 0,
                       stream, ea);
  }
}

}  // namespace

// mask_stride: n_features = per-node mask rows; 0 = ONE per-tree row
// broadcast to every node (the native driver's colsample_bytree path)
extern "C" void gbt_evaluate_masked(
    const int64_t* hist, int n_nodes, int n_bins, int n_features,
    const int32_t* cut_ptrs, const int64_t* parent_sums,
    const float* maxabs, double g_scale,
    double h_scale, double reg_lambda, double reg_alpha,
    double max_delta_step, double min_child_weight, const int8_t* monotone,
    const double* node_bounds, int mask_stride,
    const uint8_t* feature_mask,
    const uint8_t* cat_feature, double* out_gain, int32_t* out_bin,
    uint8_t* out_dir, int64_t* out_lsum, const int32_t* k_dev,
    int narrow_max, hipStream_t stream) {
  LaunchEvaluate(false, hist, n_nodes, n_bins, n_features, cut_ptrs,
                 parent_sums, maxabs, g_scale, h_scale, reg_lambda, reg_alpha,
                 max_delta_step, min_child_weight, monotone, node_bounds,
                 mask_stride, feature_mask, cat_feature, out_gain, out_bin,
                 out_dir, out_lsum, k_dev, narrow_max, stream);
}

// The single-wave evaluator behind the same arguments: the reference
// the tests compare gbt_evaluate_masked against, bit for bit.
extern "C" void gbt_evaluate_ref(
    const int64_t* hist, int n_nodes, int n_bins, int n_features,
    const int32_t* cut_ptrs, const int64_t* parent_sums,
    const float* maxabs, double g_scale,
    double h_scale, double reg_lambda, double reg_alpha,
    double max_delta_step, double min_child_weight, const int8_t* monotone,
    const double* node_bounds, int mask_stride,
    const uint8_t* feature_mask,
    const uint8_t* cat_feature, double* out_gain, int32_t* out_bin,
    uint8_t* out_dir, int64_t* out_lsum, const int32_t* k_dev,
    int narrow_max, hipStream_t stream) {
  LaunchEvaluate(true, hist, n_nodes, n_bins, n_features, cut_ptrs,
                 parent_sums, maxabs, g_scale, h_scale, reg_lambda, reg_alpha,
                 max_delta_step, min_child_weight, monotone, node_bounds,
                 mask_stride, feature_mask, cat_feature, out_gain, out_bin,
                 out_dir, out_lsum, k_dev, narrow_max, stream);
}
