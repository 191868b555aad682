// Sorted-partition split evaluation for wide categorical features on
// CDNA4: the categories of one (node, feature) are ordered by their
// gradient ratio, scanned like the bins of a numeric feature, and the best
// prefix goes LEFT; the complement is emitted as the go-RIGHT bitset that
// partition.hip takes.  The host routine this stands in for is
// splits._sorted_cat_split (reference behaviour:
// src/tree/gpu_hist/evaluate_splits.cu, SortHistogram + the partition
// agent, which sorts every feature of a level with one device-wide
// segmented sort; here each (node, feature) sorts on its own).
//
// Design
//   * Work split: one (node, wide feature) per wave64 (w <= 64) or per
//     256-thread block (64 < w <= kCatCap).  A per-node merge kernel then
//     folds the wide slots into gbt_select_best's record.
//   * Order: rank by counting.  A category's sorted position is the number
//     of categories whose (key, index) is smaller, counted against all
//     keys: readlane broadcasts in the wave tier, broadcast LDS reads
//     (every lane reads the same address: conflict-free) in the block
//     tier.  Chosen over an LDS bitonic network because it needs ONE
//     barrier instead of log^2 w, pads nothing to a power of two, the
//     index tiebreak that makes the order total (and so equal to numpy's
//     stable argsort) is one compare, and a rank stays in the register of
//     the thread that owns the category, which is all the go-RIGHT bitset
//     needs (bit c = rank_c > best position): no sorted index array.  The
//     w^2 compares are 4 M at the cap, where one block takes about 0.4 ms
//     (profiles/categorical_mi355x.md), and the levels that have many
//     (node, feature) pairs fill the chip.
//   * Keys: the fp64 ratio (G*inv_g)/(H*inv_h+lambda) mapped to a uint64
//     that orders as numpy's `<` does: -0.0 and +0.0 collapse to one key
//     (equal: the index decides), a present NaN sorts after +inf, and an
//     absent category (H == 0) sorts after everything.  The present
//     categories are therefore exactly a prefix of the order, position p is
//     present iff its H != 0, and "fewer than two present" is "position 1
//     is absent": nothing is counted.
//   * Scan: (G, H) go to their sorted positions (wave tier: a ds_permute
//     push, registers only; block tier: LDS), then an exact int64
//     inclusive scan (wave shuffle scan + wave totals through LDS, as
//     evaluate.hip).  Its last element is the feature total, so the
//     missing remainder costs no pass.
//   * Gains: TryCandidate<kSeq> with mono = 0 and no node bounds (the host
//     routine applies neither), position j standing in for the bin, so
//     `Better` gives the host's tie rule: missing-right first, lowest j.
//   * LDS, block tier: 24 B per category (8 B key, 8 B + 8 B sorted G and
//     H).  kCatCap = 2048 categories = 48 KiB static (+ 112 B of wave
//     totals): three blocks per 160 KiB CU at 256 threads, 8 categories
//     per thread held in registers.
//   * No atomics, no global scratch beyond the outputs, a fixed evaluation
//     order: bit-reproducible.
#include "gbt_kernels.h"
#include "split_gain.h"

namespace {

constexpr int kCatBlock = 256;
constexpr int kCatWaves = kCatBlock / 64;
constexpr int kCatItems = 8;  // categories per thread at the cap
constexpr int kCatCap = kCatBlock * kCatItems;
constexpr unsigned long long kKeyAbsent = ~0ull;
constexpr int kNoKey = 0x7fffffff;

struct CatArgs {
  const int64_t* hist;  // [n_nodes, n_bins, 2]
  int n_nodes, n_bins, n_features;
  const int32_t* cut_ptrs;
  const int64_t* parent_sums;  // [n_nodes, 2]
  double g_scale, h_scale;
  double reg_lambda, reg_alpha, max_delta_step, min_child_weight;
  int max_prefix;       // max_cat_threshold + 1 candidate positions
  const int32_t* wide;  // [n_wide] feature ids, ascending
  int n_wide;
  const uint8_t* feature_mask;  // null, or [n_nodes, n_features]
  int64_t* out_rec;    // [n_nodes, n_wide, 4]: gain bits, dir, left g, h
  uint32_t* out_bits;  // [n_nodes, n_wide, words]
  int words;
};

struct CatCtx {
  SplitParams p;
  int fb0, w;
  long long pg, ph;
  double inv_g, inv_h, parent_gain;
  const int64_t* nh;  // the node's histogram
  size_t item;        // node * n_wide + slot
};

// Fills *c for (node, slot); false = the node's feature set excludes the
// feature.  Uniform over the threads that share the slot.
__device__ __forceinline__ bool CatSetup(const CatArgs& a, int node, int slot,
                                         CatCtx* c) {
  const int f = a.wide[slot];
  c->item = (size_t)node * a.n_wide + slot;
  c->fb0 = a.cut_ptrs[f];
  c->w = a.cut_ptrs[f + 1] - c->fb0;
  c->nh = a.hist + (size_t)node * a.n_bins * 2;
  if (a.feature_mask != nullptr &&
      a.feature_mask[(size_t)node * a.n_features + f] == 0)
    return false;
  c->p.lam = a.reg_lambda;
  c->p.alpha = a.reg_alpha;
  c->p.mds = a.max_delta_step;
  c->p.mcw = a.min_child_weight;
  c->p.lo = -INFINITY;
  c->p.hi = INFINITY;
  c->pg = a.parent_sums[2 * node];
  c->ph = a.parent_sums[2 * node + 1];
  c->inv_g = 1.0 / a.g_scale;
  c->inv_h = 1.0 / a.h_scale;
  const double pw = CalcWeight(c->pg * c->inv_g, c->ph * c->inv_h, c->p);
  c->parent_gain = GainGivenWeight<true>(c->pg * c->inv_g, c->ph * c->inv_h,
                                         pw, c->p);
  return true;
}

// uint64 whose unsigned order is numpy's order of the ratios, absent last
__device__ __forceinline__ unsigned long long SortKey(long long g,
                                                      long long h,
                                                      const CatCtx& c) {
  if (h == 0) return kKeyAbsent;
  const double r = (g * c.inv_g) / (h * c.inv_h + c.p.lam);
  if (r != r) return kKeyAbsent - 1;  // NaN: after +inf, before absent
  const long long b = __double_as_longlong(r == 0.0 ? 0.0 : r);
  return b < 0 ? ~(unsigned long long)b
               : ((unsigned long long)b | 0x8000000000000000ull);
}

__device__ __forceinline__ int Precedes(unsigned long long ka, int ia,
                                        unsigned long long kb, int ib) {
  return (ka < kb) | ((ka == kb) & (ia < ib));
}

__device__ __forceinline__ void WriteRec(const CatArgs& a, size_t item,
                                         const Best& b) {
  int64_t* r = a.out_rec + 4 * item;
  r[0] = __double_as_longlong(b.gain);
  r[1] = b.dir;
  r[2] = b.lg;
  r[3] = b.lh;
}

// Both missing directions of "the first j+1 sorted categories go left";
// (sg, sh) is the inclusive prefix at j.  With no missing remainder the two
// directions tie and dir 0 wins, so dir 1 is not evaluated.
__device__ __forceinline__ void TryPrefix(const CatCtx& c, int j, long long sg,
                                          long long sh, long long miss_g,
                                          long long miss_h, Best* best) {
  const int n_dir = (miss_g != 0 || miss_h != 0) ? 2 : 1;
  for (int dir = 0; dir < n_dir; ++dir) {
    TryCandidate<true>(sg + (dir ? miss_g : 0), sh + (dir ? miss_h : 0), c.pg,
                       c.ph, c.inv_g, c.inv_h, c.p, 0, c.parent_gain, j, dir,
                       best);
  }
}

__device__ __forceinline__ int TieKey(const Best& b) {
  return b.bin < 0 ? kNoKey : ((b.dir << 30) | b.bin);
}

// wave argmax over (gain, key); every lane returns the winner
__device__ __forceinline__ void WaveArgmaxKey(double* gain, int* key) {
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_down(*gain, off, 64);
    const int ok = __shfl_down(*key, off, 64);
    const bool take = og > *gain || (og == *gain && ok < *key);
    *gain = take ? og : *gain;
    *key = take ? ok : *key;
  }
  *gain = __shfl(*gain, 0, 64);
  *key = __shfl(*key, 0, 64);
}

// lane `dst` receives v (dst is a permutation of the lanes)
__device__ __forceinline__ long long PushLL(int dst, long long v) {
  const int lo = __builtin_amdgcn_ds_permute(dst << 2, (int)v);
  const int hi = __builtin_amdgcn_ds_permute(dst << 2, (int)(v >> 32));
  return ((long long)hi << 32) | (unsigned int)lo;
}

}  // namespace

// w <= 64: one wave64 per (node, wide feature), lane = category, then lane
// = sorted position.  Keys and sums live in registers; the waves of a
// block are independent, so there is no barrier.
__global__ __launch_bounds__(kCatBlock) void EvaluateCatWaveKernel(CatArgs a) {
  const int lane = threadIdx.x & 63;
  const long long item =
      (long long)blockIdx.x * kCatWaves + (threadIdx.x >> 6);
  // wave-uniform exits, ahead of every cross-lane operation
  if (item >= (long long)a.n_nodes * a.n_wide) return;
  CatCtx c;
  const bool live =
      CatSetup(a, (int)(item / a.n_wide), (int)(item % a.n_wide), &c);
  if (c.w > 64) return;  // the block kernel's
  Best best{-INFINITY, -1, 0, 0, 0};
  if (!live) {
    if (lane == 0) WriteRec(a, c.item, best);
    return;
  }
  const bool in = lane < c.w;
  const long long g = in ? (long long)c.nh[2 * (c.fb0 + lane)] : 0;
  const long long h = in ? (long long)c.nh[2 * (c.fb0 + lane) + 1] : 0;
  // lanes past the feature sort as absent categories after the real ones,
  // so the ranks are a permutation of all 64 lanes
  const unsigned long long key = SortKey(g, h, c);
  int rank = 0;
  for (int d = 0; d < 64; ++d) {
    const unsigned long long kd =
        (unsigned long long)__shfl((long long)key, d, 64);
    rank += Precedes(kd, d, key, lane);
  }
  const long long own_g = PushLL(rank, g);
  const long long own_h = PushLL(rank, h);
  long long sg = own_g, sh = own_h;
  for (int off = 1; off < 64; off <<= 1) {
    const long long tg = __shfl_up(sg, off, 64);
    const long long th = __shfl_up(sh, off, 64);
    if (lane >= off) {
      sg += tg;
      sh += th;
    }
  }
  const long long miss_g = c.pg - __shfl(sg, 63, 64);
  const long long miss_h = c.ph - __shfl(sh, 63, 64);
  const bool two_present = __shfl(own_h, 1, 64) != 0;
  if (two_present && own_h != 0 && lane < a.max_prefix)
    TryPrefix(c, lane, sg, sh, miss_g, miss_h, &best);
  const int my_key = TieKey(best);
  double win_gain = best.gain;
  int win_key = my_key;
  WaveArgmaxKey(&win_gain, &win_key);
  if (win_key == kNoKey) {
    if (lane == 0) WriteRec(a, c.item, best);  // the no-split record
    return;
  }
  if (my_key == win_key) WriteRec(a, c.item, best);
  const int j = win_key & 0x3fffffff;
  const unsigned long long right = __ballot(in && rank > j);
  if (lane == 0) {
    uint32_t* bits = a.out_bits + c.item * a.words;
    bits[0] = (uint32_t)right;
    if (c.w > 32) bits[1] = (uint32_t)(right >> 32);
  }
}

// 64 < w <= kCatCap: one block per (node, wide feature).  Thread t owns the
// categories t, t + 256, ... for load, key and rank (a wave covers 64
// consecutive categories: its ballot is two bitset words), and the sorted
// positions 8t .. 8t+7 for the scan and the candidates.
__global__ __launch_bounds__(kCatBlock) void EvaluateCatBlockKernel(CatArgs a) {
  __shared__ unsigned long long s_key[kCatCap];
  __shared__ long long s_g[kCatCap], s_h[kCatCap];
  __shared__ long long s_tg[kCatWaves], s_th[kCatWaves];
  __shared__ double s_gain[kCatWaves];
  __shared__ int s_wkey[kCatWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  CatCtx c;
  // block-uniform exits, ahead of every barrier
  const bool live = CatSetup(a, blockIdx.y, blockIdx.x, &c);
  if (c.w <= 64 || c.w > kCatCap) return;  // the wave kernel's / the host's
  Best best{-INFINITY, -1, 0, 0, 0};
  if (!live) {
    if (tid == 0) WriteRec(a, c.item, best);
    return;
  }
  const int w = c.w;

  long long g[kCatItems], h[kCatItems];
  unsigned long long key[kCatItems];
  int rank[kCatItems];
#pragma unroll
  for (int i = 0; i < kCatItems; ++i) {
    const int cat = tid + i * kCatBlock;
    const bool in = cat < w;
    g[i] = in ? (long long)c.nh[2 * (c.fb0 + cat)] : 0;
    h[i] = in ? (long long)c.nh[2 * (c.fb0 + cat) + 1] : 0;
    key[i] = SortKey(g[i], h[i], c);
    if (in) s_key[cat] = key[i];
  }
  __syncthreads();
  // rank = the number of (key, index) pairs that precede this one; every
  // lane reads the same s_key[d], a broadcast.  (Splitting the loop at the
  // wave's own 64 categories, outside which the index tiebreak is uniform
  // and one compare decides, measured 15 % slower at the cap, so the
  // compares are not what bounds this loop; profiles/categorical_mi355x.md.)
#pragma unroll
  for (int i = 0; i < kCatItems; ++i) {
    rank[i] = 0;
    if (i * kCatBlock < w) {  // block-uniform
      const int cat = tid + i * kCatBlock;
      int r = 0;
      for (int d = 0; d < w; ++d) r += Precedes(s_key[d], d, key[i], cat);
      rank[i] = r;
    }
  }
  // the ranks of the categories below w are a permutation of [0, w)
#pragma unroll
  for (int i = 0; i < kCatItems; ++i) {
    if (tid + i * kCatBlock < w) {
      s_g[rank[i]] = g[i];
      s_h[rank[i]] = h[i];
    }
  }
  __syncthreads();
  // fewer than two present categories: no candidate (w > 64: s_h[1] exists)
  if (s_h[1] == 0) {
    if (tid == 0) WriteRec(a, c.item, best);
    return;
  }
  // thread-local inclusive prefixes of positions 8t .. 8t+7, then the
  // block scan of the thread totals
  long long pre_g[kCatItems], pre_h[kCatItems];
  bool present[kCatItems];
  long long run_g = 0, run_h = 0;
#pragma unroll
  for (int i = 0; i < kCatItems; ++i) {
    const int pos = tid * kCatItems + i;
    const long long og = pos < w ? s_g[pos] : 0;
    const long long oh = pos < w ? s_h[pos] : 0;
    present[i] = oh != 0;
    run_g += og;
    run_h += oh;
    pre_g[i] = run_g;
    pre_h[i] = run_h;
  }
  long long sg = run_g, sh = run_h;
  for (int off = 1; off < 64; off <<= 1) {
    const long long tg = __shfl_up(sg, off, 64);
    const long long th = __shfl_up(sh, off, 64);
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
  long long base_g = sg - run_g, base_h = sh - run_h;  // exclusive
  long long fg = 0, fh = 0;
  for (int v = 0; v < kCatWaves; ++v) {
    const long long tg = s_tg[v], th = s_th[v];
    if (v < wave) {
      base_g += tg;
      base_h += th;
    }
    fg += tg;
    fh += th;
  }
  const long long miss_g = c.pg - fg;
  const long long miss_h = c.ph - fh;
#pragma unroll
  for (int i = 0; i < kCatItems; ++i) {
    const int pos = tid * kCatItems + i;
    if (present[i] && pos < a.max_prefix)
      TryPrefix(c, pos, base_g + pre_g[i], base_h + pre_h[i], miss_g, miss_h,
                &best);
  }
  // block argmax over the tie key, as EvaluateKernel: a key names one
  // position, so the winner is one thread and it writes its own sums
  const int my_key = TieKey(best);
  double win_gain = best.gain;
  int win_key = my_key;
  WaveArgmaxKey(&win_gain, &win_key);
  if (lane == 0) {
    s_gain[wave] = win_gain;
    s_wkey[wave] = win_key;
  }
  __syncthreads();
  win_gain = s_gain[0];
  win_key = s_wkey[0];
  for (int v = 1; v < kCatWaves; ++v) {
    const double og = s_gain[v];
    const int ok = s_wkey[v];
    const bool take = og > win_gain || (og == win_gain && ok < win_key);
    win_gain = take ? og : win_gain;
    win_key = take ? ok : win_key;
  }
  if (win_key == kNoKey) {
    if (tid == 0) WriteRec(a, c.item, best);  // the no-split record
    return;
  }
  if (my_key == win_key) WriteRec(a, c.item, best);
  const int j = win_key & 0x3fffffff;
  uint32_t* bits = a.out_bits + c.item * a.words;
#pragma unroll
  for (int i = 0; i < kCatItems; ++i) {
    const int cat = tid + i * kCatBlock;
    const unsigned long long right = __ballot(cat < w && rank[i] > j);
    const int cat0 = cat - lane;  // the wave's first category
    if (lane == 0 && cat0 < w) {
      bits[cat0 >> 5] = (uint32_t)right;
      if (cat0 + 32 < w) bits[(cat0 >> 5) + 1] = (uint32_t)(right >> 32);
    }
  }
}

// Per node, after gbt_select_best: the best wide slot (ties: the lower
// slot, i.e. the lower feature) replaces the node's record only with a
// STRICTLY greater gain, which is the host rule "numeric and one-hot
// first, then the wide features in ascending order, each with `>`".  The
// winner's bitset goes to out_bits[node].  One wave per node.
__global__ __launch_bounds__(64) void MergeCatKernel(
    const int64_t* __restrict__ rec, const uint32_t* __restrict__ bits,
    const int32_t* __restrict__ wide, int n_wide, int words,
    const int32_t* __restrict__ cut_ptrs, int64_t* __restrict__ out_best,
    uint32_t* __restrict__ out_bits) {
  const int node = blockIdx.x;
  const int lane = threadIdx.x;
  const size_t base = (size_t)node * n_wide;
  double gain = -INFINITY;
  int slot = kNoKey;
  for (int s = lane; s < n_wide; s += 64) {
    const double gv = __longlong_as_double(rec[4 * (base + s)]);
    if (gv > gain) {
      gain = gv;
      slot = s;
    }
  }
  WaveArgmaxKey(&gain, &slot);
  int64_t* ob = out_best + (size_t)node * 6;
  // lane 0 reads the standing record for the wave, then overwrites it
  double cur = -INFINITY;
  if (lane == 0 && ob[1] >= 0) cur = __longlong_as_double(ob[0]);
  cur = __shfl(cur, 0, 64);
  if (slot == kNoKey || !(gain > cur)) return;
  const int f = wide[slot];
  const int b0 = cut_ptrs[f];
  const int nw = (cut_ptrs[f + 1] - b0 + 31) >> 5;
  if (lane == 0) {
    const int64_t* r = rec + 4 * (base + slot);
    ob[0] = r[0];
    ob[1] = b0;
    ob[2] = r[1];
    ob[3] = r[2];
    ob[4] = r[3];
    ob[5] = f;
  }
  for (int v = lane; v < nw; v += 64)
    out_bits[(size_t)node * words + v] = bits[(base + slot) * words + v];
}

// the widest feature gbt_evaluate_cat serves
extern "C" int gbt_evaluate_cat_max_width() { return kCatCap; }

// Evaluates the n_wide listed categorical features (ascending ids, each at
// most gbt_evaluate_cat_max_width() wide) of every node as sorted-partition
// splits and merges them into out_best, which gbt_select_best has filled
// from the other features on the same stream.  tiers: bit 0 = some listed
// feature has at most 64 categories, bit 1 = some has more.  feature_mask
// is the per-node feature set with the wide columns still in it, or null.
// words >= ceil(width / 32) of the widest listed feature.
extern "C" void gbt_evaluate_cat(
    const int64_t* hist, int n_nodes, int n_bins, int n_features,
    const int32_t* cut_ptrs, const int64_t* parent_sums, double g_scale,
    double h_scale, double reg_lambda, double reg_alpha,
    double max_delta_step, double min_child_weight, int max_cat_threshold,
    const int32_t* wide, int n_wide, int tiers, const uint8_t* feature_mask,
    int64_t* slot_rec /* [n_nodes, n_wide, 4] */,
    uint32_t* slot_bits /* [n_nodes, n_wide, words] */, int words,
    int64_t* out_best /* [n_nodes, 6] */,
    uint32_t* out_bits /* [n_nodes, words] */, hipStream_t stream) {
  if (n_nodes <= 0 || n_wide <= 0) return;
  const int max_prefix =
      max_cat_threshold >= kCatCap ? kCatCap : max_cat_threshold + 1;
  const CatArgs ca{hist, n_nodes, n_bins, n_features, cut_ptrs, parent_sums,
                   g_scale, h_scale, reg_lambda, reg_alpha, max_delta_step,
                   min_child_weight, max_prefix, wide, n_wide, feature_mask,
                   slot_rec, slot_bits, words};
  if (tiers & 1) {
    const long long items = (long long)n_nodes * n_wide;
    hipLaunchKernelGGL(EvaluateCatWaveKernel,
                       dim3((unsigned)((items + kCatWaves - 1) / kCatWaves)),
                       dim3(kCatBlock), 0, stream, ca);
  }
  // grid.y holds 65535 nodes: more go in slices of the node-major arrays
  for (int n0 = 0; (tiers & 2) && n0 < n_nodes; n0 += 65535) {
    CatArgs cs = ca;
    cs.n_nodes = n_nodes - n0 < 65535 ? n_nodes - n0 : 65535;
    cs.hist += (size_t)n0 * n_bins * 2;
    cs.parent_sums += (size_t)n0 * 2;
    if (feature_mask != nullptr) cs.feature_mask += (size_t)n0 * n_features;
    cs.out_rec += (size_t)n0 * n_wide * 4;
    cs.out_bits += (size_t)n0 * n_wide * words;
    hipLaunchKernelGGL(EvaluateCatBlockKernel, dim3(n_wide, cs.n_nodes),
                       dim3(kCatBlock), 0, stream, cs);
  }
  hipLaunchKernelGGL(MergeCatKernel, dim3(n_nodes), dim3(64), 0, stream,
                     slot_rec, slot_bits, wide, n_wide, words, cut_ptrs,
                     out_best, out_bits);
}
