// Gradient-based (minimal variance) row sampling on the device.
//
// Reference behavior: GradientBasedSampling (gpu_hist/sampler.cu).  The
// score of row i is s_i = sqrtf(g_i^2 + lambda * h_i^2) in fp32, the
// threshold u solves  sum_i min(1, s_i / u) = T  with T = subsample * n,
// row i is kept with probability kp_i = min(1, s_i / u) and a kept row is
// scaled by 1 / kp_i.  The reference sorts the scores; here u is found by
// a radix select and nothing is sorted or read back.
//
// Between two neighbouring scores the equation is linear:
//     u = S_lt / (T - C_ge)
// with C_ge the count of rows with s_i >= u and S_lt the sum of the scores
// below u, so all that is needed is where u falls among the scores.
// Non-negative floats order like their bit patterns.  Three histogram
// passes over the 31 value bits (digits of 11 + 10 + 10 bits) narrow the
// position down to one float: each pass builds a table of (count,
// significand sum) per digit value for the rows whose leading digits match
// the prefix found so far, and Select() picks the digit whose lower edge e
// is the last with  f(e) = C_ge(e) + S_lt(e) / e >= T.  f is continuous and
// falling, so a choice that rounding pushes into the neighbouring digit
// moves u by no more than that rounding.  A selected digit may be empty:
// the root then lies in a gap between scores, the later tables stay empty
// and the closed form holds from the carried context alone.
//
// Exact, order-free sums.  The first digit covers the whole exponent, so
// all rows of a bin, and of every sub-bin after it, share their exponent
// and the u64 sum of their 24-bit significands is their exact sum.  The
// tables are filled with integer atomics only (ds_add_u64 in LDS, one
// global u64 atomic per non-empty bin and block), so they do not depend on
// arrival order; Select() turns them into fp64 in a fixed order, and every
// block of a launch derives the same context from the same table.  The
// threshold is therefore the same bit pattern on every run.
//
// Skewed scores (reg:squarederror early on, two-valued logistic gradients,
// any constant-score input) would serialise a plain LDS histogram on one
// address.  The mitigation is aggregation inside the wave: up to kPeel
// times the lowest pending lane's bin is broadcast, the lanes that share it
// are counted with a ballot, their significands are summed with shuffles
// and one lane issues the two LDS atomics for all of them.  Rows left after
// that go in one by one.  Constant scores cost one round per 64 rows;
// spread-out scores pay four ballots and then behave like a plain
// histogram.  Per-wave sub-tables were not used: four copies of the 32 KB
// first-pass table would hold a CU to one block.
//
// Conventions.
//  * Scores below FLT_MIN count as zero, and a zero score is never kept.
//    (fp32 arithmetic does that by itself: the square root of the smallest
//    subnormal is already above FLT_MIN.)
//  * If at most T rows have a positive score there is no root: every such
//    row is kept with probability 1 and scale 1, and the threshold written
//    is 0.
//  * The threshold is taken over the rows given, i.e. per rank.
//  * Gradients are assumed finite.
//
// Scratch: three tables and two contexts (gbt_mvs_sample_scratch_bytes()).
// The first table must be zero when the first launch starts.  The caller
// zeroes the scratch once, when allocating it; every call leaves it zeroed
// again (the first launch clears tables 2 and 3, which it does not use, the
// last clears table 1, which it no longer reads).  Four launches per call.
#include "gbt_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 512;
constexpr int kBins1 = 2048;  // digit 1: value bits 30..20
constexpr int kBins2 = 1024;  // digit 2: bits 19..10, digit 3: bits 9..0
constexpr int kPeel = 4;      // aggregation rounds per wave and row batch

// u64 words of the scratch area: tables of {count, significand sum}
constexpr int kTab1 = 0;
constexpr int kTab2 = kTab1 + 2 * kBins1;
constexpr int kTab3 = kTab2 + 2 * kBins2;
constexpr int kCtx1 = kTab3 + 2 * kBins2;
constexpr int kCtx2 = kCtx1 + 4;
constexpr int kScratchWords = kCtx2 + 4;

// Where the root lies after some digits: `prefix` holds the digits chosen
// so far in their bit positions, `above` counts the rows whose score lies
// above the chosen range, `below` is the sum of the scores under it.  cnt
// and msum are the chosen bin's own table entry.
struct Context {
  u64 above;
  double below;
  unsigned int prefix;
  u64 cnt, msum;
};

__device__ inline float Score(float g, float h, float reg_lambda) {
  // no contraction (the file is built with -ffp-contract=off) and a
  // correctly rounded sqrtf: with h == 0 the score is |g| bit for bit
  const float s = sqrtf(g * g + reg_lambda * (h * h));
  return s < FLT_MIN ? 0.0f : s;
}

// the exact value of a significand sum of rows with biased exponent e
__device__ inline double BinSum(u64 msum, unsigned int e) {
  return ldexp((double)msum, (int)e - 150);
}

// Picks from a table of kBins digit values at bit `shift` the last bin b
// whose lower edge e_b has f(e_b) >= target, i.e.
//     below_b >= (target - above_b - count_b) * e_b,
// and returns the context narrowed to it.  Bin 0 shares its edge with the
// incoming range and always qualifies.  Every thread returns the same
// value; the whole block must call.
template <int kBins>
__device__ Context Select(const u64* table, const Context in, int shift,
                          double target) {
  constexpr int kPer = kBins / kThreads;
  constexpr int kWaves = kThreads / 64;
  __shared__ u64 wave_cnt[kWaves];
  __shared__ double wave_sum[kWaves];
  __shared__ int best;
  __shared__ Context chosen;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) best = 0;

  u64 cnt[kPer], msum[kPer];
  u64 my_cnt = 0;
  double my_sum = 0.0;
  for (int j = 0; j < kPer; ++j) {
    const int b = tid * kPer + j;
    cnt[j] = table[2 * b];
    msum[j] = table[2 * b + 1];
    my_cnt += cnt[j];
    my_sum += BinSum(msum[j], (in.prefix | ((unsigned int)b << shift)) >> 23);
  }
  // inclusive scan over the wave, then over the waves: a fixed tree, so
  // the fp64 sums round the same way in every block and on every run
  u64 inc_cnt = my_cnt;
  double inc_sum = my_sum;
  for (int off = 1; off < 64; off <<= 1) {
    const u64 c = __shfl_up(inc_cnt, off, 64);
    const double s = __shfl_up(inc_sum, off, 64);
    if (lane >= off) {
      inc_cnt += c;
      inc_sum += s;
    }
  }
  if (lane == 63) {
    wave_cnt[wave] = inc_cnt;
    wave_sum[wave] = inc_sum;
  }
  u64 exc_cnt = __shfl_up(inc_cnt, 1, 64);
  double exc_sum = __shfl_up(inc_sum, 1, 64);
  if (lane == 0) {
    exc_cnt = 0;
    exc_sum = 0.0;
  }
  __syncthreads();
  u64 total = 0, base_cnt = 0;
  double base_sum = 0.0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) {
      base_cnt += wave_cnt[w];
      base_sum += wave_sum[w];
    }
    total += wave_cnt[w];
  }
  u64 run_cnt = base_cnt + exc_cnt;           // rows in the bins below b
  double run_sum = in.below + (base_sum + exc_sum);  // scores below bin b
  int mine = -1;
  Context c = in;
  for (int j = 0; j < kPer; ++j) {
    const int b = tid * kPer + j;
    const unsigned int bits = in.prefix | ((unsigned int)b << shift);
    const double edge = (double)__uint_as_float(bits);
    const u64 above = in.above + (total - run_cnt - cnt[j]);
    if (b == 0 ||
        run_sum >= (target - (double)(above + cnt[j])) * edge) {
      mine = b;
      c.above = above;
      c.below = run_sum;
      c.prefix = bits;
      c.cnt = cnt[j];
      c.msum = msum[j];
    }
    run_cnt += cnt[j];
    run_sum += BinSum(msum[j], bits >> 23);
  }
  if (mine > 0) atomicMax(&best, mine);
  __syncthreads();
  if (mine == best) chosen = c;  // one thread: bins are disjoint
  __syncthreads();
  c = chosen;
  __syncthreads();  // the shared cells are reused by the next call
  return c;
}

__device__ inline void StoreContext(u64* w, const Context& c) {
  w[0] = c.above;
  w[1] = (u64)__double_as_longlong(c.below);
  w[2] = c.prefix;
}

__device__ inline Context LoadContext(const u64* w) {
  Context c;
  c.above = w[0];
  c.below = __longlong_as_double((long long)w[1]);
  c.prefix = (unsigned int)w[2];
  c.cnt = 0;
  c.msum = 0;
  return c;
}

// Adds one wave's rows to the LDS table, rows of one bin together (see the
// header).  Called by whole waves; `valid` marks the lanes with a row.
__device__ inline void WaveBinAdd(u64* tab, bool valid, unsigned int bin,
                                  unsigned int sig) {
  const int lane = (int)threadIdx.x & 63;
  u64 todo = __ballot(valid);
  for (int round = 0; round < kPeel && todo != 0; ++round) {
    const int leader = __ffsll(todo) - 1;
    const unsigned int lbin = __shfl(bin, leader, 64);
    const bool same = valid && bin == lbin;
    const u64 m = __ballot(same);
    unsigned int part = same ? sig : 0u;  // <= 64 * 2^24: fits 32 bits
    if (m != (1ull << leader)) {          // wave-uniform
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    }
    if (lane == leader) {
      atomicAdd(&tab[2 * lbin], (u64)__popcll(m));
      if (part) atomicAdd(&tab[2 * lbin + 1], (u64)part);
    }
    if (same) valid = false;
    todo &= ~m;
  }
  if (valid) {
    atomicAdd(&tab[2 * bin], 1ull);
    if (sig) atomicAdd(&tab[2 * bin + 1], (u64)sig);
  }
}

// One histogram pass.  kPass 0 bins every row by digit 1; kPass 1 and 2
// first select on the previous pass's table, then bin the rows under the
// selected prefix by the next digit.
template <int kPass>
__global__ __launch_bounds__(kThreads) void MvsHistKernel(
    const float* __restrict__ gh, long long n, float reg_lambda,
    double target, u64* __restrict__ scratch) {
  constexpr int kBins = kPass == 0 ? kBins1 : kBins2;
  constexpr int kShift = kPass == 0 ? 20 : (kPass == 1 ? 10 : 0);
  __shared__ u64 tab[2 * kBins];
  u64* out = scratch + (kPass == 0 ? kTab1 : (kPass == 1 ? kTab2 : kTab3));
  const int tid = (int)threadIdx.x;

  unsigned int prefix = 0;
  if (kPass == 0) {
    // tables 2 and 3 are idle during this launch: clear them for it
    for (int w = (int)blockIdx.x * kThreads + tid; w < 4 * kBins2;
         w += (int)gridDim.x * kThreads) {
      scratch[kTab2 + w] = 0;
    }
  } else if (kPass == 1) {
    Context zero;
    zero.above = 0;
    zero.below = 0.0;
    zero.prefix = 0;
    zero.cnt = zero.msum = 0;
    const Context c = Select<kBins1>(scratch + kTab1, zero, 20, target);
    if (blockIdx.x == 0 && tid == 0) StoreContext(scratch + kCtx1, c);
    prefix = c.prefix;
  } else {
    const Context c = Select<kBins2>(scratch + kTab2,
                                     LoadContext(scratch + kCtx1), 10, target);
    if (blockIdx.x == 0 && tid == 0) StoreContext(scratch + kCtx2, c);
    prefix = c.prefix;
  }
  for (int w = tid; w < 2 * kBins; w += kThreads) tab[w] = 0;
  __syncthreads();

  // whole waves stay in the loop together: WaveBinAdd is wave-collective
  for (long long base = (long long)blockIdx.x * kThreads; base < n;
       base += (long long)gridDim.x * kThreads) {
    const long long i = base + tid;
    bool valid = i < n;
    unsigned int bits = 0;
    if (valid) {
      const float2 v = reinterpret_cast<const float2*>(gh)[i];
      bits = __float_as_uint(Score(v.x, v.y, reg_lambda));
      if (kPass != 0) valid = (bits >> (kShift + 10)) == (prefix >> (kShift + 10));
    }
    const unsigned int sig = bits ? ((bits & 0x7FFFFFu) | 0x800000u) : 0u;
    WaveBinAdd(tab, valid, (bits >> kShift) & (unsigned int)(kBins - 1), sig);
  }
  __syncthreads();
  for (int b = tid; b < kBins; b += kThreads) {
    const u64 c = tab[2 * b];
    if (c != 0) {
      atomicAdd(&out[2 * b], c);
      if (tab[2 * b + 1]) atomicAdd(&out[2 * b + 1], tab[2 * b + 1]);
    }
  }
}

// Philox4x32-10 (Salmon et al., SC'11) on counter (row, 0) and key seed;
// the first output word.
__device__ inline unsigned int Philox(u64 row, u64 seed) {
  unsigned int c0 = (unsigned int)row, c1 = (unsigned int)(row >> 32);
  unsigned int c2 = 0, c3 = 0;
  unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ inline void AtomicMaxAbsF(float* addr, float v) {
  // floats >= 0 compare as their bit patterns (as in gpair.hip)
  atomicMax((unsigned int*)addr, __float_as_uint(fabsf(v)));
}

// Selects on the third table, forms the threshold and samples.  gh and
// out_gh may be the same array: a thread reads its row before writing it.
__global__ __launch_bounds__(kThreads) void MvsApplyKernel(
    const float* gh, long long n, float reg_lambda, double target, u64 seed,
    const float* __restrict__ rand, u64* __restrict__ scratch, float* out_gh,
    float* __restrict__ out_maxabs, double* __restrict__ out_threshold) {
  __shared__ float smax_g, smax_h;
  const int tid = (int)threadIdx.x;
  if (tid == 0) {
    smax_g = 0.0f;
    smax_h = 0.0f;
  }
  const Context c = Select<kBins2>(scratch + kTab3,
                                   LoadContext(scratch + kCtx2), 0, target);
  // the root lies in [v, next(v)) for the float v = c.prefix: the rows at v
  // are below it, c.above rows are at or above it
  const double rest = target - (double)c.above;
  const double u =
      rest > 0.0 ? (c.below + BinSum(c.msum, c.prefix >> 23)) / rest : 0.0;
  if (blockIdx.x == 0 && tid == 0) *out_threshold = u;
  // table 1 was last read by the second launch: clear it for the next call
  for (int w = (int)blockIdx.x * kThreads + tid; w < 2 * kBins1;
       w += (int)gridDim.x * kThreads) {
    scratch[kTab1 + w] = 0;
  }
  const float uf = (float)u;

  float mg = 0.0f, mh = 0.0f;
  for (long long i = (long long)blockIdx.x * kThreads + tid; i < n;
       i += (long long)gridDim.x * kThreads) {
    const float2 v = reinterpret_cast<const float2*>(gh)[i];
    const float s = Score(v.x, v.y, reg_lambda);
    float kp = 0.0f;
    if (s > 0.0f) kp = u > 0.0 ? fminf(1.0f, s / uf) : 1.0f;
    const float r = rand != nullptr
                        ? rand[i]
                        : (float)(Philox((u64)i, seed) >> 8) * 0x1p-24f;
    float2 o = make_float2(0.0f, 0.0f);
    if (r < kp) {
      const float inv = 1.0f / kp;
      o.x = v.x * inv;
      o.y = v.y * inv;
    }
    reinterpret_cast<float2*>(out_gh)[i] = o;
    mg = fmaxf(mg, fabsf(o.x));
    mh = fmaxf(mh, fabsf(o.y));
  }
  if (out_maxabs == nullptr) return;
  // as GpairKernel: wave shuffle, one LDS atomic per wave, one global
  // atomic pair per block
  for (int off = 32; off > 0; off >>= 1) {
    mg = fmaxf(mg, __shfl_down(mg, off, 64));
    mh = fmaxf(mh, __shfl_down(mh, off, 64));
  }
  if ((tid & 63) == 0) {
    AtomicMaxAbsF(&smax_g, mg);
    AtomicMaxAbsF(&smax_h, mh);
  }
  __syncthreads();
  if (tid == 0) {
    AtomicMaxAbsF(&out_maxabs[0], smax_g);
    AtomicMaxAbsF(&out_maxabs[1], smax_h);
  }
}

}  // namespace

extern "C" {

size_t gbt_mvs_sample_scratch_bytes() { return kScratchWords * sizeof(u64); }

void gbt_mvs_sample(const float* gh, long long n, float reg_lambda,
                    double target_rows, unsigned long long seed,
                    const float* rand, unsigned long long* tables,
                    float* out_gh, float* out_maxabs, double* out_threshold,
                    hipStream_t stream) {
  if (n <= 0) return;
  // few blocks, grid-stride: the table flushes and the max-abs tail are
  // same-line global atomics, as in gbt_gpair_fused
  const int blocks = (int)std::min<long long>((n + kThreads - 1) / kThreads,
                                              kMaxBlocks);
  hipLaunchKernelGGL((MvsHistKernel<0>), dim3(blocks), dim3(kThreads), 0,
                     stream, gh, n, reg_lambda, target_rows, tables);
  hipLaunchKernelGGL((MvsHistKernel<1>), dim3(blocks), dim3(kThreads), 0,
                     stream, gh, n, reg_lambda, target_rows, tables);
  hipLaunchKernelGGL((MvsHistKernel<2>), dim3(blocks), dim3(kThreads), 0,
                     stream, gh, n, reg_lambda, target_rows, tables);
  hipLaunchKernelGGL(MvsApplyKernel, dim3(blocks), dim3(kThreads), 0, stream,
                     gh, n, reg_lambda, target_rows, seed, rand, tables,
                     out_gh, out_maxabs, out_threshold);
}

}  // extern "C"
