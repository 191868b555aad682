// Multiclass softmax gradients (multi:softmax / multi:softprob) in one
// launch per boosting round: reads the row-major margin [n, K] once and
// writes one contiguous (g, h) plane [n, 2] per class plus the per-class
// max-abs the quantiser scales by.
//
// Reference behavior: SoftmaxMultiClassObj::GetGradient
// (multiclass_obj.cu), in the fp32 operation order of
// SoftmaxMulti.get_gradient:
//   m = max_c x_c, e_c = expf(x_c - m), p_c = e_c / sum e,
//   g_c = p_c - [c == y], h_c = max(2 p_c (1 - p_c), 1e-16), both times w.
//
// The input is row-major and the output class-major, so a thread-per-row
// kernel would store with stride n.  A block therefore owns a tile of R
// rows and transposes through LDS:
//   load     R x K floats with coalesced dword loads into the front of
//            each LDS row (a row is K float2 slots, stride K | 1 slots:
//            odd, so 8-byte accesses of consecutive rows at one class
//            fall in distinct banks);
//   compute  a row belongs to L adjacent lanes of one wave, lane l holding
//            float2 slots l, l + L, ... (2 P classes) in registers; max
//            and sum are xor butterflies over the L lanes; (g, h) go back
//            over the same LDS row as float2 per class.  Every lane's
//            reads of a row come before any lane's writes to it: the
//            writes depend on the butterflies (L > 1), or the row has one
//            owner (L == 1);
//   write    for class c consecutive lanes take consecutive rows and
//            store float2 to plane c: runs of R * 8 contiguous bytes.
// Max-abs: a lane holds the same classes for every row it ever computes,
// so it keeps their running max |g|, |h| in registers; the hot loop has no
// reduction at all.  At block end the lanes that share a class set are
// folded with shuffles, one lane per wave and class set raises a per-block
// LDS max (uint-bits atomicMax, as gpair.hip), and the block issues one
// global atomicMax per class and component.  No float atomics and no
// cross-thread float sums: the output does not depend on the grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxClasses = 256;
// Every block ends with 2 K global atomicMax ops on the same few lines
// (gpair.hip's same-line atomic tail), so the grid is capped and strides.
constexpr int kMaxBlocks = 512;

__device__ inline void AtomicMaxBits(float* addr, float v) {
  // v >= 0: non-negative floats order as their bit patterns
  atomicMax((unsigned int*)addr, __float_as_uint(v));
}

template <int W>
__device__ inline float GroupMax(float v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, W));
  return v;
}

template <int W>
__device__ inline float GroupSum(float v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, W);
  return v;
}

// L lanes per row, P float2 slots (2 P classes) per lane, R rows per tile.
// Serves K <= 2 * L * P.
template <int L, int P, int R>
__global__ __launch_bounds__(kThreads) void SoftmaxGpairKernel(
    const float* __restrict__ margin /* [n, K] */,
    const float* __restrict__ label /* [n] */,
    const float* __restrict__ weight /* [n] or null */, long long n, int K,
    float2* __restrict__ out_gh /* [K][n] */,
    float* __restrict__ out_maxabs /* [K][2], zeroed by the caller */) {
  constexpr int kRowsPerPass = kThreads / L;
  static_assert(R % kRowsPerPass == 0, "a tile is whole passes");
  static_assert((R & (R - 1)) == 0 && R >= 16, "R: power of two, >= 16");
  static_assert(L == 1 || L == 4 || L == 16 || L == 64, "L within a wave");
  extern __shared__ float2 tile[];  // [R][S2], then block max [K]
  const int S2 = K | 1;
  float2* bmax = tile + R * S2;
  const int tid = (int)threadIdx.x;
  for (int c = tid; c < K; c += kThreads) bmax[c] = make_float2(0.f, 0.f);
  // (the first barrier of the tile loop orders this before any use; a
  // block always has at least one tile)

  const int lg = tid % L;   // lane within the row's group
  const int grp = tid / L;  // row within a pass
  float mg[2 * P], mh[2 * P];
#pragma unroll
  for (int i = 0; i < 2 * P; ++i) mg[i] = mh[i] = 0.f;

  // loader: flat element f = tid + 256 q of the tile is (row, class) =
  // (f / K, f % K); stepping f by 256 steps the pair without a division
  const int dr = kThreads / K, dc = kThreads % K;
  const int r0 = tid / K, c0 = tid % K;
  float* tf = (float*)tile;

  const long long n_tiles = (n + R - 1) / R;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long row0 = t * R;
    const int rows = n - row0 < R ? (int)(n - row0) : R;
    const int cnt = rows * K;
    const float* __restrict__ src = margin + row0 * K;
    {
      int r = r0, c = c0;
#pragma unroll 4
      for (int f = tid; f < cnt; f += kThreads) {
        tf[r * 2 * S2 + c] = src[f];
        c += dc;
        r += dr;
        if (c >= K) {
          c -= K;
          ++r;
        }
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int rp = grp; rp < R; rp += kRowsPerPass) {
      // rows past the tail compute on stale LDS and are never stored
      const bool live = rp < rows;
      float2* rowp = tile + rp * S2;
      float x[2 * P];
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int j = lg + i * L;
        float2 v = make_float2(-INFINITY, -INFINITY);
        if (2 * j < K) v = rowp[j];
        if (2 * j + 1 >= K) v.y = -INFINITY;  // slot past the last class
        x[2 * i] = v.x;
        x[2 * i + 1] = v.y;
        m = fmaxf(m, fmaxf(v.x, v.y));
      }
      m = GroupMax<L>(m);
      // the lane's 2 P terms are summed pairwise, like the butterfly that
      // follows: log2(2 P L) roundings on every path instead of a chain
      // of 2 P - 1 (max abs error of g against fp64 at K = 16, 515 rows:
      // 3.1e-7 with a running sum, 1.7e-7 pairwise, the torch chain's
      // figure; profiles/multiclass_mi355x.md)
      float part[2 * P];
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) {
        x[i] = expf(x[i] - m);  // classes past K: expf(-inf) = 0
        part[i] = x[i];
      }
#pragma unroll
      for (int half = P; half > 0; half >>= 1) {
#pragma unroll
        for (int i = 0; i < half; ++i) part[i] += part[i + half];
      }
      const float s = GroupSum<L>(part[0]);
      float y = -1.f, w = 1.f;
      if (live) {
        y = label[row0 + rp];
        if (weight != nullptr) w = weight[row0 + rp];
      }
      // target class as the generic path's .long() truncation gives it;
      // out of range or not finite: no class is the target
      const int yc = (y > -1.f && y < (float)K) ? (int)y : -1;
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) {
        const int c = 2 * (lg + (i >> 1) * L) + (i & 1);
        if (c < K) {
          const float p = x[i] / s;
          const float g = (c == yc ? p - 1.0f : p) * w;
          const float h = fmaxf(2.0f * p * (1.0f - p), 1e-16f) * w;
          rowp[c] = make_float2(g, h);
          if (live) {
            mg[i] = fmaxf(mg[i], fabsf(g));
            mh[i] = fmaxf(mh[i], fabsf(h));
          }
        }
      }
    }
    __syncthreads();

    for (int idx = tid; idx < R * K; idx += kThreads) {
      const int c = idx / R, r = idx % R;  // R is a power of two
      if (r < rows) out_gh[(long long)c * n + row0 + r] = tile[r * S2 + c];
    }
    __syncthreads();
  }

  // fold the lanes of a wave that hold the same classes (same lane % L)
#pragma unroll
  for (int i = 0; i < 2 * P; ++i) {
#pragma unroll
    for (int off = 32; off >= L; off >>= 1) {
      mg[i] = fmaxf(mg[i], __shfl_xor(mg[i], off, 64));
      mh[i] = fmaxf(mh[i], __shfl_xor(mh[i], off, 64));
    }
    const int c = 2 * (lg + (i >> 1) * L) + (i & 1);
    if ((tid & 63) < L && c < K) {
      AtomicMaxBits(&bmax[c].x, mg[i]);
      AtomicMaxBits(&bmax[c].y, mh[i]);
    }
  }
  __syncthreads();
  for (int c = tid; c < K; c += kThreads) {
    AtomicMaxBits(&out_maxabs[2 * c], bmax[c].x);
    AtomicMaxBits(&out_maxabs[2 * c + 1], bmax[c].y);
  }
}

template <int L, int P, int R>
int Launch(const float* margin, const float* label, const float* weight,
           long long n, int K, float* out_gh, float* out_maxabs,
           hipStream_t stream) {
  if (K > 2 * L * P) return -1;
  const long long n_tiles = (n + R - 1) / R;
  const int blocks = (int)std::min<long long>(n_tiles, kMaxBlocks);
  const size_t lds = ((size_t)R * (K | 1) + K) * sizeof(float2);
  hipLaunchKernelGGL((SoftmaxGpairKernel<L, P, R>), dim3(blocks),
                     dim3(kThreads), lds, stream, margin, label, weight, n, K,
                     (float2*)out_gh, out_maxabs);
  return 0;
}

}  // namespace

extern "C" {

int gbt_softmax_gpair_max_classes() { return kMaxClasses; }

// Block shapes (lanes per row L, classes per lane 2 P, rows per tile R);
// every tile is at most 35 KB of LDS, so four blocks share a CU.  The even
// ids are the defaults of the three K tiers, the odd ids the alternatives
// benchmarks/multiclass_bench.py times against them
// (profiles/multiclass_mi355x.md).
//   0: L 1,  16 classes per lane, R 256   K <= 16
//   1: L 4,   4 classes per lane, R 256   K <= 16
//   2: L 4,  16 classes per lane, R 64    K <= 64
//   3: L 16,  4 classes per lane, R 64    K <= 64
//   4: L 16, 16 classes per lane, R 16    K <= 256
//   5: L 64,  4 classes per lane, R 16    K <= 256
// shape < 0 picks the default of K's tier.  Returns 0, or -1 when the
// shape does not serve K (nothing is launched).
int gbt_softmax_gpair_shaped(int shape, const float* margin,
                             const float* label, const float* weight,
                             long long n, int K, float* out_gh,
                             float* out_maxabs, hipStream_t stream) {
  if (K < 2 || K > kMaxClasses || n < 0) return -1;
  if (n == 0) return 0;
  if (shape < 0) shape = K <= 16 ? 0 : K <= 64 ? 2 : 4;
#define GBT_SOFTMAX_SHAPE(id, L, P, R)                                      \
  case id:                                                                  \
    return Launch<L, P, R>(margin, label, weight, n, K, out_gh, out_maxabs, \
                           stream);
  switch (shape) {
    GBT_SOFTMAX_SHAPE(0, 1, 8, 256)
    GBT_SOFTMAX_SHAPE(1, 4, 2, 256)
    GBT_SOFTMAX_SHAPE(2, 4, 8, 64)
    GBT_SOFTMAX_SHAPE(3, 16, 2, 64)
    GBT_SOFTMAX_SHAPE(4, 16, 8, 16)
    GBT_SOFTMAX_SHAPE(5, 64, 2, 16)
  }
#undef GBT_SOFTMAX_SHAPE
  return -1;
}

// margin [n, K] row-major, label [n], weight [n] or null -> out_gh
// [K][n][2], out_maxabs [K][2] (zeroed by the caller).  2 <= K <=
// gbt_softmax_gpair_max_classes(); a label outside [0, K) or not finite
// makes no class the target.
int gbt_softmax_gpair(const float* margin, const float* label,
                      const float* weight, long long n, int K, float* out_gh,
                      float* out_maxabs, hipStream_t stream) {
  return gbt_softmax_gpair_shaped(-1, margin, label, weight, n, K, out_gh,
                                  out_maxabs, stream);
}

}  // extern "C"
