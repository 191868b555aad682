// Fused gradient computation + fixed-point quantization for the hot
// objectives (binary:logistic, reg:squarederror).
//
// Reference behavior: objective .cu kernels (elementwise_objective.cuh)
// + GradientQuantiser (quantiser.cuh).  Fusing the elementwise chain
// and the max-abs reduction removes ~9 torch launches and one extra
// D2H sync per boosting round (the scale readback remains — it is also
// the distributed allreduce point).
#include "gbt_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace {

__device__ inline void AtomicMaxAbsF(float* addr, float v) {
  // monotonic max of |v| via uint bit pattern (floats >= 0 compare as uints)
  const unsigned int bits = __float_as_uint(fabsf(v));
  atomicMax((unsigned int*)addr, bits);
}

template <int kObj>  // 0 = logistic, 1 = squarederror
__global__ __launch_bounds__(256) void GpairKernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight, float scale_pos_weight, long long n,
    float* __restrict__ out_gh /* [n,2] */,
    float* __restrict__ out_maxabs /* [2] */) {
  __shared__ float smax_g, smax_h;
  if (threadIdx.x == 0) {
    smax_g = 0.0f;
    smax_h = 0.0f;
  }
  __syncthreads();
  float mg = 0.0f, mh = 0.0f;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float y = label[i];
    float g, h;
    if (kObj == 0) {
      const float p = 1.0f / (1.0f + expf(-margin[i]));
      g = p - y;
      h = fmaxf(p * (1.0f - p), 1e-16f);
      if (scale_pos_weight != 1.0f && y == 1.0f) {
        g *= scale_pos_weight;
        h *= scale_pos_weight;
      }
    } else {
      g = margin[i] - y;
      h = 1.0f;
    }
    if (weight != nullptr) {
      g *= weight[i];
      h *= weight[i];
    }
    out_gh[2 * i] = g;
    out_gh[2 * i + 1] = h;
    mg = fmaxf(mg, fabsf(g));
    mh = fmaxf(mh, fabsf(h));
  }
  // wave-reduce before touching LDS: 256 same-address LDS atomics per
  // block serialize (~90 us/launch measured); 4 do not
  for (int off = 32; off > 0; off >>= 1) {
    mg = fmaxf(mg, __shfl_down(mg, off, 64));
    mh = fmaxf(mh, __shfl_down(mh, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    AtomicMaxAbsF(&smax_g, mg);
    AtomicMaxAbsF(&smax_h, mh);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    AtomicMaxAbsF(&out_maxabs[0], smax_g);
    AtomicMaxAbsF(&out_maxabs[1], smax_h);
  }
}

// One [n, 2] plane, strided over by the blocks of grid dimension x: the
// body of both quantise kernels below.
__device__ inline void QuantizePlane(
    const float* __restrict__ gh, long long n, double g_scale, double h_scale,
    const float* __restrict__ maxabs /* null, or [2]: derive the scales
        here so the host never has to read max-abs back */,
    int32_t* __restrict__ out,
    int64_t* __restrict__ out_sums /* null, or [2] zero-initialized:
        exact totals of the quantized pairs (the tree driver's root
        sums), accumulated here instead of a separate 16 MB int64
        materialization + reduction */) {
  if (maxabs != nullptr) {
    g_scale = maxabs[0] > 0.f ? 1073741824.0 / (double)maxabs[0] : 1.0;
    h_scale = maxabs[1] > 0.f ? 1073741824.0 / (double)maxabs[1] : 1.0;
  }
  long long sg = 0, sh = 0;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n; i += (long long)gridDim.x * blockDim.x) {
    // round-half-to-even (llrint, FE_TONEAREST) matches torch.round
    const int32_t qg = (int32_t)llrint((double)gh[2 * i] * g_scale);
    const int32_t qh = (int32_t)llrint((double)gh[2 * i + 1] * h_scale);
    out[2 * i] = qg;
    out[2 * i + 1] = qh;
    sg += qg;
    sh += qh;
  }
  if (out_sums != nullptr) {
    for (int off = 32; off > 0; off >>= 1) {
      sg += __shfl_down(sg, off, 64);
      sh += __shfl_down(sh, off, 64);
    }
    __shared__ long long wg[256 / 64], wh[256 / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if (lane == 0) {
      wg[wave] = sg;
      wh[wave] = sh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long tg = 0, th = 0;
      for (int w = 0; w < (int)blockDim.x / 64; ++w) {
        tg += wg[w];
        th += wh[w];
      }
      if (tg) atomicAdd((unsigned long long*)&out_sums[0],
                        (unsigned long long)tg);
      if (th) atomicAdd((unsigned long long*)&out_sums[1],
                        (unsigned long long)th);
    }
  }
}

__global__ __launch_bounds__(256) void QuantizeKernel(
    const float* __restrict__ gh, long long n, double g_scale, double h_scale,
    const float* __restrict__ maxabs, int32_t* __restrict__ out,
    int64_t* __restrict__ out_sums) {
  QuantizePlane(gh, n, g_scale, h_scale, maxabs, out, out_sums);
}

// K planes in one launch, blockIdx.y the plane: plane k scales by its own
// maxabs[k] and accumulates its own out_sums[k].
__global__ __launch_bounds__(256) void QuantizePlanesKernel(
    const float* __restrict__ gh /* [K][n][2] */, long long n,
    const float* __restrict__ maxabs /* [K][2] */,
    int32_t* __restrict__ out /* [K][n][2] */,
    int64_t* __restrict__ out_sums /* [K][2] zero-initialized */) {
  const long long k = blockIdx.y;
  QuantizePlane(gh + 2 * k * n, n, 0.0, 0.0, maxabs + 2 * k,
                out + 2 * k * n, out_sums + 2 * k);
}

}  // namespace

extern "C" {

void gbt_gpair_fused(int objective, const float* margin, const float* label,
                     const float* weight, float scale_pos_weight, long long n,
                     float* out_gh, float* out_maxabs, hipStream_t stream) {
  // few blocks, grid-stride: every block ends with 2 same-line global
  // atomicMax ops — thousands of blocks serialize on that L2 line
  // (~90 us measured); 512 blocks stream 1M rows just as fast and cut
  // the atomic tail to noise
  const int blocks = (int)std::min<long long>((n + 255) / 256, 512);
  if (objective == 0) {
    hipLaunchKernelGGL((GpairKernel<0>), dim3(blocks), dim3(256), 0, stream,
                       margin, label, weight, scale_pos_weight, n, out_gh,
                       out_maxabs);
  } else {
    hipLaunchKernelGGL((GpairKernel<1>), dim3(blocks), dim3(256), 0, stream,
                       margin, label, weight, scale_pos_weight, n, out_gh,
                       out_maxabs);
  }
}

void gbt_quantize(const float* gh, long long n, double g_scale,
                  double h_scale, const float* maxabs, int32_t* out,
                  int64_t* out_sums, hipStream_t stream) {
  // same-line atomic lesson as the gpair kernel: few blocks
  const int blocks = (int)std::min<long long>((n + 255) / 256, 512);
  hipLaunchKernelGGL(QuantizeKernel, dim3(blocks), dim3(256), 0, stream, gh,
                     n, g_scale, h_scale, maxabs, out, out_sums);
}

// gbt_quantize over K class-major planes (softmax_gpair.hip's output) with
// device-side scales: same rounding, scale formula and exact int64 sums.
void gbt_quantize_planes(const float* gh, long long n, int n_planes,
                         const float* maxabs, int32_t* out, int64_t* out_sums,
                         hipStream_t stream) {
  if (n <= 0 || n_planes <= 0) return;
  // the per-plane atomic tail is gbt_quantize's; the grid as a whole is
  // kept near its size
  const int per = std::max(512 / n_planes, 64);
  const int blocks = (int)std::min<long long>((n + 255) / 256, per);
  hipLaunchKernelGGL(QuantizePlanesKernel, dim3(blocks, n_planes), dim3(256),
                     0, stream, gh, n, maxabs, out, out_sums);
}

}  // extern "C"

namespace {

__global__ __launch_bounds__(256) void MarginAddKernel(
    float* __restrict__ margin, const int32_t* __restrict__ pos,
    const float* __restrict__ leaf_vals, long long n, int stride, int col) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n; i += (long long)gridDim.x * blockDim.x) {
    margin[i * stride + col] += leaf_vals[pos[i]];
  }
}

}  // namespace

extern "C" void gbt_margin_add(float* margin, const int32_t* pos,
                               const float* leaf_vals, long long n,
                               int stride, int col, hipStream_t stream) {
  const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(MarginAddKernel, dim3(blocks), dim3(256), 0, stream,
                     margin, pos, leaf_vals, n, stride, col);
}
