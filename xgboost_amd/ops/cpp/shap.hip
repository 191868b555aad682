// TreeSHAP contributions on CDNA4.
//
// Reference behavior: src/predictor/interpretability/shap.cu (the
// reference uses a quadrature formulation; we implement the classic
// path-dependent TreeSHAP recursion — same exact outputs — in an
// iterative DFS with per-tree-depth path slices).  One thread per row,
// looping over trees; the path arena lives in scratch (~2 KB/thread at
// depth 10), phi accumulates in a per-thread register/scratch array.
//
// fp64 math matches the CPU oracle (xgboost_amd/shap.py) closely; the
// output is float32 like the reference predictor.
#include "gbt_kernels.h"

namespace {

constexpr int kMaxDepth = 16;    // tree depth cap for the arena
constexpr int kMaxPath = kMaxDepth + 2;
constexpr int kMaxPhi = 129;     // features + bias cap for local phi

struct PathEl {
  int f;
  double zero, one, pw;
};

__device__ inline void ExtendPath(PathEl* path, int& len, double zero,
                                  double one, int fi) {
  path[len].f = fi;
  path[len].zero = zero;
  path[len].one = one;
  path[len].pw = (len == 0) ? 1.0 : 0.0;
  for (int i = len - 1; i >= 0; --i) {
    path[i + 1].pw += one * path[i].pw * (i + 1) / (double)(len + 1);
    path[i].pw = zero * path[i].pw * (len - i) / (double)(len + 1);
  }
  ++len;
}

__device__ inline void UnwindPath(PathEl* path, int& len, int idx) {
  const int d = len - 1;
  const double one = path[idx].one;
  const double zero = path[idx].zero;
  double n = path[d].pw;
  for (int j = d - 1; j >= 0; --j) {
    if (one != 0.0) {
      const double t = path[j].pw;
      path[j].pw = n * (d + 1) / ((j + 1) * one);
      n = t - path[j].pw * zero * (d - j) / (double)(d + 1);
    } else {
      path[j].pw = path[j].pw * (d + 1) / (zero * (d - j));
    }
  }
  for (int j = idx; j < d; ++j) {
    path[j].f = path[j + 1].f;
    path[j].zero = path[j + 1].zero;
    path[j].one = path[j + 1].one;
  }
  --len;
}

__device__ inline double UnwoundSum(const PathEl* path, int len, int idx) {
  const int d = len - 1;
  const double one = path[idx].one;
  const double zero = path[idx].zero;
  double total = 0.0;
  double n = path[d].pw;
  for (int j = d - 1; j >= 0; --j) {
    if (one != 0.0) {
      const double t = n * (d + 1) / ((j + 1) * one);
      total += t;
      n = path[j].pw - t * zero * (d - j) / (double)(d + 1);
    } else {
      total += path[j].pw / (zero * (d - j) / (double)(d + 1));
    }
  }
  return total;
}

struct Frame {
  int node;
  int depth;       // arena slice index
  int parent_len;
  int pfeat;
  float zero, one; // parent fractions (float saves stack space)
};

__global__ __launch_bounds__(128) void ShapKernel(
    const float* __restrict__ X, int64_t n_rows, int n_features,
    float missing_value, int missing_is_nan,
    const int32_t* __restrict__ tree_offsets,
    const int32_t* __restrict__ left, const int32_t* __restrict__ right,
    const int32_t* __restrict__ split_index,
    const float* __restrict__ split_cond,
    const uint8_t* __restrict__ default_left,
    const uint8_t* __restrict__ split_type,
    const int32_t* __restrict__ cat_offsets,
    const uint32_t* __restrict__ cat_bits,
    const float* __restrict__ sum_hess,
    const int32_t* __restrict__ tree_group, int n_trees, int n_groups,
    int n_out_cols,  // n_features + 1
    const double* __restrict__ tree_expected,  // [n_trees]
    float* __restrict__ out_phi /* [n_rows, n_groups, n_out_cols] */) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const float* xrow = X + row * n_features;

  double phi[kMaxPhi];
  PathEl arena[kMaxDepth + 1][kMaxPath];
  Frame stack[2 * kMaxDepth + 4];

  for (int grp = 0; grp < n_groups; ++grp) {
    for (int i = 0; i < n_out_cols; ++i) phi[i] = 0.0;
    for (int t = 0; t < n_trees; ++t) {
      if (tree_group[t] != grp) continue;
      const int base = tree_offsets[t];
      phi[n_out_cols - 1] += tree_expected[t];
      int sp = 0;
      stack[sp++] = Frame{0, 0, 0, -1, 1.0f, 1.0f};
      while (sp > 0) {
        const Frame fr = stack[--sp];
        PathEl* path = arena[fr.depth];
        // copy parent slice
        if (fr.depth > 0) {
          const PathEl* parent = arena[fr.depth - 1];
          for (int i = 0; i < fr.parent_len; ++i) path[i] = parent[i];
        }
        int len = fr.parent_len;
        ExtendPath(path, len, fr.zero, fr.one, fr.pfeat);
        const int n = base + fr.node;
        if (left[n] == -1) {  // leaf
          const double leaf = split_cond[n];
          for (int i = 1; i < len; ++i) {
            const double w = UnwoundSum(path, len, i);
            phi[path[i].f] += w * (path[i].one - path[i].zero) * leaf;
          }
          continue;
        }
        // decision
        const int f = split_index[n];
        const float v = xrow[f];
        const bool missing =
            missing_is_nan ? isnan(v) : (v == missing_value || isnan(v));
        int hot, cold;
        const int l = left[n], r = right[n];
        if (missing) {
          hot = default_left[n] ? l : r;
        } else if (split_type[n] != 0) {
          const int c = (int)v;
          const int w0 = cat_offsets[n];
          const int nw = cat_offsets[n + 1] - w0;
          bool in_set = false;
          if (c >= 0 && (c >> 5) < nw) {
            in_set = (cat_bits[w0 + (c >> 5)] >> (c & 31)) & 1u;
          }
          hot = in_set ? r : l;
        } else {
          hot = (v < split_cond[n]) ? l : r;
        }
        cold = (hot == l) ? r : l;
        const double cover = fmax((double)sum_hess[n], 1e-16);
        const double hot_zero = sum_hess[base + hot] / cover;
        const double cold_zero = sum_hess[base + cold] / cover;
        double iz = 1.0, io = 1.0;
        int idx = -1;
        for (int i = 1; i < len; ++i) {
          if (path[i].f == f) {
            idx = i;
            break;
          }
        }
        if (idx >= 0) {
          iz = path[idx].zero;
          io = path[idx].one;
          UnwindPath(path, len, idx);
        }
        if (fr.depth + 1 <= kMaxDepth) {
          // an element with zero == one == 0 (a child without cover that
          // the row does not enter) zeroes every weight below it, and
          // UnwoundSum would divide by it: prune the branch, like the
          // host recursion
          const float cz = (float)(iz * cold_zero);
          const float hz = (float)(iz * hot_zero);
          const float ho = (float)io;
          if (cz != 0.0f) {
            stack[sp++] = Frame{cold, fr.depth + 1, len, f, cz, 0.0f};
          }
          if (hz != 0.0f || ho != 0.0f) {
            stack[sp++] = Frame{hot, fr.depth + 1, len, f, hz, ho};
          }
        }
      }
    }
    float* out = out_phi + (row * n_groups + grp) * n_out_cols;
    for (int i = 0; i < n_out_cols; ++i) {
      out[i] += (float)phi[i];
    }
  }
}

}  // namespace

extern "C" void gbt_shap(
    const float* X, int64_t n_rows, int n_features, float missing_value,
    int missing_is_nan, const int32_t* tree_offsets, const int32_t* left,
    const int32_t* right, const int32_t* split_index, const float* split_cond,
    const uint8_t* default_left, const uint8_t* split_type,
    const int32_t* cat_offsets, const uint32_t* cat_bits,
    const float* sum_hess, const int32_t* tree_group, int n_trees,
    int n_groups, int n_out_cols, const double* tree_expected,
    float* out_phi, hipStream_t stream) {
  const int64_t blocks = (n_rows + 127) / 128;
  hipLaunchKernelGGL(ShapKernel, dim3((uint32_t)blocks), dim3(128), 0, stream,
                     X, n_rows, n_features, missing_value, missing_is_nan,
                     tree_offsets, left, right, split_index, split_cond,
                     default_left, split_type, cat_offsets, cat_bits,
                     sum_hess, tree_group, n_trees, n_groups, n_out_cols,
                     tree_expected, out_phi);
}
