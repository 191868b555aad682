// Saabas contributions (approx_contribs) by walking the forest on the
// device.
//
// Specification: shap._saabas (shap.py).  Every node of a tree has a mean
// value: a leaf its leaf value, an internal node the cover-weighted mean
// of its children,
//
//   mean[n] = (mean[l] * h[l] + mean[r] * h[r]) / max(h[l] + h[r], 1e-16)
//
// in fp64, children before parents (a child's id is above its parent's;
// the host checks that before it launches).  A row walks each tree from
// the root, and every internal node it passes adds
// mean[next] - mean[node] to phi[row, group(tree), feature(node)].
//
// SaabasMeansKernel: one thread per tree, nodes by descending id.  The
// file is compiled without FMA contraction, so the expression rounds as
// numpy rounds it and the means equal the host's bit for bit.
//
// SaabasWalkKernel.  Work split: a block is ONE 64-lane wave that owns a
// tile of 64 rows, and a lane owns one row for the whole kernel.  Only
// that lane ever touches the row's accumulators, so there are no atomics
// and no reduction, and the adds into a cell happen in tree order and
// then path order: the host's order, so the fp64 sums are the host's.
// Nothing is shared between the lanes but the transposed write-out, so a
// larger block would buy nothing; one wave per block keeps a launch of a
// few thousand rows spread over all 256 CUs and makes the two barriers of
// a window wave-local.
//
// Accumulators: fp64 in LDS, [64 rows][window] in the compact space of
// the U columns the forest splits on (slot_of[feature] = slot, used[slot]
// = output column).  The row stride is window | 1 doubles: odd, so the 64
// lanes adding into one column (the usual case near the root) or zeroing
// their rows fall on distinct banks.  LDS budget: a CU has 160 KB and
// four SIMDs; 40 KB a block keeps four blocks resident, which is 64 rows
// x 79 columns (the default window the host passes).  A block may take up
// to 64 KB, 127 columns.  A forest that uses more columns than the window
// holds is walked once per window and keeps only the adds whose slot is
// inside it; the order within a cell does not change.
//
// Groups (one tree per output group) are passed one at a time, so the
// tile is [rows][window] whatever n_groups is, and pass g walks only the
// trees of group g.
//
// Node reads: the packed int4 record of predict_walk.h, one dwordx4 load
// a visit, with mean[] as a parallel fp64 array whose load issues with
// the record's.  WalkForest adds per leaf and does not expose its
// per-node decision, and factoring the decision out of it changed the
// code generated for the predictors, so the header is left as it is and
// the decision is restated here against the header's record constants
// and its loader convention.
//
// Row reads: X[row * row_stride + column * col_stride].  Dense input is
// row-major with column = the node's feature; the CSR route passes the
// staged feature-major tile of shap_csr.hip (row_stride 1, col_stride =
// rows of the tile, NaN = absent) with column = the node's slot.
//
// Write-out: after a window's trees the 64 lanes sweep the tile row by
// row, consecutive lanes on consecutive columns, cast to fp32 and store
// out[row, group, used[slot]]; each such cell belongs to one window of
// one group, so it is stored once.  The bias column takes the host's
// fp64 bias[group] (base margin + the trees' expected values).
#include "gbt_kernels.h"
#include "predict_walk.h"

#include <algorithm>

namespace {

using gbt_walk::kDefaultLeft;
using gbt_walk::kFeatMask;
using gbt_walk::kIsCat;

constexpr int kRows = 64;         // rows of a tile = lanes of the block
constexpr int kMaxWindow = 127;   // 64 * 127 * 8 bytes <= 64 KB
constexpr int kGridCap = 1 << 16;

__global__ __launch_bounds__(64) void SaabasMeansKernel(
    const int4* __restrict__ nodes, const int32_t* __restrict__ tree_offsets,
    const float* __restrict__ sum_hess, int n_trees,
    double* __restrict__ mean_val) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_trees) return;
  const int base = tree_offsets[t];
  const int n = tree_offsets[t + 1] - base;
  for (int nid = n - 1; nid >= 0; --nid) {
    const int4 nd = nodes[base + nid];
    double m;
    if (nd.x == -1) {
      m = (double)__int_as_float(nd.w);
    } else {
      const double hl = (double)sum_hess[base + nd.x];
      const double hr = (double)sum_hess[base + nd.y];
      const double tot = fmax(hl + hr, 1e-16);
      m = (mean_val[base + nd.x] * hl + mean_val[base + nd.y] * hr) / tot;
    }
    mean_val[base + nid] = m;
  }
}

// One row of raw floats behind the loader convention of predict_walk.h.
struct StridedRow {
  const float* x;  // the row's first column
  int64_t col_stride;
  float missing_value;
  int missing_is_nan;
  __device__ bool Get(int col, float* v) const {
    *v = x[col * col_stride];
    return !(missing_is_nan ? isnan(*v)
                            : (*v == missing_value || isnan(*v)));
  }
  __device__ static int Category(float v) { return (int)v; }
  __device__ static bool Less(float v, int w) {
    return v < __int_as_float(w);
  }
};

struct SaabasArgs {
  const float* __restrict__ X;
  int64_t n_rows;
  int64_t row_stride;
  int64_t col_stride;
  float missing_value;
  int missing_is_nan;
  const int4* __restrict__ nodes;
  const int32_t* __restrict__ tree_offsets;
  const int32_t* __restrict__ cat_offsets;
  const uint32_t* __restrict__ cat_bits;
  const int32_t* __restrict__ tree_group;
  const double* __restrict__ mean_val;
  const int32_t* __restrict__ slot_of;  // [n_features] feature -> slot
  const int32_t* __restrict__ used;     // [n_used] slot -> output column
  int n_used;
  int n_trees;
  int n_groups;
  int n_cols;
  int window;
  const double* __restrict__ bias;  // [n_groups]
  float* __restrict__ out;          // [n_rows, n_groups, n_cols]
};

// kCompact: X's columns are slots (the staged CSR tile), not features.
template <bool kCompact>
__global__ __launch_bounds__(kRows) void SaabasWalkKernel(SaabasArgs a) {
  extern __shared__ double acc[];  // [kRows][stride]
  const int lane = threadIdx.x;
  const int stride = a.window | 1;
  double* mine = acc + lane * stride;
  const int64_t n_tiles = (a.n_rows + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    const int64_t row = row0 + lane;
    const bool live = row < a.n_rows;
    const int tile_rows = (int)min((int64_t)kRows, a.n_rows - row0);
    const StridedRow rd{a.X + (live ? row : 0) * a.row_stride, a.col_stride,
                        a.missing_value, a.missing_is_nan};
    for (int g = 0; g < a.n_groups; ++g) {
      float* orow = a.out + (row0 * a.n_groups + g) * a.n_cols;
      if (live) {
        orow[(int64_t)lane * a.n_groups * a.n_cols + a.n_cols - 1] =
            (float)a.bias[g];
      }
      for (int w0 = 0; w0 < a.n_used; w0 += a.window) {
        const int wn = min(a.window, a.n_used - w0);
        for (int c = 0; c < wn; ++c) mine[c] = 0.0;
        for (int t = 0; live && t < a.n_trees; ++t) {
          if (a.tree_group[t] != g) continue;
          const int base = a.tree_offsets[t];
          int nid = 0;
          int4 nd = a.nodes[base];
          double m = a.mean_val[base];
          while (nd.x != -1) {
            const uint32_t fw = (uint32_t)nd.z;
            const int slot = a.slot_of[fw & kFeatMask];
            float v;
            bool go_left;
            if (!rd.Get(kCompact ? slot : (int)(fw & kFeatMask), &v)) {
              go_left = (fw & kDefaultLeft) != 0;
            } else if (fw & kIsCat) {
              const int c = StridedRow::Category(v);
              const int b0 = a.cat_offsets[base + nid];
              const int nw = a.cat_offsets[base + nid + 1] - b0;
              bool in_set = false;
              if (c >= 0 && (c >> 5) < nw) {
                in_set = (a.cat_bits[b0 + (c >> 5)] >> (c & 31)) & 1u;
              }
              go_left = !in_set;  // stored set goes RIGHT
            } else {
              go_left = StridedRow::Less(v, nd.w);
            }
            nid = go_left ? nd.x : nd.y;
            nd = a.nodes[base + nid];
            const double mn = a.mean_val[base + nid];
            const uint32_t c = (uint32_t)(slot - w0);
            if (c < (uint32_t)wn) mine[c] += mn - m;
            m = mn;
          }
        }
        __syncthreads();
        for (int i = lane; i < tile_rows * wn; i += kRows) {
          const int r = i / wn;
          const int c = i - r * wn;
          orow[(int64_t)r * a.n_groups * a.n_cols + a.used[w0 + c]] =
              (float)acc[r * stride + c];
        }
        __syncthreads();
      }
    }
  }
}

}  // namespace

extern "C" void gbt_saabas_means(const void* nodes,
                                 const int32_t* tree_offsets,
                                 const float* sum_hess, int n_trees,
                                 double* mean_val, hipStream_t stream) {
  if (n_trees <= 0) return;
  hipLaunchKernelGGL(SaabasMeansKernel, dim3((n_trees + 63) / 64), dim3(64),
                     0, stream, static_cast<const int4*>(nodes), tree_offsets,
                     sum_hess, n_trees, mean_val);
}

extern "C" int gbt_shap_saabas_rows() { return kRows; }

extern "C" void gbt_shap_saabas(
    const float* X, int64_t n_rows, int64_t row_stride, int64_t col_stride,
    int compact, float missing_value, int missing_is_nan, const void* nodes,
    const int32_t* tree_offsets, const int32_t* cat_offsets,
    const uint32_t* cat_bits, const int32_t* tree_group,
    const double* mean_val, const int32_t* slot_of, const int32_t* used,
    int n_used, int n_trees, int n_groups, int n_cols, int window,
    const double* bias, float* out, hipStream_t stream) {
  if (n_rows <= 0 || n_groups <= 0) return;
  window = std::max(1, std::min(window, std::min(kMaxWindow,
                                                 std::max(n_used, 1))));
  const SaabasArgs a{X, n_rows, row_stride, col_stride, missing_value,
                     missing_is_nan, static_cast<const int4*>(nodes),
                     tree_offsets, cat_offsets, cat_bits, tree_group,
                     mean_val, slot_of, used, n_used, n_trees, n_groups,
                     n_cols, window, bias, out};
  const int64_t n_tiles = (n_rows + kRows - 1) / kRows;
  const dim3 grid((unsigned)std::min<int64_t>(n_tiles, kGridCap));
  const size_t lds = (size_t)kRows * (window | 1) * sizeof(double);
  if (compact) {
    hipLaunchKernelGGL(SaabasWalkKernel<true>, grid, dim3(kRows), lds, stream,
                       a);
  } else {
    hipLaunchKernelGGL(SaabasWalkKernel<false>, grid, dim3(kRows), lds,
                       stream, a);
  }
}
