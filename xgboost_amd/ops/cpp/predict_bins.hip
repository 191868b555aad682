// Forest prediction from quantized pages, raw floats, and vector leaves.
//
// Reference behavior: src/predictor/gpu_predictor.cu (EllpackLoader +
// PredictKernel / PredictLeafKernel, multi-target leaf vectors).  MI355X
// re-design: one thread per row, 256-thread blocks, grid-stride over
// rows.  Every node is one 16-byte record, so a visit is a single
// dwordx4 load instead of the five scattered loads of predict.hip; a
// u8 page row of 28 features is 28 bytes, so the row stays in L1 while
// the thread walks the whole forest.
//
// Input kinds (row-major [n, F]):
//   float     raw values, missing = NaN (or == missing_value)
//   uint8_t   local bin ids, missing iff local >= n_bins[f]
//   uint16_t  same, stored by torch as int16
// Bin rule (tree_model.py RegTree.predict_leaf_bins): numeric node goes
// left iff local <= split_bin, categorical node uses the local bin as
// the category; category in the stored set goes RIGHT.
//
// Leaves: tree_group[t] >= 0 adds the scalar leaf to that column,
// tree_group[t] == -1 adds the K-vector at leaf_vec[(vec_offset[t] +
// nid) * K].  For every (row, k) the adds happen in tree order with
// plain fp32 adds, so the result is bit-identical to the host loops.
// The walk itself is predict_walk.h (shared with predict_csr.hip); this
// file supplies the dense row loaders.
#include "gbt_kernels.h"
#include "predict_walk.h"

#include <algorithm>
#include <type_traits>

namespace {

using gbt_walk::kDefaultGridCap;
using gbt_walk::WalkForest;

// One dense row of raw floats.
struct RawRow {
  using Value = float;
  const float* x;
  float missing_value;
  int missing_is_nan;
  __device__ bool Get(int f, float* v) const {
    *v = x[f];
    return !(missing_is_nan ? isnan(*v)
                            : (*v == missing_value || isnan(*v)));
  }
  __device__ static int Category(float v) { return (int)v; }
  __device__ static bool Less(float v, int w) {
    return v < __int_as_float(w);
  }
};

// One dense row of local bin ids (u8 / u16).
template <typename T>
struct BinRow {
  using Value = uint32_t;
  const T* x;
  const int32_t* n_bins;
  __device__ bool Get(int f, uint32_t* v) const {
    *v = (uint32_t)x[f];
    return *v < (uint32_t)n_bins[f];
  }
  __device__ static int Category(uint32_t v) { return (int)v; }
  __device__ static bool Less(uint32_t v, int w) { return v <= (uint32_t)w; }
};

template <typename T, int KMAX>
__global__ __launch_bounds__(256) void PredictQKernel(
    const T* __restrict__ X, int64_t n_rows, int n_features,
    float missing_value, int missing_is_nan,
    const int32_t* __restrict__ n_bins, const int4* __restrict__ nodes,
    const int32_t* __restrict__ tree_offsets,
    const int32_t* __restrict__ cat_offsets,
    const uint32_t* __restrict__ cat_bits,
    const int32_t* __restrict__ tree_group,
    const int32_t* __restrict__ vec_offset,
    const float* __restrict__ leaf_vec, int n_trees, int n_groups,
    float* __restrict__ out_margin, int32_t* __restrict__ out_leaf) {
  const int64_t row0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t row = row0; row < n_rows;
       row += (int64_t)gridDim.x * blockDim.x) {
    const T* xrow = X + row * n_features;
    if constexpr (std::is_same<T, float>::value) {
      const RawRow rd{xrow, missing_value, missing_is_nan};
      WalkForest<KMAX>(rd, row, nodes, tree_offsets, cat_offsets, cat_bits,
                       tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                       out_margin, out_leaf);
    } else {
      const BinRow<T> rd{xrow, n_bins};
      WalkForest<KMAX>(rd, row, nodes, tree_offsets, cat_offsets, cat_bits,
                       tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                       out_margin, out_leaf);
    }
  }
}

template <typename T>
void Launch(const void* X, int64_t n_rows, int n_features,
            float missing_value, int missing_is_nan, const int32_t* n_bins,
            const void* nodes, const int32_t* tree_offsets,
            const int32_t* cat_offsets, const uint32_t* cat_bits,
            const int32_t* tree_group, const int32_t* vec_offset,
            const float* leaf_vec, int n_trees, int n_groups,
            float* out_margin, int32_t* out_leaf, hipStream_t stream) {
  const int64_t blocks64 = (n_rows + 255) / 256;
  const dim3 grid((unsigned)std::min<int64_t>(blocks64, kDefaultGridCap));
  const dim3 block(256);
  const T* Xt = static_cast<const T*>(X);
  const int4* nd = static_cast<const int4*>(nodes);
#define GBT_PREDICT_Q_LAUNCH(K)                                             \
  hipLaunchKernelGGL((PredictQKernel<T, K>), grid, block, 0, stream, Xt,    \
                     n_rows, n_features, missing_value, missing_is_nan,     \
                     n_bins, nd, tree_offsets, cat_offsets, cat_bits,       \
                     tree_group, vec_offset, leaf_vec, n_trees, n_groups,   \
                     out_margin, out_leaf)
  if (n_groups == 1) {
    GBT_PREDICT_Q_LAUNCH(1);
  } else if (n_groups <= 4) {
    GBT_PREDICT_Q_LAUNCH(4);
  } else {
    GBT_PREDICT_Q_LAUNCH(0);
  }
#undef GBT_PREDICT_Q_LAUNCH
}

}  // namespace

// kind: 0 = float raw values, 1 = uint8 local bins, 2 = uint16 local bins
extern "C" void gbt_predict_q(
    const void* X, int kind, int64_t n_rows, int n_features,
    float missing_value, int missing_is_nan, const int32_t* n_bins,
    const void* nodes, const int32_t* tree_offsets,
    const int32_t* cat_offsets, const uint32_t* cat_bits,
    const int32_t* tree_group, const int32_t* vec_offset,
    const float* leaf_vec, int n_trees, int n_groups, float* out_margin,
    int32_t* out_leaf, hipStream_t stream) {
  if (n_rows <= 0 || n_trees <= 0) {
    return;
  }
  if (kind == 0) {
    Launch<float>(X, n_rows, n_features, missing_value, missing_is_nan,
                  n_bins, nodes, tree_offsets, cat_offsets, cat_bits,
                  tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                  out_margin, out_leaf, stream);
  } else if (kind == 1) {
    Launch<uint8_t>(X, n_rows, n_features, missing_value, missing_is_nan,
                    n_bins, nodes, tree_offsets, cat_offsets, cat_bits,
                    tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                    out_margin, out_leaf, stream);
  } else {
    Launch<uint16_t>(X, n_rows, n_features, missing_value, missing_is_nan,
                     n_bins, nodes, tree_offsets, cat_offsets, cat_bits,
                     tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                     out_margin, out_leaf, stream);
  }
}
