// Forest prediction from sparse CSR rows.
//
// Reference behavior: src/predictor/gpu_predictor.cu (SparsePageLoader:
// a shared-memory dense row when it fits, otherwise a per-row binary
// search).  MI355X re-design: the forest walk is predict_walk.h, the
// one predict_bins.hip uses, with a CSR row loader in front: one thread
// per row, 256-thread blocks, grid-stride over rows, packed 16-byte
// node records, plain fp32 adds in tree order (bit-identical to the
// host loops).
//
// A feature absent from the row is missing and takes the node's default
// direction; a stored NaN is missing too; a stored 0.0 is a value.
// Column indices are sorted within a row and unique.
//
// Two loaders, chosen on the host:
//   search  lower-bound search of indices[indptr[r] : indptr[r+1]) at
//           every node visit; any n_features.
//   LDS     the row is scattered once into a dense NaN-filled column of
//           a feature-major LDS tile, tile[f * 256 + tid], and the walk
//           reads LDS.  Lanes of a wave read consecutive dwords, so no
//           bank conflicts.  Thread tid fills, scatters into and reads
//           only column tid of the tile, so program order alone orders
//           the three phases: the kernel holds no barrier, and rows past
//           the end simply leave the loop.
// A feature index >= n_features is missing in both.
#include "gbt_kernels.h"
#include "predict_walk.h"

#include <algorithm>

namespace {

using gbt_walk::kDefaultGridCap;
using gbt_walk::WalkForest;

constexpr int kBlock = 256;
// LDS tile budget per block: n_features * 1 KiB must fit.  64 KiB is the
// most a launch gets without raising the kernel's dynamic-LDS limit and
// still leaves two blocks per CU resident (160 KiB of LDS); measured up
// to there the LDS loader is 2.5x-6x the search loader
// (profiles/predict_csr_mi355x.md).
constexpr int64_t kLdsBudget = 64 * 1024;

__device__ __forceinline__ bool StoredValue(float v, float* out) {
  *out = v;
  return !isnan(v);
}

// Row r of the CSR, searched at every visit.
struct CsrSearchRow {
  using Value = float;
  const int32_t* idx;  // first column index of the row
  const float* val;
  int len;
  __device__ bool Get(int f, float* v) const {
    int lo = 0;
    int hi = len;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (idx[mid] < f) {
        lo = mid + 1;
      } else {
        hi = mid;
      }
    }
    if (lo < len && idx[lo] == f) {
      return StoredValue(val[lo], v);
    }
    return false;
  }
  __device__ static int Category(float v) { return (int)v; }
  __device__ static bool Less(float v, int w) {
    return v < __int_as_float(w);
  }
};

// This thread's dense column of the LDS tile.
struct LdsRow {
  using Value = float;
  const float* col;  // tile + tid
  int n_features;
  __device__ bool Get(int f, float* v) const {
    if (f >= n_features) {
      return false;
    }
    return StoredValue(col[f * kBlock], v);
  }
  __device__ static int Category(float v) { return (int)v; }
  __device__ static bool Less(float v, int w) {
    return v < __int_as_float(w);
  }
};

template <int KMAX, bool kLds>
__global__ __launch_bounds__(kBlock) void PredictCsrKernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, int64_t n_rows, int n_features,
    const int4* __restrict__ nodes, const int32_t* __restrict__ tree_offsets,
    const int32_t* __restrict__ cat_offsets,
    const uint32_t* __restrict__ cat_bits,
    const int32_t* __restrict__ tree_group,
    const int32_t* __restrict__ vec_offset,
    const float* __restrict__ leaf_vec, int n_trees, int n_groups,
    float* __restrict__ out_margin, int32_t* __restrict__ out_leaf) {
  extern __shared__ float tile[];  // kLds: [n_features][kBlock]
  const int64_t row0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (int64_t row = row0; row < n_rows;
       row += (int64_t)gridDim.x * kBlock) {
    const int64_t beg = indptr[row];
    const int len = (int)(indptr[row + 1] - beg);
    if constexpr (kLds) {
      float* col = tile + threadIdx.x;
      for (int f = 0; f < n_features; ++f) {
        col[f * kBlock] = __int_as_float(0x7fc00000);  // NaN
      }
      for (int p = 0; p < len; ++p) {
        const int f = indices[beg + p];
        if ((uint32_t)f < (uint32_t)n_features) {
          col[f * kBlock] = values[beg + p];
        }
      }
      const LdsRow rd{col, n_features};
      WalkForest<KMAX>(rd, row, nodes, tree_offsets, cat_offsets, cat_bits,
                       tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                       out_margin, out_leaf);
    } else {
      const CsrSearchRow rd{indices + beg, values + beg, len};
      WalkForest<KMAX>(rd, row, nodes, tree_offsets, cat_offsets, cat_bits,
                       tree_group, vec_offset, leaf_vec, n_trees, n_groups,
                       out_margin, out_leaf);
    }
  }
}

}  // namespace

// force_search: nonzero skips the LDS loader.  grid_cap: most blocks to
// launch, 0 = the default cap of gbt_predict_q.
extern "C" void gbt_predict_csr(
    const int64_t* indptr, const int32_t* indices, const float* values,
    int64_t n_rows, int n_features, const void* nodes,
    const int32_t* tree_offsets, const int32_t* cat_offsets,
    const uint32_t* cat_bits, const int32_t* tree_group,
    const int32_t* vec_offset, const float* leaf_vec, int n_trees,
    int n_groups, float* out_margin, int32_t* out_leaf, int force_search,
    int grid_cap, hipStream_t stream) {
  if (n_rows <= 0 || n_trees <= 0) {
    return;
  }
  const int64_t tile_bytes = (int64_t)n_features * kBlock * sizeof(float);
  const bool lds =
      force_search == 0 && n_features > 0 && tile_bytes <= kLdsBudget;
  const int64_t blocks64 = (n_rows + kBlock - 1) / kBlock;
  const int64_t cap = grid_cap > 0 ? (int64_t)grid_cap : kDefaultGridCap;
  const dim3 grid((unsigned)std::min<int64_t>(blocks64, cap));
  const dim3 block(kBlock);
  const int4* nd = static_cast<const int4*>(nodes);
#define GBT_PREDICT_CSR_LAUNCH(K, LDS)                                       \
  hipLaunchKernelGGL((PredictCsrKernel<K, LDS>), grid, block,                \
                     LDS ? (size_t)tile_bytes : 0, stream, indptr, indices,  \
                     values, n_rows, n_features, nd, tree_offsets,           \
                     cat_offsets, cat_bits, tree_group, vec_offset,          \
                     leaf_vec, n_trees, n_groups, out_margin, out_leaf)
#define GBT_PREDICT_CSR_KMAX(LDS)      \
  if (n_groups == 1) {                 \
    GBT_PREDICT_CSR_LAUNCH(1, LDS);    \
  } else if (n_groups <= 4) {          \
    GBT_PREDICT_CSR_LAUNCH(4, LDS);    \
  } else {                             \
    GBT_PREDICT_CSR_LAUNCH(0, LDS);    \
  }
  if (lds) {
    GBT_PREDICT_CSR_KMAX(true)
  } else {
    GBT_PREDICT_CSR_KMAX(false)
  }
#undef GBT_PREDICT_CSR_KMAX
#undef GBT_PREDICT_CSR_LAUNCH
}
