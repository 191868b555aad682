// Forest walk shared by the packed-node predictors (predict_bins.hip,
// predict_csr.hip): one thread walks every tree for one row and adds the
// leaves in tree order.  The row is read through a loader object, so the
// node decision and the leaf accumulation exist once:
//
//   bool Get(int f, Value* v) const   false when feature f is missing
//   static int Category(Value v)      category id of a stored value
//   static bool Less(Value v, int w)  numeric "goes left" against the
//                                     node's value word
//
// Node record (int4): {left, right, feature | default_left<<31 |
// is_cat<<30, value word}; left == -1 marks a leaf whose value word is
// the fp32 leaf value.  Categorical nodes: category in the stored set
// goes RIGHT.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gbt_walk {

constexpr uint32_t kDefaultLeft = 1u << 31;
constexpr uint32_t kIsCat = 1u << 30;
constexpr uint32_t kFeatMask = kIsCat - 1u;

// Blocks of 256 rows per launch before the grid-stride loop takes over.
constexpr int64_t kDefaultGridCap = 2048 * 4;

// KMAX: 1 = single output column in a register, 4 = up to four columns
// in registers (statically indexed), 0 = accumulate in global memory.
template <int KMAX, typename Loader>
__device__ __forceinline__ void WalkForest(
    const Loader& row_data, int64_t row, const int4* __restrict__ nodes,
    const int32_t* __restrict__ tree_offsets,
    const int32_t* __restrict__ cat_offsets,
    const uint32_t* __restrict__ cat_bits,
    const int32_t* __restrict__ tree_group,
    const int32_t* __restrict__ vec_offset,
    const float* __restrict__ leaf_vec, int n_trees, int n_groups,
    float* __restrict__ out_margin, int32_t* __restrict__ out_leaf) {
  constexpr int kRegs = KMAX > 0 ? KMAX : 1;
  float* orow = out_margin != nullptr ? out_margin + row * n_groups : nullptr;
  float acc[kRegs];
  if (KMAX > 0 && orow != nullptr) {
#pragma unroll
    for (int k = 0; k < kRegs; ++k) {
      acc[k] = k < n_groups ? orow[k] : 0.0f;
    }
  }
  for (int t = 0; t < n_trees; ++t) {
    const int base = tree_offsets[t];
    int nid = 0;
    int4 nd = nodes[base];
    while (nd.x != -1) {
      const uint32_t fw = (uint32_t)nd.z;
      const int f = (int)(fw & kFeatMask);
      typename Loader::Value v;
      const bool missing = !row_data.Get(f, &v);
      bool go_left;
      if (missing) {
        go_left = (fw & kDefaultLeft) != 0;
      } else if (fw & kIsCat) {
        const int c = Loader::Category(v);
        const int w0 = cat_offsets[base + nid];
        const int nw = cat_offsets[base + nid + 1] - w0;
        bool in_set = false;
        if (c >= 0 && (c >> 5) < nw) {
          in_set = (cat_bits[w0 + (c >> 5)] >> (c & 31)) & 1u;
        }
        go_left = !in_set;  // stored set goes RIGHT
      } else {
        go_left = Loader::Less(v, nd.w);
      }
      nid = go_left ? nd.x : nd.y;
      nd = nodes[base + nid];
    }
    if (out_leaf != nullptr) {
      out_leaf[row * n_trees + t] = nid;
    }
    if (orow == nullptr) {
      continue;
    }
    const int g = tree_group[t];
    if (g >= 0) {
      const float leaf = __int_as_float(nd.w);
      if (KMAX > 0) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) {
          if (k == g) acc[k] += leaf;
        }
      } else {
        orow[g] += leaf;
      }
    } else {
      const float* lv = leaf_vec + ((int64_t)vec_offset[t] + nid) * n_groups;
      if (KMAX > 0) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) {
          if (k < n_groups) acc[k] += lv[k];
        }
      } else {
        for (int k = 0; k < n_groups; ++k) {
          orow[k] += lv[k];
        }
      }
    }
  }
  if (KMAX > 0 && orow != nullptr) {
#pragma unroll
    for (int k = 0; k < kRegs; ++k) {
      if (k < n_groups) orow[k] = acc[k];
    }
  }
}

}  // namespace gbt_walk
