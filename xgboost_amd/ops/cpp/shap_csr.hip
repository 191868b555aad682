// CSR -> compact feature-major tile for TreeSHAP on sparse input.
//
// The SHAP kernels (shap_paths.hip, shap_ix.hip, shap.hip) read a dense
// matrix; a forest over a wide sparse matrix splits on only U of its F
// columns, so the host numbers those U columns 0..U-1 in ascending
// order (col_map[c] = compact id, -1 for an unused column) and this
// kernel stages one row chunk of the CSR as the [U, n_rows_chunk]
// feature-major tile ShapPathsKernel was tuned for.  The caller fills
// the tile with NaN first: an absent entry stays missing, a stored NaN
// is written and is missing, a stored 0.0 is a value.
//
// Mapping: one 64-lane wave per row, the lanes striding the row's
// entries, so indices[] and values[] are read coalesced; the writes are
// one dword per used entry at stride n_rows_chunk and scattered under
// any mapping that reads the CSR coalesced.  Column indices within a
// row are unique, so no two lanes write one cell.  Pure bandwidth, once
// per chunk: no LDS, no barrier.
#include "gbt_kernels.h"

namespace {

constexpr int kWavesPerBlock = 4;

__global__ __launch_bounds__(64 * kWavesPerBlock) void CsrGatherColumnsKernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, long long row_begin,
    long long n_rows_chunk, const int32_t* __restrict__ col_map,
    int n_col_map, int n_used, float* __restrict__ tile) {
  const int lane = threadIdx.x & 63;
  const long long wave0 =
      (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * kWavesPerBlock;
  for (long long r = wave0; r < n_rows_chunk; r += stride) {
    const int64_t beg = indptr[row_begin + r];
    const int64_t end = indptr[row_begin + r + 1];
    for (int64_t k = beg + lane; k < end; k += 64) {
      // unsigned compare: a negative or too-large column never indexes
      // col_map; the same compare drops -1 (unused) and guards the tile
      const uint32_t c = (uint32_t)indices[k];
      if (c >= (uint32_t)n_col_map) continue;
      const uint32_t u = (uint32_t)col_map[c];
      if (u >= (uint32_t)n_used) continue;
      tile[(size_t)u * (size_t)n_rows_chunk + (size_t)r] = values[k];
    }
  }
}

}  // namespace

// tile is [n_used, n_rows_chunk] float32, NaN-filled by the caller;
// rows [row_begin, row_begin + n_rows_chunk) must exist in indptr.
extern "C" void gbt_csr_gather_columns(
    const int64_t* indptr, const int32_t* indices, const float* values,
    long long row_begin, long long n_rows_chunk, const int32_t* col_map,
    int n_col_map, int n_used, float* tile, hipStream_t stream) {
  if (n_rows_chunk <= 0 || n_used <= 0 || n_col_map <= 0) return;
  const long long want = (n_rows_chunk + kWavesPerBlock - 1) / kWavesPerBlock;
  const int blocks = (int)(want < 16384 ? want : 16384);
  hipLaunchKernelGGL(CsrGatherColumnsKernel, dim3(blocks),
                     dim3(64 * kWavesPerBlock), 0, stream, indptr, indices,
                     values, row_begin, n_rows_chunk, col_map, n_col_map,
                     n_used, tile);
}
