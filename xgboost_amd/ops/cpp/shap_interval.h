// The element test of the path-table SHAP kernels (shap_paths.hip,
// shap_ix.hip): does the row's value x follow this path element?
#pragma once
#include "gbt_kernels.h"

// A missing value follows the element iff the default direction agrees
// at every occurrence of the feature (miss_ok); any other value iff
// lo <= x < hi.  An upper end of +inf means "no split sent this path
// left", so it is unbounded: +inf agrees with it, as `x < cond` is false
// in the tree walk and sends +inf right.  -inf needs no such case: it
// satisfies lo = -inf by >= and fails every finite lo.
__device__ __forceinline__ bool ShapElementAgrees(float x, float lo, float hi,
                                                  bool miss_ok,
                                                  float missing_value,
                                                  int missing_is_nan) {
  const bool miss =
      missing_is_nan ? isnan(x) : (isnan(x) || x == missing_value);
  return miss ? miss_ok : (x >= lo && (x < hi || hi == INFINITY));
}
