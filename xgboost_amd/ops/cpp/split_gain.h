// The one definition of a split candidate's gain, shared by every
// evaluator: the HIP kernels (evaluate.hip, mt_evaluate.hip) and the
// native CPU evaluator (cpu_hist.cpp, compiled as plain host C++).  All
// of them evaluate this fp64 expression tree in this operation order (the
// numpy oracle's, xgboost_amd/splits.py) and apply this tie rule, which is
// what keeps CPU trees, GPU trees and the oracle identical.
#pragma once
#include <cmath>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GBT_HD __host__ __device__ __forceinline__
#else
#define GBT_HD inline
#endif

struct SplitParams {
  double lam, alpha, mds, mcw;
  double lo, hi;  // node weight bounds; -/+INFINITY when unconstrained
};

struct Best {
  double gain;
  int bin;       // global bin id
  int dir;       // 1 = missing-left
  long long lg;  // left sums (quantized)
  long long lh;
};

GBT_HD bool Better(const Best& a, const Best& b) {
  // match numpy: strictly-greater gain wins; ties keep (dir asc, bin asc)
  if (a.gain != b.gain) return a.gain > b.gain;
  if (a.dir != b.dir) return a.dir < b.dir;
  return a.bin < b.bin;
}

GBT_HD double ThresholdL1(double g, double alpha) {
  if (alpha == 0.0) return g;
  double s = (g > 0.0) ? 1.0 : ((g < 0.0) ? -1.0 : 0.0);
  double m = fabs(g) - alpha;
  if (m < 0.0) m = 0.0;
  return s * m;
}

GBT_HD double CalcWeight(double g, double h, const SplitParams& p) {
  double w = -ThresholdL1(g, p.alpha) / (h + p.lam);
  if (p.mds > 0.0) {
    w = fmin(fmax(w, -p.mds), p.mds);
  }
  return w;
}

GBT_HD double GainGivenWeight(double g, double h, double w,
                              const SplitParams& p) {
  return -(2.0 * g * w + (h + p.lam) * (w * w));
}

// One candidate split (bin b, missing direction dir, left sums glq/hlq)
// of a node with sums pg/ph: scaling, CalcWeight, the bound clamp, the
// validity test and the gain expression.  Every single-target evaluator
// calls this, so all evaluate the same fp64 expression tree and their
// results are bit-identical.
GBT_HD void TryCandidate(long long glq, long long hlq, long long pg,
                         long long ph, double inv_g, double inv_h,
                         const SplitParams& p, int mono, double parent_gain,
                         int b, int dir, Best* best) {
  const long long grq = pg - glq;
  const long long hrq = ph - hlq;
  const double gl = glq * inv_g;
  const double hl = hlq * inv_h;
  const double gr = grq * inv_g;
  const double hr = hrq * inv_h;
  double wl = CalcWeight(gl, hl, p);
  double wr = CalcWeight(gr, hr, p);
  wl = fmin(fmax(wl, p.lo), p.hi);
  wr = fmin(fmax(wr, p.lo), p.hi);
  // empty-side splits rejected via exact hessian counts; the
  // last-bin + missing-right split (present vs absent) is valid
  bool ok = (hl >= p.mcw) && (hr >= p.mcw) && hlq > 0 && hrq > 0;
  if (mono > 0) ok = ok && (wl <= wr);
  if (mono < 0) ok = ok && (wl >= wr);
  if (ok) {
    const double gain = GainGivenWeight(gl, hl, wl, p)
                        + GainGivenWeight(gr, hr, wr, p) - parent_gain;
    Best cand{gain, b, dir, glq, hlq};
    if (std::isfinite(gain) && Better(cand, *best)) *best = cand;
  }
}
