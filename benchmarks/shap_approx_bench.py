#!/usr/bin/env python
"""approx_contribs (Saabas, shap_saabas.hip) on 1 MI355X against

  host   the Python loop shap._saabas, which every approx_contribs call
         took before the kernel (a CPU copy of the same model), at a shape
         that loop can finish: 20k rows x 100 trees, depth 6;
  exact  this commit's exact device pred_contribs at the shape of
         shap_bench.py: 1e6 x 28, 500 trees, depth 6.

Times are host clocks around predict() ending in a device synchronise,
after one warm call on the same matrix; the device calls are repeated
and the median is reported with the spread.  Prints one JSON line per
comparison."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xgboost_amd as xgb  # noqa: E402
from bench import make_higgs_like  # noqa: E402

APPROX = {"pred_contribs": True, "approx_contribs": True}


def _timed(bst, d, reps, **mode):
    """(median, min, max) seconds of `reps` predict calls after a warm one,
    and the last result."""
    out = bst.predict(d, **mode)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = bst.predict(d, **mode)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times), out


def _train(rows, trees, depth):
    X, y = make_higgs_like(rows, 28, seed=7)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "binary:logistic", "max_depth": depth,
                     "device": "cuda", "eta": 0.1}, d, trees,
                    verbose_eval=False)
    return bst, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--host-rows", type=int, default=20_000)
    ap.add_argument("--host-trees", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shap_approx_bench.py measures the device: no GPU")

    # host loop against the kernel
    bst, d = _train(args.host_rows, args.host_trees, args.depth)
    med, lo, hi, dev = _timed(bst, d, args.reps, **APPROX)
    cpu = xgb.Booster({"device": "cpu"})
    cpu.load_model(bytes(bst.save_raw("json")))
    t0 = time.perf_counter()
    host = cpu.predict(d, **APPROX)
    t_host = time.perf_counter() - t0
    print(json.dumps({
        "metric": "approx_contribs_device_vs_host", "rows": args.host_rows,
        "trees": args.host_trees, "depth": args.depth,
        "device_seconds": med, "device_min": lo, "device_max": hi,
        "host_seconds": t_host, "speedup": t_host / med,
        "max_abs_diff": float(np.abs(dev - host).max()),
    }), flush=True)

    # the kernel against exact device SHAP
    bst, d = _train(args.rows, args.trees, args.depth)
    a_med, a_lo, a_hi, approx = _timed(bst, d, args.reps, **APPROX)
    e_med, e_lo, e_hi, _ = _timed(bst, d, args.reps, pred_contribs=True)
    margin = bst.predict(d, output_margin=True)
    print(json.dumps({
        "metric": "approx_vs_exact_contribs", "rows": args.rows,
        "trees": args.trees, "depth": args.depth,
        "approx_seconds": a_med, "approx_min": a_lo, "approx_max": a_hi,
        "exact_seconds": e_med, "exact_min": e_lo, "exact_max": e_hi,
        "approx_rows_per_sec": args.rows / a_med,
        "exact_rows_per_sec": args.rows / e_med,
        "exact_over_approx": e_med / a_med,
        "approx_efficiency_max_err":
            float(np.abs(approx.sum(axis=1) - margin).max()),
    }), flush=True)


if __name__ == "__main__":
    main()
