#!/usr/bin/env python
"""Training with wide categorical columns on 1 MI355X, one JSON line per
measurement.

Data: n rows, 8 numeric columns and a set of categorical columns
(--shape): "mixed" has cardinalities 40, 100 and 500 (both sides of the
64-category wave tier), "cap" has one column of 2000 categories (near the
2048 cap of ops/cpp/evaluate_cat.hip) and one of 30, "many" has eight
columns of 40 and 100.  reg:squarederror, depth 8, max_bin 256,
max_cat_to_onehot 4, so every categorical column takes sorted-partition
splits and the tree grows on the level-by-level driver.

Per shape, in the order kernel, host, host, kernel (XGB_AMD_CAT_HIP = 1 / 0;
0 is the host routine GpuOps._host_sorted_cat, the only route before the
kernel existed): rounds/s over --steps Booster.update calls after --warmup,
a host clock around work that ends in a device synchronise.  Then one more
pass per route with a synchronising clock around every
GpuOps.evaluate_splits call, reported as median ms per tree level.  The
"control" rows are the same data without the categorical columns (the
whole-tree native driver, which none of this touches), run under both
settings of the variable to give the run-to-run noise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xgboost_amd as xgb  # noqa: E402
from xgboost_amd.backend.gpu import GpuOps  # noqa: E402

SHAPES = {"mixed": [40, 100, 500], "cap": [2000, 30],
          "many": [40, 100] * 4}
N_NUMERIC = 8


def _data(n, cards):
    rng = np.random.RandomState(7)
    xn = rng.randn(n, N_NUMERIC).astype(np.float32)
    cats = [rng.randint(0, c, n) for c in cards]
    y = xn[:, :4] @ rng.randn(4) + rng.randn(n)
    for c, codes in zip(cards, cats):
        y += rng.randn(c)[codes]  # one random effect per category
    X = np.column_stack([xn] + cats).astype(np.float32)
    ft = ["q"] * N_NUMERIC + ["c"] * len(cards)
    return (xgb.DMatrix(X, label=y.astype(np.float32), feature_types=ft),
            xgb.DMatrix(xn, label=y.astype(np.float32)))


PARAMS = {"objective": "reg:squarederror", "max_depth": 8, "max_bin": 256,
          "eta": 0.1, "tree_method": "hist", "device": "cuda", "seed": 7,
          "max_cat_to_onehot": 4}


def _rounds(d, steps, warmup):
    bst = xgb.Booster(PARAMS, cache=[d])
    for it in range(warmup):
        bst.update(d, it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        bst.update(d, warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return bst, ms


def _evaluate_levels(d, steps, warmup):
    """Median ms of evaluate_splits per tree level over `steps` trees."""
    levels = {}
    state = {"level": 0, "on": False}
    inner = GpuOps.evaluate_splits

    def timed(self, hist, quantizer, parent_sums, nids, *a, **kw):
        state["level"] = 0 if len(nids) == 1 else state["level"] + 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(self, hist, quantizer, parent_sums, nids, *a, **kw)
        torch.cuda.synchronize()
        if state["on"]:
            levels.setdefault(state["level"], []).append(
                (time.perf_counter() - t0) * 1e3)
        return out

    GpuOps.evaluate_splits = timed
    try:
        bst = xgb.Booster(PARAMS, cache=[d])
        for it in range(warmup + steps):
            state["on"] = it >= warmup
            bst.update(d, it)
    finally:
        GpuOps.evaluate_splits = inner
    return {lv: round(float(np.median(t)), 3) for lv, t in sorted(levels.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--no-control", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    for shape in args.shape or sorted(SHAPES):
        d_cat, d_num = _data(args.rows, SHAPES[shape])
        base = {"rows": args.rows, "shape": shape,
                "cardinalities": SHAPES[shape], "steps": args.steps,
                "warmup": args.warmup}
        runs = [("categorical", d_cat)]
        if not args.no_control:
            runs.append(("control", d_num))
        preds = {}
        for data, d in runs:
            for flag in ("1", "0", "0", "1"):
                os.environ["XGB_AMD_CAT_HIP"] = flag
                bst, ms = _rounds(d, args.steps, args.warmup)
                p = bst.predict(d)
                same = np.array_equal(preds.setdefault(data, p), p)
                print(json.dumps(dict(
                    base, data=data, route="kernel" if flag == "1" else "host",
                    rounds_per_s=round(args.steps / ms * 1e3, 3),
                    ms_per_round=round(ms / args.steps, 3),
                    predictions_equal_first_run=bool(same))), flush=True)
        for flag in ("1", "0"):
            os.environ["XGB_AMD_CAT_HIP"] = flag
            lv = _evaluate_levels(d_cat, min(args.steps, 5), args.warmup)
            print(json.dumps(dict(
                base, data="categorical",
                route="kernel" if flag == "1" else "host",
                evaluate_splits_ms_per_level=lv)), flush=True)
    os.environ.pop("XGB_AMD_CAT_HIP", None)


if __name__ == "__main__":
    main()
