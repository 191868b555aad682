"""SHAP throughput on sparse CSR input (shap_csr.hip + the SHAP kernels).

Hand-built forests (full trees of depth `--depth`, so an older checkout
gets the very same forest) and two row shapes:

  narrow   `--features` columns, 40 % of the entries stored:
           pred_contribs and pred_interactions on the CSR DMatrix, and,
           as the yardstick, the dense device path on the same rows
           densified with NaN (CSR and dense alternate in one process)
  onehot   39 fields of `--cardinality` one-hot columns each (the Criteo
           row shape), a forest over `--split-cols` of them:
           pred_contribs on the CSR DMatrix, with few enough rows that
           the full-width float32 output stays under 1 GiB

Public rates are host-clock, synchronised, around bst.predict on a
DMatrix built beforehand: upload of the rows on first use, kernels, the
device-to-host copy and the expansion to full width.  The gather
kernel's share of device time is taken from device events around the
NaN fill + gbt_csr_gather_columns and around the path kernel on the
staged tile, the whole matrix as one chunk.

Every path is warmed up, then timed `--repeats` times; the median, min
and max rows/s are reported so the spread is visible.  One JSON line per
shape.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import xgboost_amd as xgb  # noqa: E402
from xgboost_amd.tree_model import RegTree  # noqa: E402

FIELDS = 39


def _rates(n_rows, seconds):
    r = sorted(n_rows / s for s in seconds)
    return {"median": statistics.median(r), "min": r[0], "max": r[-1],
            "runs": len(r)}


def _host_timed_interleaved(fns, warmup, repeats):
    """Host clock around synchronised calls, the paths alternating."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append(time.perf_counter() - t0)
    return out


def _event_timed_interleaved(fns, warmup, repeats, inner):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / 1e3 / inner)
    return out


def narrow_rows(rng, n, f):
    X = rng.randn(n, f).astype(np.float32)
    X[rng.rand(n, f) >= 0.4] = 0.0
    return sp.csr_matrix(X)


def onehot_rows(rng, n, cardinality):
    """One stored 1.0 per field; categories follow a long-tailed law."""
    cat = np.minimum((rng.pareto(1.2, (n, FIELDS)) * 4).astype(np.int64),
                     cardinality - 1)
    cols = (cat + np.arange(FIELDS) * cardinality).astype(np.int32)
    indptr = np.arange(n + 1, dtype=np.int64) * FIELDS
    return sp.csr_matrix((np.ones(n * FIELDS, np.float32), cols.ravel(),
                          indptr), shape=(n, FIELDS * cardinality))


def dense_nan(csr):
    coo = csr.tocoo()
    X = np.full(csr.shape, np.nan, np.float32)
    X[coo.row, coo.col] = coo.data
    return X


def full_tree(rng, n_col, columns, cond_of, depth):
    """Covers halve at every level, so zero fractions are all 0.5."""
    tree = RegTree(n_col)
    frontier = [0]
    h = 1024.0
    for _ in range(depth):
        nxt = []
        for nid in frontier:
            f = int(columns[rng.randint(len(columns))])
            nxt += tree.add_split(nid, f, cond_of(), bool(rng.rand() < 0.5),
                                  1.0, 0.0, 0.01 * rng.randn(),
                                  0.01 * rng.randn(), h, h / 2, h / 2)
        frontier = nxt
        h /= 2
    return tree


def make_booster(rng, n_col, columns, cond_of, n_trees, depth):
    """A cuda booster that holds the hand-built forest."""
    Xs = rng.randn(64, 4).astype(np.float32)
    seed = xgb.train({"max_depth": 1, "objective": "reg:squarederror"},
                     xgb.DMatrix(Xs, label=Xs[:, 0]), 1, verbose_eval=False)
    bst = xgb.Booster({"device": "cuda"})
    bst.load_model(bytes(seed.save_raw("json")))
    bst.trees = [full_tree(rng, n_col, columns, cond_of, depth)
                 for _ in range(n_trees)]
    bst.tree_info = [0] * n_trees
    bst.iteration_indptr = list(range(n_trees + 1))
    bst.n_features = n_col
    return bst


def gather_share(bst, d, args):
    """Device time of the gather against the path kernel, one chunk."""
    from xgboost_amd.backend.gpu import _ShapCsrPlan, _gather_csr_columns
    from xgboost_amd.shap import used_columns
    used, col_map = used_columns(bst.trees, d.num_col())
    plan = _ShapCsrPlan(bst, d, 0, len(bst.trees), used, col_map, False)
    n = d.num_row()
    tile = plan.tile(0, n)
    secs = _event_timed_interleaved(
        {"gather": lambda: _gather_csr_columns(plan.csr, 0, plan.col_map,
                                               tile),
         "paths": lambda: plan.contribs(tile)},
        args.warmup, args.repeats, args.inner)
    g = statistics.median(secs["gather"])
    p = statistics.median(secs["paths"])
    return {"used_columns": len(used), "gather_s": g, "paths_s": p,
            "gather_share_of_device_time": g / (g + p)}


def run_narrow(args):
    rng = np.random.RandomState(0)
    csr = narrow_rows(rng, args.rows, args.features)
    bst = make_booster(rng, args.features, np.arange(args.features),
                       lambda: float(rng.randn() * 0.5), args.trees,
                       args.depth)
    res = {"variant": "narrow", "rows": args.rows, "columns": args.features,
           "nnz_per_row": csr.nnz / args.rows, "trees": args.trees,
           "max_depth": args.depth,
           "interaction_rows": args.interaction_rows}
    d_csr, d_dense = xgb.DMatrix(csr), xgb.DMatrix(dense_nan(csr))
    k = args.interaction_rows
    i_csr = xgb.DMatrix(csr[:k])
    i_dense = xgb.DMatrix(dense_nan(csr[:k]))
    got = bst.predict(d_csr, pred_contribs=True)
    want = bst.predict(d_dense, pred_contribs=True).astype(np.float32)
    res["contribs_equal_dense"] = bool(np.array_equal(got, want))
    got = bst.predict(i_csr, pred_interactions=True)
    want = bst.predict(i_dense, pred_interactions=True)
    res["interactions_equal_dense"] = bool(np.array_equal(got, want))
    del got, want
    secs = _host_timed_interleaved(
        {"csr": lambda: bst.predict(d_csr, pred_contribs=True),
         "dense": lambda: bst.predict(d_dense, pred_contribs=True)},
        args.public_warmup, args.public_repeats)
    res["contribs_csr_rows_per_s"] = _rates(args.rows, secs["csr"])
    res["contribs_dense_rows_per_s"] = _rates(args.rows, secs["dense"])
    secs = _host_timed_interleaved(
        {"csr": lambda: bst.predict(i_csr, pred_interactions=True),
         "dense": lambda: bst.predict(i_dense, pred_interactions=True)},
        args.public_warmup, args.public_repeats)
    res["interactions_csr_rows_per_s"] = _rates(k, secs["csr"])
    res["interactions_dense_rows_per_s"] = _rates(k, secs["dense"])
    res.update(gather_share(bst, d_csr, args))
    return res


def run_onehot(args):
    rng = np.random.RandomState(0)
    n_col = FIELDS * args.cardinality
    n = args.onehot_rows
    if n * (n_col + 1) * 4 >= 1 << 30:
        raise SystemExit("--onehot-rows: the output would pass 1 GiB")
    csr = onehot_rows(rng, n, args.cardinality)
    freq = np.bincount(csr.indices, minlength=n_col)
    columns = np.argsort(-freq, kind="stable")[:args.split_cols]
    bst = make_booster(rng, n_col, columns, lambda: 0.5, args.trees,
                       args.depth)
    res = {"variant": "onehot", "rows": n, "columns": n_col,
           "nnz_per_row": csr.nnz / n, "trees": args.trees,
           "max_depth": args.depth}
    d = xgb.DMatrix(csr)
    secs = _host_timed_interleaved(
        {"csr": lambda: bst.predict(d, pred_contribs=True)},
        args.public_warmup, args.public_repeats)
    res["contribs_csr_rows_per_s"] = _rates(n, secs["csr"])
    res.update(gather_share(bst, d, args))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--interaction-rows", type=int, default=20_000)
    ap.add_argument("--onehot-rows", type=int, default=2_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--cardinality", type=int, default=2560)
    ap.add_argument("--split-cols", type=int, default=100)
    ap.add_argument("--trees", type=int, default=50)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5,
                    help="kernel launches per timed window")
    ap.add_argument("--public-warmup", type=int, default=1)
    ap.add_argument("--public-repeats", type=int, default=5)
    ap.add_argument("--shapes", default="narrow,onehot")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shap_csr_bench needs a GPU")
    for name in args.shapes.split(","):
        run = run_narrow if name == "narrow" else run_onehot
        print(json.dumps(run(args)), flush=True)


if __name__ == "__main__":
    main()
