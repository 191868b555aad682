"""Prediction throughput on sparse CSR input (predict_csr.hip).

One forest shape (100 full trees of depth 8, scalar leaves, built by hand
so the number of distinct split columns is a parameter and an older
checkout gets the very same forest) and two row shapes:

  narrow   28 columns, about half of the entries stored
  onehot   39 fields of `--cardinality` one-hot columns each, one stored
           1.0 per field and row (the Criteo row shape); the forest
           splits on `--split-cols` distinct columns, drawn from the
           frequent categories

Paths:

  (a) public    bst.predict(DMatrix(csr)): everything a caller pays for
                (DMatrix construction, upload, kernel or host walk, D2H;
                host clock, synchronised)
  (b) search    gbt_predict_csr alone, binary-search loader, on
                device-resident CSR arrays (device events)
  (c) lds       the same with the LDS-dense loader (narrow shape), and a
                sweep over `--lds-widths` columns at the same density
                (up to the 64 columns the loader is used for), search
                and LDS interleaved in one process

Every path is warmed up, then timed `--repeats` times; the median, min
and max rows/s are reported so the spread is visible.  One JSON line per
variant.  `--only-public` runs (a) alone and uses nothing newer than the
public API, so the same script can time an older checkout.
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

DEPTH = 8
FIELDS = 39


def _rates(n_rows, seconds):
    r = sorted(n_rows / s for s in seconds)
    return {"median": statistics.median(r), "min": r[0], "max": r[-1],
            "runs": len(r)}


def _host_timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def _event_timed_interleaved(fns, warmup, repeats, inner):
    """Times several launches in alternating rounds of one process."""
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
    X[rng.rand(n, f) < 0.5] = 0.0
    return sp.csr_matrix(X)


def onehot_rows(rng, n, cardinality):
    """One stored 1.0 per field; categories follow a long-tailed law."""
    cat = np.minimum((rng.pareto(1.2, (n, FIELDS)) * 4).astype(np.int64),
                     cardinality - 1)
    cols = (cat + np.arange(FIELDS) * cardinality).astype(np.int32)
    indptr = np.arange(n + 1, dtype=np.int64) * FIELDS
    return sp.csr_matrix((np.ones(n * FIELDS, np.float32), cols.ravel(),
                          indptr), shape=(n, FIELDS * cardinality))


def full_tree(rng, n_col, columns, cond_of):
    tree = RegTree(n_col)
    frontier = [0]
    for _ in range(DEPTH):
        nxt = []
        for nid in frontier:
            f = int(columns[rng.randint(len(columns))])
            nxt += tree.add_split(nid, f, cond_of(), bool(rng.rand() < 0.5),
                                  1.0, 0.0, 0.01 * rng.randn(),
                                  0.01 * rng.randn(), 1.0, 0.5, 0.5)
        frontier = nxt
    return tree


def make_booster(rng, n_col, columns, cond_of, n_trees):
    """A cuda booster that holds the hand-built forest."""
    Xs = rng.randn(64, 4).astype(np.float32)
    seed = xgb.train({"max_depth": 1, "objective": "reg:squarederror"},
                     xgb.DMatrix(Xs, label=Xs[:, 0]), 1, verbose_eval=False)
    bst = xgb.Booster({"device": "cuda"})
    bst.load_model(bytes(seed.save_raw("json")))
    bst.trees = [full_tree(rng, n_col, columns, cond_of)
                 for _ in range(n_trees)]
    bst.tree_info = [0] * n_trees
    bst.iteration_indptr = list(range(n_trees + 1))
    bst.n_features = n_col
    return bst


def kernel_fns(bst, csr, variants):
    from xgboost_amd.backend.gpu import (_cached_forest_q,
                                         _launch_predict_csr, _upload_csr)
    dev = torch.device("cuda")
    fa = _cached_forest_q(bst, 0, len(bst.trees), dev, None)
    indptr, indices, values = _upload_csr(csr, dev)
    outs = {k: torch.zeros((csr.shape[0], 1), dtype=torch.float32,
                           device=dev) for k in variants}

    def launcher(k, force):
        return lambda: _launch_predict_csr(fa, indptr, indices, values,
                                           csr.shape[1], outs[k], None,
                                           force_search=force)
    fns = {k: launcher(k, force) for k, force in variants.items()}
    return fns, outs


def _same_margins(fns, outs):
    """One launch of each loader on zeroed outputs: bit-equal margins."""
    for o in outs.values():
        o.zero_()
    for fn in fns.values():
        fn()
    return bool(torch.equal(outs["lds"], outs["search"]))


def run_shape(name, args, rng, csr, columns, cond_of):
    bst = make_booster(rng, csr.shape[1], columns, cond_of, args.trees)
    used = len({int(t.split_index[i]) for t in bst.trees
                for i in range(t.n_nodes) if not t.is_leaf(i)})
    n = csr.shape[0]
    res = {"variant": name, "rows": n, "columns": csr.shape[1],
           "nnz_per_row": csr.nnz / n, "trees": len(bst.trees),
           "max_depth": DEPTH, "split_columns": used}
    res["public_rows_per_s"] = _rates(n, _host_timed(
        lambda: bst.predict(xgb.DMatrix(csr)), args.public_warmup,
        args.public_repeats))
    if args.only_public:
        return res
    variants = {"search": 1}
    if name == "narrow":
        variants["lds"] = 0
    fns, outs = kernel_fns(bst, csr, variants)
    for k, secs in _event_timed_interleaved(fns, args.warmup, args.repeats,
                                            args.inner).items():
        res[f"kernel_{k}_rows_per_s"] = _rates(n, secs)
    if "lds" in outs:
        res["lds_equals_search"] = _same_margins(fns, outs)
    return res


def run_lds_width(args, rng, width):
    csr = narrow_rows(rng, args.rows, width)
    bst = make_booster(rng, width, np.arange(width),
                       lambda: float(rng.randn() * 0.5), args.trees)
    fns, outs = kernel_fns(bst, csr, {"search": 1, "lds": 0})
    res = {"variant": "lds_width", "rows": args.rows, "columns": width,
           "lds_bytes_per_block": width * 1024}
    for k, secs in _event_timed_interleaved(fns, args.warmup, args.repeats,
                                            args.inner).items():
        res[f"kernel_{k}_rows_per_s"] = _rates(args.rows, secs)
    res["lds_equals_search"] = _same_margins(fns, outs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--onehot-rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--cardinality", type=int, default=2560)
    ap.add_argument("--split-cols", type=int, default=2000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5,
                    help="kernel launches per timed window")
    ap.add_argument("--public-warmup", type=int, default=1)
    ap.add_argument("--public-repeats", type=int, default=3)
    ap.add_argument("--only-public", action="store_true")
    ap.add_argument("--shapes", default="narrow,onehot")
    ap.add_argument("--lds-widths", default="8,16,28,32,48,64",
                    help="column counts of the LDS/search sweep ('' = skip)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_csr_bench needs a GPU")
    for name in args.shapes.split(","):
        rng = np.random.RandomState(0)
        if name == "narrow":
            csr = narrow_rows(rng, args.rows, args.features)
            columns = np.arange(args.features)

            def cond_of():
                return float(rng.randn() * 0.5)
        else:
            csr = onehot_rows(rng, args.onehot_rows, args.cardinality)
            # the most frequent columns carry the splits
            freq = np.bincount(csr.indices, minlength=csr.shape[1])
            columns = np.argsort(-freq, kind="stable")[:args.split_cols]

            def cond_of():
                return 0.5
        print(json.dumps(run_shape(name, args, rng, csr, columns, cond_of)),
              flush=True)
    if args.only_public or not args.lds_widths:
        return
    for width in (int(w) for w in args.lds_widths.split(",")):
        rng = np.random.RandomState(width)
        print(json.dumps(run_lds_width(args, rng, width)), flush=True)


if __name__ == "__main__":
    main()
