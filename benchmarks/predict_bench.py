"""Prediction throughput of the packed-node predictor (predict_bins.hip).

One forest (100 trees, depth 8, 28 features; scalar leaves, plus a K=3
vector-leaf variant) and four paths over the same rows:

  (a) extmem   bst.predict(ExtMemQuantileDMatrix): pages uploaded and
               walked as stored (includes H2D of the pages, D2H of the
               result and the Python around it; host clock, synchronised)
  (b) kernel_q gbt_predict_q alone on a device-resident u8 page
               (device events)
  (c) kernel_f the existing gbt_predict on the same rows as raw floats
               (device events; scalar leaves only)
  (d) kernel_qf gbt_predict_q on those same device-resident float rows
               (kind 0), timed in windows that alternate with (c) so that
               the two see the same clocks; `qf_over_f` is the ratio of
               the medians

`--trees 1 --max-depth 6` is the per-round eval-set update, where reading
the row dominates.

Every path is warmed up, then timed `--repeats` times; the median, min
and max rows/s are reported so the spread is visible.  One JSON line per
variant.  `--only-extmem` runs (a) alone and uses nothing newer than the
public API, so the same script can time an older checkout.
"""
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
from xgboost_amd.extmem import DataIter, ExtMemQuantileDMatrix  # noqa: E402


class _Pages(DataIter):
    def __init__(self, Xs):
        super().__init__()
        self.Xs, self.i = Xs, 0

    def reset(self):
        self.i = 0

    def next(self, input_data) -> bool:
        if self.i >= len(self.Xs):
            return False
        input_data(data=self.Xs[self.i])
        self.i += 1
        return True


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


def _event_timed(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / 1e3 / inner)
    return out


def _event_timed_pair(fn_a, fn_b, warmup, repeats, inner):
    """_event_timed for two calls whose windows alternate a, b, a, b."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    out_a, out_b = [], []
    for _ in range(repeats):
        out_a += _event_timed(fn_a, 0, 1, inner)
        out_b += _event_timed(fn_b, 0, 1, inner)
    return out_a, out_b


def run_variant(name, args, X, Xtrain, ytrain):
    params = {"max_depth": args.max_depth, "max_bin": 256, "eta": 0.1,
              "device": "cuda",
              "objective": "reg:squarederror"}
    if name == "vector_k3":
        params["multi_strategy"] = "multi_output_tree"
    dtrain = xgb.DMatrix(Xtrain, label=ytrain)
    bst = xgb.train(params, dtrain, args.trees, verbose_eval=False)
    n = X.shape[0]
    res = {"variant": name, "rows": n, "features": X.shape[1],
           "trees": len(bst.trees), "max_depth": args.max_depth,
           "nodes": int(sum(t.n_nodes for t in bst.trees)),
           "pages": args.pages}
    d_ext = ExtMemQuantileDMatrix(_Pages(np.array_split(X, args.pages)),
                                  max_bin=256, ref=dtrain)
    ext_repeats = args.extmem_repeats or args.repeats
    res["extmem_rows_per_s"] = _rates(n, _host_timed(
        lambda: bst.predict(d_ext), 0 if args.only_extmem else args.warmup,
        ext_repeats))
    if args.only_extmem:
        return res

    from xgboost_amd.backend.gpu import (_cached_forest_q, _launch_predict_q,
                                         predict_margin_gpu)
    dev = torch.device("cuda")
    K = bst.n_outputs
    page = torch.cat([d_ext.page_qm(i).gidx for i in range(args.pages)])
    assert page.dtype == torch.uint8
    page = page.to(dev)
    fa = _cached_forest_q(bst, 0, len(bst.trees), dev, d_ext.cuts)
    out = torch.zeros((n, K), dtype=torch.float32, device=dev)
    res["kernel_q_rows_per_s"] = _rates(n, _event_timed(
        lambda: _launch_predict_q(fa, page, float("nan"), out, None),
        args.warmup, args.repeats, args.inner))
    if name == "scalar":
        d_dev = xgb.DMatrix(torch.from_numpy(X).to(dev))
        Xd = d_dev.device_data()
        fa_f = _cached_forest_q(bst, 0, len(bst.trees), dev, None)
        t_f, t_qf = _event_timed_pair(
            lambda: predict_margin_gpu(bst, d_dev, out, 0, len(bst.trees)),
            lambda: _launch_predict_q(fa_f, Xd, float("nan"), out, None),
            args.warmup, args.repeats, args.inner)
        res["kernel_f_rows_per_s"] = _rates(n, t_f)
        res["kernel_qf_rows_per_s"] = _rates(n, t_qf)
        res["qf_over_f"] = (res["kernel_qf_rows_per_s"]["median"]
                            / res["kernel_f_rows_per_s"]["median"])
        # same rows, same forest: the kernels must agree exactly (bins
        # too, when the split conditions are cut values)
        a = torch.zeros((n, K), dtype=torch.float32, device=dev)
        b = torch.zeros((n, K), dtype=torch.float32, device=dev)
        c = torch.zeros((n, K), dtype=torch.float32, device=dev)
        _launch_predict_q(fa, page, float("nan"), a, None)
        predict_margin_gpu(bst, d_dev, b, 0, len(bst.trees))
        _launch_predict_q(fa_f, Xd, float("nan"), c, None)
        res["q_equals_f"] = bool(torch.equal(a, b))
        res["qf_equals_f"] = bool(torch.equal(c, b))
    else:
        res["kernel_f_rows_per_s"] = None  # gbt_predict has no vector leaves
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5,
                    help="kernel launches per timed window")
    ap.add_argument("--extmem-repeats", type=int, default=0)
    ap.add_argument("--only-extmem", action="store_true")
    ap.add_argument("--variants", default="scalar,vector_k3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench needs a GPU")
    rng = np.random.RandomState(0)
    X = rng.randn(args.rows, args.features).astype(np.float32)
    Xtrain = X[:args.train_rows]
    W = rng.randn(args.features, 3)
    Y = (Xtrain @ W + Xtrain[:, :1] * Xtrain[:, 1:2]).astype(np.float32)
    for name in args.variants.split(","):
        y = Y if name == "vector_k3" else Y[:, 0]
        print(json.dumps(run_variant(name, args, X, Xtrain, y)), flush=True)


if __name__ == "__main__":
    main()
