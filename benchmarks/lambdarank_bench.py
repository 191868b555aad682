#!/usr/bin/env python
"""LambdaMART get_gradient alone on 1 MI355X: the HIP kernel
(XGB_AMD_RANK_HIP=1) against the torch formulation (=0), alternated call
by call in one process, device-synchronised.  One JSON line per
measurement (median / min / max in ms) and one per output comparison.

Shape (a): 1M documents in 10k groups of 100, feature_bench.py's labels,
scores from a few boosting rounds.  Shape (b): about 1M documents in
seeded log-normal group sizes clipped to 1..1251, same scores.
--tiers also times the kernel's alternative block shapes.

--slab times the slab tier instead (lambdarank_slab.hip, groups above
2048 documents): one group of 2^12 .. 2^18 documents, the kernel against
the torch path for the three objectives, which sets LAMBDARANK_MAX_GROUP;
the slab shapes; and shape (m), 1M documents in groups of 100 with two
groups of 4096 among them (0.8% of the documents), against the torch path
that a data set with one such group took whole before this tier, with the
same groups of 100 alone beside it.

--metrics times the ranking metrics instead (rank_metric.hip): Booster.
eval_set per call at shape (a) for ndcg, map@10 and pre@10, the kernel
against XGB_AMD_RANK_METRIC_HIP=0; the kernel's block shapes at shape (b)
and at shape (c), 61 groups of 16384; and one group of 2^m documents on
the kernel against the host's copy + argsort, which sets
RANK_METRIC_MAX_GROUP."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xgboost_amd as xgb  # noqa: E402
from xgboost_amd.backend import gpu as gpu_backend  # noqa: E402
from xgboost_amd.data import MetaInfo  # noqa: E402
from xgboost_amd.objectives import create_objective  # noqa: E402


def _info(labels, sizes):
    info = MetaInfo()
    info.num_row = int(labels.shape[0])
    info.labels = labels
    info.group_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return info


def _call(obj, preds, info, flag):
    os.environ["XGB_AMD_RANK_HIP"] = flag
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = obj.get_gradient(preds, info, 0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ab(name, shape, info, preds, calls, warmup):
    """Alternate the two paths; report each and their output difference."""
    objs = {"1": create_objective(name), "0": create_objective(name)}
    times = {"1": [], "0": []}
    outs = {}
    for i in range(warmup + calls):
        for flag in ("1", "0"):
            ms, outs[flag] = _call(objs[flag], preds, info, flag)
            if i >= warmup:
                times[flag].append(ms)
    for flag, path in (("1", "hip"), ("0", "torch")):
        t = np.asarray(times[flag])
        print(json.dumps({"bench": f"{name} get_gradient {shape}",
                          "path": path, "calls": calls,
                          "median_ms": round(float(np.median(t)), 4),
                          "min_ms": round(float(t.min()), 4),
                          "max_ms": round(float(t.max()), 4)}), flush=True)
    for which, a, b in (("g", outs["1"][0], outs["0"][0]),
                        ("h", outs["1"][1], outs["0"][1])):
        a, b = a.double().view(-1), b.double().view(-1)
        d = (a - b).abs()
        big = b.abs() > 1e-6 * b.abs().max()
        print(json.dumps({"compare": f"{name} {shape} {which}",
                          "max_abs_diff": float(d.max()),
                          "max_abs_ref": float(b.abs().max()),
                          "max_rel_diff": float((d[big] / b.abs()[big]).max())
                          }), flush=True)


def tiers(name, shape, info, preds, calls, warmup):
    """The kernel with each alternative block shape, alternated."""
    default = dict(gpu_backend.LAMBDARANK_TIERS)
    variants = {"mid128": {"mid": (256, 1)}, "mid256": {"mid": (256, 2)},
                "large256": {"large": (2048, 3)},
                "large512": {"large": (2048, 4)}}
    obj = create_objective(name)
    times = {v: [] for v in variants}
    try:
        for i in range(warmup + calls):
            for v, patch in variants.items():
                gpu_backend.LAMBDARANK_TIERS = dict(default, **patch)
                ms, _ = _call(obj, preds, info, "1")
                if i >= warmup:
                    times[v].append(ms)
    finally:
        gpu_backend.LAMBDARANK_TIERS = default
    for v, t in times.items():
        print(json.dumps({"bench": f"{name} kernel {shape}", "tier": v,
                          "calls": calls,
                          "median_ms": round(float(np.median(t)), 4),
                          "min_ms": round(float(np.min(t)), 4),
                          "max_ms": round(float(np.max(t)), 4)}), flush=True)


SLAB_SHAPES = {"256x1": (256, 0), "256x2": (512, 1), "256x4": (1024, 2),
               "256x8": (2048, 3)}


def slab_shapes(name, shape, info, preds, calls, warmup):
    """The slab tier with each block shape, alternated."""
    default = gpu_backend.LAMBDARANK_SLAB
    objs = {}
    try:
        for v, sl in SLAB_SHAPES.items():
            gpu_backend.LAMBDARANK_SLAB = sl
            objs[v] = create_objective(name)
            _call(objs[v], preds, info, "1")  # builds the state
    finally:
        gpu_backend.LAMBDARANK_SLAB = default
    times = {v: [] for v in objs}
    for i in range(warmup + calls):
        for v, obj in objs.items():
            ms, _ = _call(obj, preds, info, "1")
            if i >= warmup:
                times[v].append(ms)
    for v, t in times.items():
        _report(f"{name} kernel {shape}", {"slab": v}, t, calls)


def slab_mode(y, ybin, preds, calls, warmup):
    names = ("rank:ndcg", "rank:map", "rank:pairwise")
    saved = gpu_backend.LAMBDARANK_MAX_GROUP
    gpu_backend.LAMBDARANK_MAX_GROUP = 1 << 18
    try:
        for m in (12, 14, 16, 18):
            n = 1 << m
            for name in names:
                lab = ybin if name == "rank:map" else y
                ab(name, f"one group 2^{m}", _info(lab[:n], [n]),
                   preds[:n].contiguous(), calls, warmup)
        for m in (12, 16):
            n = 1 << m
            for name in ("rank:ndcg", "rank:map"):
                lab = ybin if name == "rank:map" else y
                slab_shapes(name, f"one group 2^{m}", _info(lab[:n], [n]),
                            preds[:n].contiguous(), calls, warmup)
    finally:
        gpu_backend.LAMBDARANK_MAX_GROUP = saved
    n = preds.shape[0]
    n100 = (n - 2 * 4096) // 100
    sizes_m = np.full(n100 + 2, 100)
    sizes_m[[n100 // 3, 2 * n100 // 3]] = 4096
    nm = int(sizes_m.sum())
    for name in names:
        lab = ybin if name == "rank:map" else y
        ab(name, "m", _info(lab[:nm], sizes_m), preds[:nm].contiguous(),
           calls, warmup)
        ab(name, "m, groups of 100 alone", _info(lab[:n100 * 100],
                                                 np.full(n100, 100)),
           preds[:n100 * 100].contiguous(), calls, warmup)
    slab_shapes("rank:ndcg", "m", _info(y[:nm], sizes_m),
                preds[:nm].contiguous(), calls, warmup)


def _report(bench, extra, t, calls):
    t = np.asarray(t)
    print(json.dumps(dict({"bench": bench}, **extra, calls=calls,
                          median_ms=round(float(np.median(t)), 4),
                          min_ms=round(float(t.min()), 4),
                          max_ms=round(float(t.max()), 4))), flush=True)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def metrics_ab(bst, shape, d, calls, warmup):
    """Booster.eval_set per call (margin cached), the ranking-metric kernel
    (XGB_AMD_RANK_METRIC_HIP=1) against the host loop (=0), alternated."""
    for metric in ("ndcg", "map@10", "pre@10"):
        bst.set_param("eval_metric", metric)
        times, outs = {"1": [], "0": []}, {}
        for i in range(warmup + calls):
            for flag in ("1", "0"):
                os.environ["XGB_AMD_RANK_METRIC_HIP"] = flag
                ms, outs[flag] = _timed(lambda: bst.eval_set([(d, "e")]))
                if i >= warmup:
                    times[flag].append(ms)
        os.environ.pop("XGB_AMD_RANK_METRIC_HIP")
        for flag, path in (("1", "hip"), ("0", "host")):
            _report(f"eval_set {metric} {shape}",
                    {"path": path, "value": outs[flag].split(":")[-1]},
                    times[flag], calls)


def _metric_kernel_times(variants, info, scores, kinds, calls, warmup):
    """rank_metric_gpu alone per (block shape, metric), alternated."""
    states = {v: gpu_backend.RankMetricState(
        info.labels, info.group_ptr, scores.device, block)
        for v, block in variants.items()}
    times = {(v, k): [] for v in variants for k in kinds}
    for i in range(warmup + calls):
        for v, state in states.items():
            for k in kinds:
                ms, _ = _timed(lambda: gpu_backend.rank_metric_gpu(
                    scores, state, k, 10, False))
                if i >= warmup:
                    times[(v, k)].append(ms)
    return times


METRIC_SHAPES = {"256x8 tile 1024": (2048, 1), "256x4 tile 1024": (1024, 2),
                 "512x4 tile 1024": (2048, 3), "256x8 tile 256": (2048, 4)}


def metric_shapes(shape, info, scores, calls, warmup):
    """The metric kernel with each alternative block shape."""
    times = _metric_kernel_times(METRIC_SHAPES, info, scores,
                                 ("ndcg", "map"), calls, warmup)
    for (v, k), t in times.items():
        _report(f"rank_metric_gpu {k}@10 {shape}", {"block": v}, t, calls)


def metric_cap(calls, warmup, lo=12, hi=21):
    """One group of 2^m documents: the kernel against the host path for the
    same group (device-to-host copy + stable argsort), per metric."""
    rng = np.random.RandomState(5)
    saved = gpu_backend.RANK_METRIC_MAX_GROUP
    gpu_backend.RANK_METRIC_MAX_GROUP = 1 << hi
    try:
        for m in range(lo, hi + 1):
            n = 1 << m
            info = _info(rng.randint(0, 2, n).astype(np.float32), [n])
            scores = torch.from_numpy(rng.randn(n).astype(np.float32)).cuda()
            c = max(3, calls // (1 + max(0, m - 15) * 4))
            times = _metric_kernel_times(
                {"256x8 tile 1024": (2048, 1), "256x4 tile 1024": (1024, 2)},
                info, scores, ("ndcg", "map"), c, warmup)
            for (v, k), t in times.items():
                _report(f"one group 2^{m} {k}@10", {"path": "hip " + v}, t, c)
            host = []
            for i in range(warmup + c):
                ms, _ = _timed(lambda: np.argsort(
                    -scores.cpu().numpy().astype(np.float64), kind="stable"))
                if i >= warmup:
                    host.append(ms)
            _report(f"one group 2^{m}", {"path": "host copy+argsort"}, host, c)
    finally:
        gpu_backend.RANK_METRIC_MAX_GROUP = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiers", action="store_true")
    ap.add_argument("--metrics", action="store_true")
    ap.add_argument("--slab", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"

    rng = np.random.RandomState(7)
    n, f = args.docs, 28
    X = rng.randn(n, f).astype(np.float32)
    y = np.clip((X[:, 0] * 2 + 2).astype(int), 0, 4).astype(np.float32)
    sizes_a = np.full(n // 100, 100)
    d = xgb.DMatrix(X, label=y, qid=np.repeat(np.arange(n // 100), 100))
    bst = xgb.train({"objective": "rank:ndcg", "max_depth": 6,
                     "max_bin": 256, "eta": 0.3, "device": "cuda",
                     "seed": 7}, d, args.rounds, verbose_eval=False)
    margin = np.asarray(bst.predict(d, output_margin=True), np.float32)
    preds = torch.from_numpy(margin).cuda().view(-1, 1)

    sizes_b = np.clip(np.random.RandomState(11).lognormal(4.0, 1.0, n),
                      1, 1251).astype(np.int64)
    sizes_b = sizes_b[:int(np.searchsorted(np.cumsum(sizes_b), n))]
    nb = int(sizes_b.sum())
    shapes = {"a": (_info(y, sizes_a), preds),
              "b": (_info(y[:nb], sizes_b), preds[:nb].contiguous())}
    ybin = (y >= 2).astype(np.float32)

    if args.metrics:
        metrics_ab(bst, "a", d, args.calls, args.warmup)
        nc = 61 * 16384
        shapes["c"] = (_info(y[:nc], np.full(61, 16384)),
                       preds[:nc].contiguous())
        for shape in ("b", "c"):
            info, p = shapes[shape]
            metric_shapes(shape, info, p.view(-1), args.calls, args.warmup)
        metric_cap(args.calls, args.warmup)
        return
    if args.slab:
        slab_mode(y, ybin, preds, args.calls, args.warmup)
        return
    for name in ("rank:ndcg", "rank:map", "rank:pairwise"):
        info = _info(ybin, sizes_a) if name == "rank:map" else shapes["a"][0]
        ab(name, "a", info, preds, args.calls, args.warmup)
    ab("rank:ndcg", "b", *shapes["b"], args.calls, args.warmup)
    if args.tiers:
        for shape, (info, p) in shapes.items():
            tiers("rank:ndcg", shape, info, p, args.calls, args.warmup)


if __name__ == "__main__":
    main()
