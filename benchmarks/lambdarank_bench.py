#!/usr/bin/env python
"""LambdaMART get_gradient alone on 1 MI355X: the HIP kernel
(XGB_AMD_RANK_HIP=1) against the torch formulation (=0), alternated call
by call in one process, device-synchronised.  One JSON line per
measurement (median / min / max in ms) and one per output comparison.

Shape (a): 1M documents in 10k groups of 100, feature_bench.py's labels,
scores from a few boosting rounds.  Shape (b): about 1M documents in
seeded log-normal group sizes clipped to 1..1251, same scores.
--tiers also times the kernel's alternative block shapes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiers", action="store_true")
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

    for name in ("rank:ndcg", "rank:map", "rank:pairwise"):
        info = _info(ybin, sizes_a) if name == "rank:map" else shapes["a"][0]
        ab(name, "a", info, preds, args.calls, args.warmup)
    ab("rank:ndcg", "b", *shapes["b"], args.calls, args.warmup)
    if args.tiers:
        for shape, (info, p) in shapes.items():
            tiers("rank:ndcg", shape, info, p, args.calls, args.warmup)


if __name__ == "__main__":
    main()
