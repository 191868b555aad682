#!/usr/bin/env python
"""Multiclass softmax on 1 MI355X, one JSON line per measurement.

Rounds: multi:softprob, 1M x 28, depth 8, K = 7; Booster.update per round,
the fused path (ops/cpp/softmax_gpair.hip) against the generic chain
(XGB_AMD_FUSED_MULTI=0), one fresh booster per run, run in the order
fused, generic, generic, fused; a host clock around the timed rounds, which
end in a device synchronise.

Gradient step alone (--grad): at 1M rows and K in 3, 7, 64, 256, the
kernel with every block shape that serves K, the kernel plus the batched
quantise, and SoftmaxMulti.get_gradient on the same margin (the torch chain
the kernel replaces, without the per-class quantise that follows it on the
generic path); alternated call by call, median / min / max in ms, and the
kernel's achieved bytes/s over the 12 n K bytes it has to move."""
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


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _report(bench, extra, t, **more):
    t = np.asarray(t)
    print(json.dumps(dict({"bench": bench}, **extra, calls=len(t),
                          median_ms=round(float(np.median(t)), 4),
                          min_ms=round(float(t.min()), 4),
                          max_ms=round(float(t.max()), 4), **more)),
          flush=True)


def grad_step(n, K, calls, warmup):
    g = torch.Generator().manual_seed(K)
    margin = (torch.randn(n, K, generator=g) * 2).cuda()
    y = torch.randint(0, K, (n,), generator=g).float()
    info = MetaInfo()
    info.labels = y.numpy()
    labels = y.cuda()
    gh = torch.empty((K, n, 2), dtype=torch.float32, device="cuda")
    qg = torch.empty((K, n, 2), dtype=torch.int32, device="cuda")
    maxabs = torch.zeros((K, 2), dtype=torch.float32, device="cuda")
    sums = torch.zeros((K, 2), dtype=torch.int64, device="cuda")
    obj = create_objective("multi:softprob", {"num_class": K})

    def kernel(shape):
        maxabs.zero_()
        gpu_backend.softmax_gpair_gpu(margin, labels, None, gh, maxabs, shape)

    def kernel_quantize():
        kernel(-1)
        sums.zero_()
        gpu_backend.quantize_planes_gpu(gh, maxabs, qg, sums)

    variants = {f"kernel shape {s}": (lambda s=s: kernel(s))
                for s, cap in gpu_backend.SOFTMAX_GPAIR_SHAPES.items()
                if cap >= K}
    variants["kernel + quantise"] = kernel_quantize
    variants["torch get_gradient"] = lambda: obj.get_gradient(margin, info, 0)
    times = {v: [] for v in variants}
    for i in range(warmup + calls):
        for v, fn in variants.items():
            ms = _timed(fn)
            if i >= warmup:
                times[v].append(ms)
    for v, t in times.items():
        more = {}
        if v.startswith("kernel shape"):
            more["gbytes_per_s"] = round(12.0 * n * K / np.median(t) / 1e6, 1)
        _report(f"gradient step n={n} K={K}", {"variant": v}, t, **more)


def rounds(n, K, depth, steps, warmup):
    rng = np.random.RandomState(7)
    X = rng.randn(n, 28).astype(np.float32)
    y = (X[:, :8] @ rng.randn(8, K) + 0.5 * rng.randn(n, K)).argmax(axis=1)
    d = xgb.DMatrix(X, label=y.astype(np.float32))
    params = {"objective": "multi:softprob", "num_class": K,
              "max_depth": depth, "max_bin": 256, "eta": 0.1,
              "tree_method": "hist", "device": "cuda", "seed": 7}
    for flag in ("1", "0", "0", "1"):
        os.environ["XGB_AMD_FUSED_MULTI"] = flag
        bst = xgb.Booster(params, cache=[d])
        for it in range(warmup):
            bst.update(d, it)
        ms = _timed(lambda: [bst.update(d, warmup + i) for i in range(steps)])
        assert hasattr(bst, "_fused_cache") == (flag == "1")
        from xgboost_amd.metrics import create_metric
        loss = float(create_metric("mlogloss")(bst.predict(d), d.info))
        print(json.dumps({"bench": f"rounds n={n} K={K} depth={depth}",
                          "path": "fused" if flag == "1" else "generic",
                          "steps": steps, "warmup": warmup,
                          "rounds_per_s": round(steps / ms * 1e3, 3),
                          "ms_per_round": round(ms / steps, 3),
                          "train_mlogloss": round(loss, 6)}), flush=True)
    os.environ.pop("XGB_AMD_FUSED_MULTI")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--grad", action="store_true",
                    help="time the gradient step alone instead of rounds")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    if args.grad:
        for K in (3, 7, 64, 256):
            grad_step(args.rows, K, args.calls, args.warmup)
    else:
        rounds(args.rows, args.classes, args.max_depth, args.steps,
               args.warmup)


if __name__ == "__main__":
    main()
