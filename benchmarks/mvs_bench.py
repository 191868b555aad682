#!/usr/bin/env python
"""Gradient-based (MVS) sampling on 1 MI355X, one JSON line per measurement.

Sampling step alone (--step): Booster._subsample on [n, 2] device gradients
at subsample 0.1 and 0.5, the device path (ops/cpp/mvs_sample.hip) against
the host path (XGB_AMD_MVS_HIP=0), alternated call by call, on two score
shapes: "spread", the gradients of a binary:logistic model after a few
rounds, and "constant", the same model's gradients before its first round
(every score equal, the worst case for an LDS histogram).  Median / min /
max in ms of a host clock around a call that ends in a device synchronise;
for the device path also the bytes/s over the 40 n bytes its four launches
have to move (four reads and one write of the 8-byte pairs).

Rounds (default): binary:logistic, n x 28, depth 8, gradient_based with
subsample 0.5; Booster.update per round, one fresh booster per run, in the
order device, host, host, device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xgboost_amd as xgb  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _data(n):
    rng = np.random.RandomState(7)
    X = rng.randn(n, 28).astype(np.float32)
    y = (X[:, :8] @ rng.randn(8) + rng.randn(n) > 0).astype(np.float32)
    return xgb.DMatrix(X, label=y), y


def _params(subsample):
    return {"objective": "binary:logistic", "max_depth": 8, "max_bin": 256,
            "eta": 0.1, "tree_method": "hist", "device": "cuda", "seed": 7,
            "subsample": subsample, "sampling_method": "gradient_based"}


def step(n, calls, warmup, trained_rounds):
    d, y = _data(n)
    yd = torch.as_tensor(y, device="cuda")
    gpairs = {}
    for shape, rounds in (("constant", 0), ("spread", trained_rounds)):
        margin = torch.zeros(n, device="cuda")
        if rounds:
            bst = xgb.train(dict(_params(1.0), base_score=0.5), d, rounds,
                            verbose_eval=False)
            margin = torch.as_tensor(bst.predict(d, output_margin=True),
                                     device="cuda").view(-1)
        p = torch.sigmoid(margin)
        gpairs[shape] = torch.stack([p - yd, p * (1 - p)], dim=1).contiguous()
    for shape, gpair in gpairs.items():
        for subsample in (0.1, 0.5):
            bst = xgb.Booster(_params(subsample), cache=[d])
            times = {"device": [], "host": []}
            for i in range(warmup + calls):
                for path in times:
                    os.environ["XGB_AMD_MVS_HIP"] = "1" if path == "device" \
                        else "0"
                    ms = _timed(lambda: bst._subsample(gpair, 1000 + i))
                    if i >= warmup:
                        times[path].append(ms)
            for path, t in times.items():
                t = np.asarray(t)
                more = ({"gbytes_per_s": round(40.0 * n / np.median(t) / 1e6, 1)}
                        if path == "device" else {})
                print(json.dumps(dict(
                    {"bench": f"sampling step n={n}", "scores": shape,
                     "subsample": subsample, "path": path, "calls": len(t),
                     "median_ms": round(float(np.median(t)), 4),
                     "min_ms": round(float(t.min()), 4),
                     "max_ms": round(float(t.max()), 4)}, **more)),
                    flush=True)
    os.environ.pop("XGB_AMD_MVS_HIP")


def rounds(n, steps, warmup):
    d, y = _data(n)
    for flag in ("1", "0", "0", "1"):
        os.environ["XGB_AMD_MVS_HIP"] = flag
        bst = xgb.Booster(_params(0.5), cache=[d])
        for it in range(warmup):
            bst.update(d, it)
        ms = _timed(lambda: [bst.update(d, warmup + i) for i in range(steps)])
        assert hasattr(bst, "_fused_cache") == (flag == "1")
        p = np.clip(bst.predict(d).astype(np.float64), 1e-12, 1 - 1e-12)
        loss = float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean())
        print(json.dumps({"bench": f"rounds n={n} depth=8 subsample=0.5",
                          "path": "device" if flag == "1" else "host",
                          "steps": steps, "warmup": warmup,
                          "rounds_per_s": round(steps / ms * 1e3, 3),
                          "ms_per_round": round(ms / steps, 3),
                          "train_logloss": round(loss, 6)}), flush=True)
    os.environ.pop("XGB_AMD_MVS_HIP")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--trained-rounds", type=int, default=20)
    ap.add_argument("--step", action="store_true",
                    help="time the sampling step alone instead of rounds")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    if args.step:
        step(args.rows, args.calls, args.warmup, args.trained_rounds)
    else:
        rounds(args.rows, args.steps, args.warmup)


if __name__ == "__main__":
    main()
