"""Ranking-metric HIP kernel (ops/cpp/rank_metric.hip) against the numpy
metrics of metrics.py, which tests/test_ranking.py and test_metrics.py pin.

Tolerance 1e-12 absolute: both sides sum in fp64, every group value is at
most 1, and the worst-case reordering bound n * 2^-53 is under 1e-12 at
these group sizes.  A misranked document moves the value by far more."""
import numpy as np
import pytest
import torch

import xgboost_amd as xgb
from xgboost_amd.backend import gpu
from xgboost_amd.backend.gpu import RANK_METRIC_SLAB as S
from xgboost_amd.data import MetaInfo
from xgboost_amd.metrics import create_metric

# empty group, singleton, both sides of k = 5 and 32, of the wave (64), of
# one slab, and a group of three slabs with a ragged last one
LAYOUT = [1, 2, 5, 33, 64, 65, 257, 600, 0, 3, S, S + 1, 2 * S + 403]
PARAMS = [None, "1", "5", "32", "32-", "5000"]
CASES = [(m, p) for m in ("ndcg", "map", "pre") for p in PARAMS
         if not (m == "pre" and p == "32-")]


def _info(layout, binary, tied=False):
    """(MetaInfo, fp32 CPU scores) of a group layout."""
    rng = np.random.RandomState(0)
    info = MetaInfo()
    info.num_row = int(sum(layout))
    info.group_ptr = np.concatenate([[0], np.cumsum(layout)]).astype(np.int64)
    y = rng.randint(0, 2 if binary else 5, info.num_row)
    if len(layout) > 3:
        y[info.group_ptr[3]:info.group_ptr[4]] = 0  # no relevant document
    info.labels = y.astype(np.float32)
    p = np.random.RandomState(1).randn(info.num_row).round(1)
    return info, torch.tensor(np.full_like(p, 0.5) if tied else p,
                              dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("metric,param", CASES)
def test_values(metric, param, tied):
    info, p = _info(LAYOUT, metric != "ndcg", tied)
    m = create_metric(metric if param is None else f"{metric}@{param}")
    assert abs(m(p.cuda(), info) - m(p.numpy(), info)) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("kind,topn", [("ndcg", 5), ("map", 2 ** 31 - 1),
                                       ("pre", 3)])
def test_per_group(kind, topn):
    info, p = _info(LAYOUT, kind != "ndcg")
    y, gp = info.labels.astype(np.float64), info.group_ptr
    ref = []
    for s, e in zip(gp[:-1], gp[1:]):
        order = np.argsort(-p.numpy()[s:e].astype(np.float64), kind="stable")
        k, yr = min(topn, e - s), y[s:e][order]
        if kind == "pre":
            ref.append(float((yr[:k] > 0).sum()))
        elif not (yr > 0).any():
            ref.append(1.0)
        elif kind == "map":
            rel = yr > 0
            ref.append(float((rel * np.cumsum(rel) / np.arange(1, e - s + 1))
                             [:k].sum() / rel.sum()))
        else:
            disc = 1.0 / np.log2(np.arange(2, e - s + 2))
            ref.append(float(((2.0 ** yr - 1) * disc)[:k].sum() /
                             ((2.0 ** np.sort(yr)[::-1] - 1) * disc)[:k].sum()))
    state = gpu.rank_metric_state(info, torch.device("cuda", 0))
    got = gpu.rank_metric_gpu(p.cuda(), state, kind, topn, False)
    assert got.dtype == torch.float64 and got.is_cuda
    assert np.abs(got.cpu().numpy() - np.asarray(ref)).max() <= 1e-12
    assert torch.equal(got, gpu.rank_metric_gpu(p.cuda(), state, kind, topn,
                                                False))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["oversized", "fp64", "env"])
def test_dispatch(case, monkeypatch):
    calls = []
    monkeypatch.setattr(gpu, "rank_metric_gpu",
                        lambda *a, **k: calls.append(a))
    info, p = _info([gpu.RANK_METRIC_MAX_GROUP + 1] if case == "oversized"
                    else LAYOUT, False)
    if case == "env":
        monkeypatch.setenv("XGB_AMD_RANK_METRIC_HIP", "0")
    dev = p.cuda().double() if case == "fp64" else p.cuda()
    for name in ("ndcg@5", "map", "pre@3"):
        m = create_metric(name)
        assert m(dev, info) == m(p.numpy(), info)
    assert not calls


@pytest.mark.gpu
def test_train_evals_result(monkeypatch):
    rng = np.random.RandomState(3)
    X = rng.randn(400, 6).astype(np.float32)
    y = np.clip((X[:, 0] * 2 + 2).astype(int), 0, 4).astype(np.float32)
    qid = np.repeat(np.arange(8), 50)
    results = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("XGB_AMD_RANK_METRIC_HIP", flag)
        d = xgb.DMatrix(X, label=y, qid=qid)
        results[flag] = {}
        xgb.train({"objective": "rank:ndcg", "device": "cuda", "max_depth": 3,
                   "eval_metric": ["ndcg@5", "map", "pre@3"], "seed": 0}, d,
                  3, evals=[(d, "train")], evals_result=results[flag],
                  verbose_eval=False)
    assert list(results["1"]["train"]) == ["ndcg@5", "map", "pre@3"]
    for name, vals in results["1"]["train"].items():
        assert len(vals) == 3
        assert np.abs(np.subtract(vals, results["0"]["train"][name])).max() \
            <= 1e-5


def test_schedule():
    s = gpu.rank_metric_schedule(np.concatenate([[0], np.cumsum(LAYOUT)]))
    assert s["eligible"] and s["max_group"] == 2 * S + 403
    assert s["wave"].tolist() == [0, 1, 2, 3, 4, 9]
    assert s["block"].tolist() == [
        [12, 0], [12, S], [12, 2 * S], [11, 0], [11, S], [10, 0], [7, 0],
        [6, 0], [5, 0]]
    assert s["part_off"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 10,
                                      12, 15]
    assert not gpu.rank_metric_schedule(
        np.array([0, 3, 3 + gpu.RANK_METRIC_MAX_GROUP + 1]))["eligible"]
