"""Multiclass softmax on the fused path: ops/cpp/softmax_gpair.hip against
numpy fp64, the batched quantise against torch, and the driver end to end.

Measured on one MI355X, largest absolute error against fp64 over the
kernel cases below: kernel g 2.06e-07, h 3.76e-07; the torch fp32 chain g
2.68e-07, h 5.18e-07 (per K in profiles/multiclass_mi355x.md)."""
import numpy as np
import pytest
import torch

import xgboost_amd as xgb
from xgboost_amd.backend.gpu import (SOFTMAX_GPAIR_SHAPES,
                                     quantize_planes_gpu,
                                     softmax_gpair_gpu,
                                     softmax_gpair_max_classes)
from xgboost_amd.data import MetaInfo
from xgboost_amd.objectives import create_objective

pytestmark = pytest.mark.gpu

R_MAX = 256  # rows per tile of the small-K shapes, the largest tile
# both sides of the lanes-per-row tier edges at K = 16 and K = 64, the cap
KS = [2, 3, 16, 17, 64, 65, 256]
NS = [1, R_MAX - 1, 2 * R_MAX + 3]


def _ref(x, y, w):
    """SoftmaxMulti.get_gradient in fp64: planes [K, n, 2]."""
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    g = p.copy()
    g[np.arange(len(y)), y.astype(np.int64)] -= 1.0
    h = np.maximum(2.0 * p * (1.0 - p), 1e-16)
    gh = np.stack([g, h], axis=2) * w.astype(np.float64)[:, None, None]
    return gh.transpose(1, 0, 2)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_kernel_matches_fp64(K, n, weighted):
    rng = np.random.RandomState(K * 1000 + n)
    x = (rng.randn(n, K) * 5).astype(np.float32)
    x[0, 0] = 80.0
    x[3 % n, K - 1] = -80.0
    x[5 % n] = 1.25
    y = rng.randint(0, K, n).astype(np.float32)
    y[0], y[-1] = 0, K - 1
    # at most 1, so that no output exceeds the 1.0 the floor below is for
    w = (rng.uniform(0.25, 1.0, n).astype(np.float32) if weighted
         else np.ones(n, np.float32))
    ref = _ref(x, y, w)

    dev = torch.device("cuda")
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    wd = torch.tensor(w, device=dev) if weighted else None
    info = MetaInfo()
    info.labels, info.weights = y, (w if weighted else None)
    g, h = create_objective("multi:softprob", {"num_class": K}).get_gradient(
        xd, info, 0)
    chain = torch.stack([g, h], dim=2).permute(1, 0, 2).cpu().double().numpy()
    chain_err = np.abs(chain - ref).max(axis=(0, 1))

    cap = min(c for c in SOFTMAX_GPAIR_SHAPES.values() if c >= K)
    for shape in [-1] + [s for s, c in SOFTMAX_GPAIR_SHAPES.items()
                         if c == cap]:
        gh = torch.full((K, n, 2), float("nan"), device=dev)
        maxabs = torch.zeros((K, 2), device=dev)
        softmax_gpair_gpu(xd, yd, wd, gh, maxabs, shape)
        err = np.abs(gh.cpu().double().numpy() - ref).max(axis=(0, 1))
        print(f"K={K} n={n} w={weighted} shape={shape} kernel g/h "
              f"{err[0]:.3e} {err[1]:.3e} chain g/h {chain_err[0]:.3e} "
              f"{chain_err[1]:.3e}")
        assert np.all(err <= 2.0 * chain_err + 2.0 ** -24), (err, chain_err)
        assert torch.equal(maxabs, gh.abs().amax(dim=1))
        gh2 = torch.empty_like(gh)
        softmax_gpair_gpu(xd, yd, wd, gh2, torch.zeros_like(maxabs), shape)
        assert torch.equal(gh, gh2)


@pytest.mark.parametrize("K", [2, 5])
def test_quantize_planes_exact(K):
    n = 1500
    gh = torch.randn((K, n, 2), generator=torch.Generator().manual_seed(K))
    gh[..., 1].abs_()
    gh[1, :, 1] = 0.0  # an all-zero hessian plane: scale 1
    gh = gh.cuda()
    maxabs = gh.abs().amax(dim=1)
    qg = torch.empty((K, n, 2), dtype=torch.int32, device=gh.device)
    sums = torch.zeros((K, 2), dtype=torch.int64, device=gh.device)
    quantize_planes_gpu(gh, maxabs, qg, sums)
    m = maxabs.double()
    scale = torch.where(m > 0, 2.0 ** 30 / m, torch.ones_like(m))
    want = torch.round(gh.double() * scale[:, None, :]).int()
    assert torch.equal(qg, want)
    assert torch.equal(sums, want.long().sum(dim=1))


def _train(K, rounds=8, n=10000, weight=None, **extra):
    rng = np.random.RandomState(K)
    X = rng.randn(n, 8).astype(np.float32)
    y = (X @ rng.randn(8, K)).argmax(axis=1).astype(np.float32)
    d = xgb.DMatrix(X, label=y, weight=weight)
    res = {}
    bst = xgb.train(dict({"objective": "multi:softprob", "num_class": K,
                          "device": "cuda", "max_depth": 4,
                          "eval_metric": "mlogloss"}, **extra), d, rounds,
                    evals=[(d, "t")], evals_result=res, verbose_eval=False)
    return bst, res["t"]["mlogloss"][-1]


@pytest.mark.parametrize("K", [3, 5])
def test_train_fused_matches_generic(K):
    b1, loss1 = _train(K)
    assert hasattr(b1, "_fused_cache"), "fused path was not taken"
    b2, loss2 = _train(K, subsample=0.9999999)
    assert not hasattr(b2, "_fused_cache")
    print(f"K={K} mlogloss fused {loss1:.6f} generic {loss2:.6f}")
    assert abs(loss1 - loss2) < 0.01
    assert len(b1.trees) == 8 * K
    assert list(b1.tree_info) == list(range(K)) * 8
    assert list(b1.iteration_indptr) == list(range(0, 8 * K + 1, K))
    assert b1.get_dump() == _train(K)[0].get_dump()
    w = np.random.RandomState(0).rand(10000).astype(np.float32) + 0.5
    b3, loss3 = _train(K, weight=w)
    assert hasattr(b3, "_fused_cache")
    assert abs(loss3 - _train(K, weight=w, subsample=0.9999999)[1]) < 0.01


@pytest.mark.parametrize("how", ["above_cap", "opt_out"])
def test_fallback_to_generic_path(how, monkeypatch):
    K = 3
    if how == "above_cap":
        K = softmax_gpair_max_classes() + 1
    else:
        monkeypatch.setenv("XGB_AMD_FUSED_MULTI", "0")
    bst, loss = _train(K, rounds=2, n=600, max_depth=2)
    assert not hasattr(bst, "_fused_cache")
    assert len(bst.trees) == 2 * K and np.isfinite(loss)
