"""Gradient-based (MVS) sampling on the device: ops/cpp/mvs_sample.hip
against a sort-based numpy fp64 solution of the definition, the apply step
with pinned draws, the device generator, and training end to end.

Measured on one MI355X: largest relative threshold error 3.3e-16 on the
exact inputs and 0 on the general ones; train logloss, device path against
opt-out, mean of five seeds 0.16533 against 0.16627, opt-out spread 0.00281
(profiles/mvs_mi355x.md)."""
import math

import numpy as np
import pytest
import torch

import xgboost_amd as xgb
from conftest import make_classification
from xgboost_amd.backend.gpu import mvs_sample_gpu

pytestmark = pytest.mark.gpu

FLT_MIN = float(np.finfo(np.float32).tiny)
N_BIG = 512 * 256 + 5  # past the 512-block grid-stride edge
NS = [1, 63, 257, N_BIG]
SUBS = [0.1, 0.5, 0.9]


def _ref_threshold(s, target):
    """u with sum(min(1, s/u)) == target by sorting; 0 when at most
    `target` scores are positive.  Scores below FLT_MIN count as zero."""
    s = np.sort(np.where(s < FLT_MIN, 0.0, s).astype(np.float64))
    n = len(s)
    if np.count_nonzero(s) <= target:
        return 0.0
    below = np.concatenate([[0.0], np.cumsum(s)])[:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (n - np.arange(n)) + np.where(s > 0, below / s, np.inf)
    k = int(np.count_nonzero(f > target))  # rows strictly below u
    return math.fsum(s[:k]) / (target - (n - k))


def _log_uniform(rng, n, sub):
    return np.exp2(rng.uniform(-15, 15, n))


def _all_equal(rng, n, sub):
    return np.full(n, 0.3)


def _two_values(rng, n, sub):  # 5 % large: the root lies between the two
    g = np.ones(n)
    g[:n // 20] = 1000.0
    return rng.permutation(g)


def _mostly_zero(rng, n, sub):  # fewer positive rows than the target
    g = np.zeros(n)
    g[:int(sub * n / 2)] = rng.uniform(0.5, 2.0, int(sub * n / 2))
    return rng.permutation(g)


def _low_bits(rng, n, sub):  # equal but for the last 10 significand bits
    return (np.uint32(0x3F800000)
            + rng.randint(0, 1024, n).astype(np.uint32)).view(np.float32)


def _with_subnormals(rng, n, sub):
    g = _log_uniform(rng, n, sub)
    idx = rng.choice(n, min(n, 5), replace=False)
    g[idx] = [1e-39, 1e-42, 5e-39, 1e-40, 1e-45][:len(idx)]
    return g


CASES = [_log_uniform, _all_equal, _two_values, _mostly_zero, _low_bits,
         _with_subnormals]


def _sample(gh, sub, lam, seed=0, **kw):
    out, u = mvs_sample_gpu(torch.tensor(gh, device="cuda"), sub, lam, seed,
                            **kw)
    return out.cpu().numpy(), float(u.cpu())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__.strip("_"))
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("n", NS)
def test_threshold_exact_inputs(n, sub, case):
    rng = np.random.RandomState(n % 1000 + int(sub * 10))
    g = case(rng, n, sub).astype(np.float32) * rng.choice([-1, 1], n)
    gh = np.stack([g, np.zeros(n)], axis=1).astype(np.float32)
    ref = _ref_threshold(np.abs(g), sub * n)  # h = 0, lambda = 0: s = |g|
    out, u = _sample(gh, sub, 0.0)
    _, u2 = _sample(gh, sub, 0.0)
    print(f"u {u!r} ref {ref!r} rel {abs(u - ref) / max(ref, 1e-300):.3e}")
    assert np.float64(u).tobytes() == np.float64(u2).tobytes()
    if ref == 0.0:
        # no root: positive rows come back unscaled, the rest is dropped
        assert u == 0.0
        assert np.array_equal(
            out, np.where(np.abs(gh) < FLT_MIN, np.float32(0), gh))
    else:
        assert abs(u - ref) <= 1e-12 * ref


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("n", [257, N_BIG])
def test_threshold_general_inputs(n, sub):
    rng = np.random.RandomState(n)
    gh = rng.randn(n, 2).astype(np.float32)
    s = np.sqrt(gh[:, 0] * gh[:, 0] + np.float32(1.0) * (gh[:, 1] * gh[:, 1]))
    ref = _ref_threshold(s, sub * n)
    _, u = _sample(gh, sub, 1.0)
    print(f"u {u!r} ref {ref!r} rel {abs(u - ref) / ref:.3e}")
    assert abs(u - ref) <= 1e-5 * ref


@pytest.mark.parametrize("n", [257, N_BIG])
def test_apply_pinned_draws(n):
    rng = np.random.RandomState(n)
    gh = rng.randn(n, 2).astype(np.float32)
    lam, sub = np.float32(1.0), 0.5
    s = np.sqrt(gh[:, 0] * gh[:, 0] + lam * (gh[:, 1] * gh[:, 1]))
    _, u = _sample(gh, sub, lam)
    kp = np.minimum(np.float32(1.0), s / np.float32(u))
    want = rng.rand(n) < 0.5
    rand = np.where(want, kp / 2, kp + np.float32(0.25)).astype(np.float32)
    assert np.all(np.abs(rand - kp) > 2.0 ** -23)  # nothing to exclude
    keep = rand < kp

    ghd = torch.tensor(gh, device="cuda")
    maxabs = torch.zeros(2, device="cuda")
    out_d, u_d = mvs_sample_gpu(ghd, sub, lam, 0, maxabs=maxabs,
                                rand=torch.tensor(rand, device="cuda"))
    out = out_d.cpu().numpy()
    assert float(u_d.cpu()) == u
    assert np.array_equal(np.any(out != 0, axis=1), keep)
    assert np.all(out[~keep] == 0)
    exact = gh.astype(np.float64) / kp.astype(np.float64)[:, None]
    err = np.abs(out[keep] - exact[keep])
    assert np.all(err <= 4 * np.spacing(np.abs(exact[keep]).astype(np.float32)))
    assert np.array_equal(maxabs.cpu().numpy(), np.abs(out).max(axis=0))
    # in place
    mvs_sample_gpu(ghd, sub, lam, 0, out=ghd,
                   rand=torch.tensor(rand, device="cuda"))
    assert torch.equal(ghd, out_d)


def test_generator():
    n, sub = N_BIG, 0.5
    rng = np.random.RandomState(7)
    gh = (rng.randn(n, 2) * np.exp2(rng.uniform(-3, 3, (n, 1)))).astype(
        np.float32)
    s = np.sqrt(gh[:, 0] * gh[:, 0] + np.float32(1.0) * (gh[:, 1] * gh[:, 1]))
    out, u = _sample(gh, sub, 1.0, seed=11)
    kept = np.any(out != 0, axis=1)
    assert np.array_equal(kept, np.any(_sample(gh, sub, 1.0, seed=11)[0] != 0,
                                       axis=1))
    assert not np.array_equal(
        kept, np.any(_sample(gh, sub, 1.0, seed=12)[0] != 0, axis=1))
    kp = np.minimum(1.0, s.astype(np.float64) / np.float32(u))
    # the whole range, then its quarters: no period in the row index
    for part in [slice(None)] + [slice(q * n // 4, (q + 1) * n // 4)
                                 for q in range(4)]:
        p = kp[part]
        assert abs(kept[part].sum() - p.sum()) <= 6 * np.sqrt(
            (p * (1 - p)).sum())


def _logloss(bst, d, y):
    p = np.clip(bst.predict(d).astype(np.float64), 1e-12, 1 - 1e-12)
    if p.ndim == 2:
        return float(-np.log(p[np.arange(len(y)), y.astype(int)]).mean())
    return float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean())


def test_training_binary_fused(monkeypatch):
    X, y = make_classification(n=4000, f=10, seed=3)
    d = xgb.DMatrix(X, label=y)

    def fit(seed):
        return xgb.train({"objective": "binary:logistic", "max_depth": 4,
                          "device": "cuda", "subsample": 0.5, "seed": seed,
                          "sampling_method": "gradient_based"}, d, 20,
                         verbose_eval=False)

    def generic(*a, **k):
        raise AssertionError("a tree came from boost_gpair")

    with monkeypatch.context() as mp:
        mp.setattr(xgb.core.Booster, "boost_gpair", generic)
        boosters = [fit(seed) for seed in range(5)]
        again = fit(0)
    assert "_fused_cache" in boosters[0].__dict__
    assert bytes(boosters[0].save_raw()) == bytes(again.save_raw())
    assert bytes(boosters[0].save_raw()) != bytes(boosters[1].save_raw())
    dev = [_logloss(b, d, y) for b in boosters]
    monkeypatch.setenv("XGB_AMD_MVS_HIP", "0")
    host_b = [fit(seed) for seed in range(5)]
    assert "_fused_cache" not in host_b[0].__dict__
    host = [_logloss(b, d, y) for b in host_b]
    print("logloss device", dev, "opt-out", host)
    assert abs(np.mean(dev) - np.mean(host)) <= max(host) - min(host)


def test_training_multiclass_generic_chain():
    X, y = make_classification(n=3000, f=10, seed=5, n_class=3)
    d = xgb.DMatrix(X, label=y)
    params = {"objective": "multi:softprob", "num_class": 3, "max_depth": 4,
              "device": "cuda", "subsample": 0.5,
              "sampling_method": "gradient_based"}
    losses = [_logloss(xgb.train(params, d, r, verbose_eval=False), d, y)
              for r in (1, 10)]
    assert losses[1] < losses[0] < math.log(3)
