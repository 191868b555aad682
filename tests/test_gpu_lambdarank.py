"""LambdaMART HIP kernel (ops/cpp/lambdarank.hip) against the torch path
on CPU tensors, which tests/test_ranking.py pins to the per-pair oracle.

Tolerance: both sides accumulate in fp64 and cast once to fp32 (2^-24
relative each); fp64 reordering noise at these sizes is below 1e-9 of the
largest entry.  Anything larger is a wrong pair, not rounding."""
import functools

import numpy as np
import pytest
import torch

from xgboost_amd.backend.gpu import (LAMBDARANK_MAX_GROUP,
                                     lambdarank_gpair_gpu,
                                     lambdarank_schedule)
from xgboost_amd.data import MetaInfo
from xgboost_amd.objectives import create_objective

# empty group, singleton, both sides of k = 32, of the wave (64) and of the
# mid tier (256), and one group several block strides long
LAYOUT = [1, 2, 5, 33, 64, 65, 257, 600, 0, 3]
OBJECTIVES = ["rank:ndcg", "rank:map", "rank:pairwise"]
CONFIGS = {
    "default": {},
    "k5": {"lambdarank_num_pair_per_sample": 5},
    "k1000": {"lambdarank_num_pair_per_sample": 1000},
    "no_score_norm": {"lambdarank_score_normalization": 0},
    "no_norm": {"lambdarank_normalization": 0},
    "linear_gain": {"ndcg_exp_gain": 0},
    "group_weights": {},
}
CASES = [(o, c) for o in OBJECTIVES for c in CONFIGS
         if c != "linear_gain" or o == "rank:ndcg"]


def _info(layout, binary, weights=None, seed=0):
    rng = np.random.RandomState(seed)
    info = MetaInfo()
    info.num_row = int(sum(layout))
    info.group_ptr = np.concatenate([[0], np.cumsum(layout)]).astype(np.int64)
    y = rng.randint(0, 2 if binary else 5, info.num_row)
    if binary and len(layout) > 3:
        y[info.group_ptr[3]:info.group_ptr[4]] = 0  # a group with no hit
    info.labels = y.astype(np.float32)
    if weights is not None:
        info.weights = np.asarray(weights, np.float32)
    return info


@functools.lru_cache(maxsize=None)
def _case(obj_name, cfg, ties=False):
    """(info, scores, objective params, CPU reference g and h)."""
    w = (np.random.RandomState(5).uniform(0.5, 2.0, len(LAYOUT))
         if cfg == "group_weights" else None)
    info = _info(LAYOUT, obj_name == "rank:map", w)
    p = np.random.RandomState(1).randn(info.num_row).round(1)
    p = np.full_like(p, 0.5) if ties else p
    p = torch.tensor(p, dtype=torch.float32).view(-1, 1)
    g, h = create_objective(obj_name, CONFIGS[cfg]).get_gradient(p, info, 0)
    return info, p, CONFIGS[cfg], g, h


def _close(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape
    bound = 2.0 ** -22 * ref.abs() + 1e-9 * ref.abs().max()
    err = (got - ref).abs()
    assert bool((err <= bound).all()), (
        f"max err {float(err.max()):.3e} at {int(err.argmax())}, "
        f"bound there {float(bound.view(-1)[err.argmax()]):.3e}")


def _kernel(obj_name, params, info, p):
    obj = create_objective(obj_name, params)
    scores = p.cuda().view(-1)
    state = obj._hip_state(scores, info)
    assert state is not None
    return lambdarank_gpair_gpu(scores, state, obj._hip_metric, obj._k(),
                                obj.score_norm, obj.normalize, obj.exp_gain)


@pytest.mark.gpu
@pytest.mark.parametrize("obj_name,cfg", CASES)
def test_kernel_matches_reference(obj_name, cfg):
    info, p, params, rg, rh = _case(obj_name, cfg)
    g, h = _kernel(obj_name, params, info, p)
    _close(g, rg.view(-1))
    _close(h, rh.view(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("obj_name", OBJECTIVES)
def test_round0_ties(obj_name):
    """All scores equal: rank order is document order and the degenerate
    group branch skips the score normalisation."""
    info, p, params, rg, rh = _case(obj_name, "default", ties=True)
    g, h = _kernel(obj_name, params, info, p)
    _close(g, rg.view(-1))
    _close(h, rh.view(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("obj_name", OBJECTIVES)
def test_reproducible(obj_name):
    info, p, params, _, _ = _case(obj_name, "default")
    g1, h1 = _kernel(obj_name, params, info, p)
    g2, h2 = _kernel(obj_name, params, info, p)
    assert torch.equal(g1, g2) and torch.equal(h1, h2)


@pytest.mark.gpu
@pytest.mark.parametrize("params,layout,rounds,on_kernel", [
    ({}, LAYOUT, 1, True),
    ({"lambdarank_unbiased": 1}, LAYOUT, 2, False),
    ({"lambdarank_pair_method": "mean"}, LAYOUT, 1, False),
    ({}, [LAMBDARANK_MAX_GROUP + 1], 1, False),
], ids=["eligible", "unbiased", "mean", "oversized"])
def test_dispatch_through_objective(params, layout, rounds, on_kernel):
    info = _info(layout, False)
    p = torch.tensor(np.random.RandomState(2).randn(info.num_row).round(1),
                     dtype=torch.float32).view(-1, 1)
    cpu = create_objective("rank:ndcg", params)
    dev = create_objective("rank:ndcg", params)
    assert (dev._hip_state(p.cuda(), info) is not None) == on_kernel
    for it in range(rounds):
        rg, rh = cpu.get_gradient(p, info, it)
        g, h = dev.get_gradient(p.cuda(), info, it)
        assert g.is_cuda and g.dtype == torch.float32
        _close(g, rg)
        _close(h, rh)


def test_schedule():
    s = lambdarank_schedule(np.concatenate([[0], np.cumsum(LAYOUT)]))
    assert s["eligible"] and s["max_group"] == 600
    assert {k: v.tolist() for k, v in s["lists"].items()} == {
        "wave": [4, 3, 2, 9, 1, 0], "mid": [5], "large": [7, 6]}
    assert not lambdarank_schedule(
        np.array([0, 3, 3 + LAMBDARANK_MAX_GROUP + 1]))["eligible"]
