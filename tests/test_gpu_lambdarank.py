"""LambdaMART HIP kernel (ops/cpp/lambdarank.hip) against the torch path
on CPU tensors; reference and tolerance in tests/rank_cases.py."""
import numpy as np
import pytest
import torch

from xgboost_amd.backend.gpu import LAMBDARANK_MAX_GROUP, lambdarank_schedule
from xgboost_amd.objectives import create_objective

from rank_cases import RankCases, _close

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

# binary labels leave group 3 without a hit
_cases = RankCases(LAYOUT, CONFIGS, no_hit=3, slab=False)
_info, _case, _kernel = _cases._info, _cases._case, _cases._kernel


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
