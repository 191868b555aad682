"""LambdaMART slab tier (ops/cpp/lambdarank_slab.hip, groups above 2048
documents) against the torch path on CPU tensors, which
tests/test_ranking.py pins to the per-pair oracle.

Tolerance: both sides accumulate in fp64 and cast once to fp32 (2^-24
relative each); fp64 reordering noise at these sizes is below 1e-9 of the
largest entry.  Anything larger is a wrong pair, not rounding."""
import functools

import numpy as np
import pytest
import torch

from xgboost_amd.backend.gpu import (LAMBDARANK_LDS_MAX_GROUP,
                                     LAMBDARANK_MAX_GROUP, LAMBDARANK_SLAB,
                                     LAMBDARANK_SLAB_ROWS,
                                     lambdarank_gpair_gpu,
                                     lambdarank_schedule)
from xgboost_amd.data import MetaInfo
from xgboost_amd.objectives import create_objective

SLAB = LAMBDARANK_SLAB[0]
# one past the LDS capacity, whole slabs and a few, empty, one wave twice:
# slab and LDS tiers in one call
LAYOUT = [LAMBDARANK_LDS_MAX_GROUP + 1,
          max(2 * SLAB, LAMBDARANK_LDS_MAX_GROUP) + 5, 0, 3, 64]
OBJECTIVES = ["rank:ndcg", "rank:map", "rank:pairwise"]
CONFIGS = {
    "default": {},
    "k5": {"lambdarank_num_pair_per_sample": 5},
    # head rows beyond the first slab of both long groups, many row chunks
    "k_over_slab": {"lambdarank_num_pair_per_sample": SLAB + 476},
    "no_score_norm": {"lambdarank_score_normalization": 0},
    "no_norm": {"lambdarank_normalization": 0},
    "group_weights": {},
}


def _info(layout, binary, weights=None):
    rng = np.random.RandomState(0)
    info = MetaInfo()
    info.num_row = int(sum(layout))
    info.group_ptr = np.concatenate([[0], np.cumsum(layout)]).astype(np.int64)
    y = rng.randint(0, 2 if binary else 5, info.num_row)
    if binary:
        y[:layout[0]] = 0  # a long group with no hit
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
    # one decimal: about 70 distinct scores, so ties cross every slab edge
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
    assert state is not None and state.slab is not None
    return lambdarank_gpair_gpu(scores, state, obj._hip_metric, obj._k(),
                                obj.score_norm, obj.normalize, obj.exp_gain)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("obj_name", OBJECTIVES)
def test_slab_matches_reference(obj_name, cfg):
    info, p, params, rg, rh = _case(obj_name, cfg)
    g, h = _kernel(obj_name, params, info, p)
    _close(g, rg.view(-1))
    _close(h, rh.view(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("obj_name", OBJECTIVES)
def test_round0_ties(obj_name):
    """All scores equal: the rank is the document order across slabs and
    the degenerate-group branch skips the score normalisation."""
    info, p, params, rg, rh = _case(obj_name, "default", ties=True)
    g, h = _kernel(obj_name, params, info, p)
    _close(g, rg.view(-1))
    _close(h, rh.view(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("obj_name", OBJECTIVES)
def test_reproducible(obj_name):
    info, p, params, _, _ = _case(obj_name, "k_over_slab")
    g1, h1 = _kernel(obj_name, params, info, p)
    g2, h2 = _kernel(obj_name, params, info, p)
    assert torch.equal(g1, g2) and torch.equal(h1, h2)


@pytest.mark.gpu
def test_dispatch_through_objective():
    info, p, _, rg, rh = _case("rank:ndcg", "default")
    obj = create_objective("rank:ndcg")
    assert obj._hip_state(p.cuda(), info) is not None
    g, h = obj.get_gradient(p.cuda(), info, 0)
    assert g.is_cuda and g.dtype == torch.float32
    _close(g, rg)
    _close(h, rh)


def test_schedule_slab_entry():
    """Groups 1, 3 and 4 are above the LDS tiers; items largest group
    first, offsets by group id."""
    gp = np.concatenate([[0], np.cumsum([3, 2049, 0, 5000, 2049])])
    s = lambdarank_schedule(gp, k=32, slab=1024)
    assert s["eligible"] and s["max_group"] == 5000
    assert {k: v.tolist() for k, v in s["lists"].items()} == {
        "wave": [0], "mid": [], "large": []}
    sl = s["slab"]
    assert sl["items"].tolist() == (
        [[3, 1024 * i] for i in range(5)] + [[1, 1024 * i] for i in range(3)]
        + [[4, 1024 * i] for i in range(3)])
    assert sl["item_off"].tolist() == [0, 0, 3, 3, 8, 11]
    assert sl["doc_off"].tolist() == [0, 0, 2049, 2049, 7049, 9098]
    assert sl["row_off"].tolist() == [0, 0, 96, 96, 256, 352]
    # k above a group: min(k, n) rows per item
    sl = lambdarank_schedule(gp, k=3000, slab=1024)["slab"]
    assert sl["row_off"].tolist() == [0, 0, 6147, 6147, 21147, 27294]
    # no long group: no items; too many row shares: not eligible
    assert lambdarank_schedule(gp[:2])["slab"]["items"].shape == (0, 2)
    full = np.arange(4) * LAMBDARANK_MAX_GROUP
    assert lambdarank_schedule(full, k=32)["eligible"]
    assert (3 * (LAMBDARANK_MAX_GROUP // SLAB) * LAMBDARANK_MAX_GROUP
            > LAMBDARANK_SLAB_ROWS)
    assert not lambdarank_schedule(full, k=10 ** 9)["eligible"]
