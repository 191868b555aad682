"""LambdaMART slab tier (ops/cpp/lambdarank_slab.hip, groups above 2048
documents) against the torch path on CPU tensors; reference and tolerance
in tests/rank_cases.py."""
import numpy as np
import pytest
import torch

from xgboost_amd.backend.gpu import (LAMBDARANK_LDS_MAX_GROUP,
                                     LAMBDARANK_MAX_GROUP, LAMBDARANK_SLAB,
                                     LAMBDARANK_SLAB_ROWS, LambdaRankState,
                                     lambdarank_gpair_gpu,
                                     lambdarank_schedule)
from xgboost_amd.objectives import create_objective

from rank_cases import RankCases, _close

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

# binary labels leave the first long group without a hit; every kernel
# call must have slab work
_cases = RankCases(LAYOUT, CONFIGS, no_hit=0, slab=True)
_info, _case, _kernel = _cases._info, _cases._case, _cases._kernel


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


@pytest.mark.gpu
@pytest.mark.parametrize("k", [32, 300])
@pytest.mark.parametrize("obj_name", OBJECTIVES)
def test_slab_agrees_with_lds_tier(obj_name, k):
    """One group of 600 documents through the LDS "large" tier and, with a
    slab entry written by hand (three items of 256; k = 300 puts head rows
    in the second), through the slab kernels, which take any group of at
    least one document.  The tiers add the row shares in different orders,
    so the bound is the file's, not equality."""
    n, kk = 600, min(k, 600)
    info = _info([n], obj_name == "rank:map", no_hit=False)
    obj = create_objective(obj_name, {"lambdarank_num_pair_per_sample": k})
    scores = torch.tensor(np.random.RandomState(1).randn(n).round(1),
                          dtype=torch.float32).cuda()
    lds = obj._hip_state(scores, info)
    assert list(lds.work) == ["large"] and lds.slab is None
    args = (obj._hip_metric, k, obj.score_norm, obj.normalize, obj.exp_gain)
    rg, rh = lambdarank_gpair_gpu(scores, lds, *args)

    inv_idcg = None if lds.inv_idcg is None else lds.inv_idcg.cpu().numpy()
    st = LambdaRankState(info.labels, info.group_ptr, None, scores.device,
                         inv_idcg, k)
    st.work = {}
    st.slab = {
        "items": torch.tensor([[0, 0], [0, SLAB], [0, 2 * SLAB]],
                              dtype=torch.int32).cuda(),
        "item_off": torch.tensor([0, 3], dtype=torch.int32).cuda(),
        "doc_off": torch.tensor([0, n], dtype=torch.int64).cuda(),
        "row_off": torch.tensor([0, 3 * kk], dtype=torch.int64).cuda()}
    st.slab_docs, st.slab_rows = n, 3 * kk
    g, h = lambdarank_gpair_gpu(scores, st, *args)
    _close(g, rg.cpu())
    _close(h, rh.cpu())


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
