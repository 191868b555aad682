"""Single-pass split evaluation against the single-wave reference kernel
(bit for bit, every (node, feature) slot) and against the numpy oracle
(the selected split per node), on synthetic int64 histograms."""
import numpy as np
import pytest
import torch

from xgboost_amd.params import make_train_param
from xgboost_amd.splits import evaluate_splits_np

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------
# evaluate: gbt_evaluate_masked vs gbt_evaluate_ref vs numpy

# one wave's chunk is 64 bins and the block covers 256: widths on both
# sides of each, a one- and a two-bin feature, and one far wider than the
# block (the max_bin 1024 case)
_WIDTHS = np.array([1, 2, 63, 64, 65, 128, 255, 256, 257, 1000])
_PTRS = np.concatenate([[0], np.cumsum(_WIDTHS)]).astype(np.int32)
_F = len(_WIDTHS)
_NB = int(_PTRS[-1])
_QS = float(1 << 30)
# a bin holds up to a few thousand rows of gradients quantized to 2^30
_BIN_MAX = 3000 * (1 << 30)
_G_SCALE = _QS / 3.7
_H_SCALE = _QS / 0.9
_SENTINEL = -77

_hist_cache = {}


def _hists(k):
    """-> (hist [k, n_bins, 2], parents [k, 2]) int64, built once per k.

    Every feature of a node sums to the node's parent minus a missing
    remainder, as real histograms do.  Even nodes have a remainder (h >=
    0, g of either sign) that differs per feature; odd nodes have none,
    so both missing directions tie at every bin.  Runs of empty bins give
    consecutive equal gains.  Node 0 has one all-empty feature; the last
    node (k >= 3) has h = 0 everywhere."""
    if k in _hist_cache:
        return _hist_cache[k]
    rng = np.random.RandomState(100 + k)
    hist = np.zeros((k, _NB, 2), np.int64)
    hist[:, :, 0] = rng.randint(-_BIN_MAX, _BIN_MAX, (k, _NB))
    hist[:, :, 1] = rng.randint(0, _BIN_MAX, (k, _NB))
    for i in range(k):
        for f in range(_F):
            b0, b1 = int(_PTRS[f]), int(_PTRS[f + 1])
            for _ in range(3):  # runs of empty bins
                if b1 - b0 >= 8:
                    s = rng.randint(b0, b1 - 4)
                    hist[i, s:s + rng.randint(2, 40), :][: b1 - s] = 0
    hist[0, _PTRS[6]:_PTRS[7], :] = 0  # an all-empty feature
    parents = np.zeros((k, 2), np.int64)
    for i in range(k):
        tot = np.stack([hist[i, _PTRS[f]:_PTRS[f + 1]].sum(0)
                        for f in range(_F)])          # [F, 2]
        parents[i, 0] = tot[:, 0].max() + rng.randint(-_BIN_MAX, _BIN_MAX)
        parents[i, 1] = tot[:, 1].max() + rng.randint(0, _BIN_MAX)
        if i % 2 == 1:
            # no missing remainder: top one bin of every feature up to the
            # parent (h stays >= 0: the parent is above every total)
            for f in range(_F):
                b = rng.randint(_PTRS[f], _PTRS[f + 1])
                hist[i, b] += parents[i] - tot[f]
    if k >= 3:
        hist[k - 1, :, 1] = 0
        parents[k - 1, 1] = 0
    _hist_cache[k] = (hist, parents)
    return _hist_cache[k]


def _launch(fn, hist, parents, k_launch, p, *, maxabs=None, scales=None,
            monotone=None, bounds=None, mask=None, mask_stride=0, cat=None,
            k_dev=None):
    """One evaluate launch with sentinel-filled outputs -> numpy
    (gain bits, bin, dir, lsum)."""
    from xgboost_amd import ops
    dev = torch.device("cuda")

    def up(a, dt):
        return (None if a is None
                else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev))

    t_hist, t_par = up(hist, np.int64), up(parents, np.int64)
    t_ptrs = up(_PTRS, np.int32)
    t_maxabs, t_mono = up(maxabs, np.float32), up(monotone, np.int8)
    t_bounds, t_mask = up(bounds, np.float64), up(mask, np.uint8)
    t_cat = up(cat, np.uint8)
    t_kdev = up(None if k_dev is None else np.array([k_dev]), np.int32)
    n = hist.shape[0]
    gain = torch.full((n, _F), _SENTINEL, dtype=torch.int64, device=dev)
    bins = torch.full((n, _F), _SENTINEL, dtype=torch.int32, device=dev)
    dirs = torch.full((n, _F), 200, dtype=torch.uint8, device=dev)
    lsum = torch.full((n, _F, 2), _SENTINEL, dtype=torch.int64, device=dev)
    gs, hs = scales if scales is not None else (_G_SCALE, _H_SCALE)
    fn(ops.ptr(t_hist), k_launch, _NB, _F, ops.ptr(t_ptrs), ops.ptr(t_par),
       ops.ptr(t_maxabs), gs, hs, p.reg_lambda, p.reg_alpha,
       p.max_delta_step, p.min_child_weight, ops.ptr(t_mono),
       ops.ptr(t_bounds), mask_stride, ops.ptr(t_mask), ops.ptr(t_cat),
       ops.ptr(gain), ops.ptr(bins), ops.ptr(dirs), ops.ptr(lsum),
       ops.ptr(t_kdev), 0, ops.stream())
    best = torch.full((n, 6), _SENTINEL, dtype=torch.int64, device=dev)
    ops.load().gbt_select_best(ops.ptr(gain), ops.ptr(bins), ops.ptr(dirs),
                               ops.ptr(lsum), k_launch, _F, ops.ptr(best),
                               ops.ptr(t_kdev), ops.stream())
    torch.cuda.synchronize()
    return (gain.cpu().numpy(), bins.cpu().numpy(), dirs.cpu().numpy(),
            lsum.cpu().numpy(), best.cpu().numpy())


def _check(k, params=None, oracle=True, **kw):
    """New kernel == reference kernel in every output slot; its selected
    split per node == the numpy oracle's.  Returns the new kernel's
    outputs."""
    from xgboost_amd import ops
    lib = ops.load()
    hist, parents = _hists(k)
    p = make_train_param(dict({"max_depth": 6}, **(params or {})))
    new = _launch(lib.gbt_evaluate_masked, hist, parents, k, p, **kw)
    ref = _launch(lib.gbt_evaluate_ref, hist, parents, k, p, **kw)
    for name, a, b in zip(("gain bits", "bin", "dir", "lsum", "best"),
                          new, ref):
        assert np.array_equal(a, b), name
    if not oracle:
        return new
    mask = kw.get("mask")
    fsets = None
    if mask is not None:
        rows = mask if kw.get("mask_stride") else np.repeat(mask, k, axis=0)
        fsets = [np.nonzero(r)[0] for r in rows.reshape(k, _F)]
    cat = kw.get("cat")
    want = evaluate_splits_np(
        hist, [tuple(int(v) for v in r) for r in parents], _G_SCALE,
        _H_SCALE, list(range(k)), _PTRS, p, feature_sets=fsets,
        monotone=kw.get("monotone"),
        cat_mask=None if cat is None else cat.astype(bool),
        node_bounds=kw.get("bounds"))
    best = new[4]
    n_valid = 0
    for i, e in enumerate(want):
        if e.feature < 0:
            assert best[i, 1] == -1 and best[i, 5] == -1, i
            continue
        n_valid += 1
        assert int(best[i, 5]) == e.feature, (i, best[i], e)
        assert int(best[i, 1]) == e.split_bin, (i, best[i], e)
        assert bool(best[i, 2]) == e.default_left, (i, best[i], e)
        assert int(best[i, 3]) == e.left_gq and int(best[i, 4]) == e.left_hq
        assert best[i, 0:1].view(np.float64)[0] == pytest.approx(
            e.gain, rel=1e-12)
    assert n_valid >= (k + 1) // 2
    return new


@pytest.mark.parametrize("k", [1, 3, 130])
def test_evaluate_matches_ref_and_oracle(k):
    gain, bins, dirs, lsum, _ = _check(k)
    hist, parents = _hists(k)
    g = gain.view(np.float64)
    # the all-empty feature of node 0: with a missing remainder the only
    # candidates put everything on one side
    assert bins[0, 6] == -1 and g[0, 6] == -np.inf
    if k >= 3:
        assert np.all(bins[k - 1] == -1)  # h = 0: nothing is valid
        # no missing remainder (odd nodes): both directions tie, dir 0 wins
        # (the one-bin feature holds the whole parent: no valid split)
        assert np.all(bins[1, 1:] >= 0) and np.all(dirs[1] == 0)
    # an empty bin ties with the bin before it, and the lower bin wins:
    # the chosen bin is never empty unless it is the feature's first
    for i in range(k):
        for f in range(_F):
            b = bins[i, f]
            if b > _PTRS[f]:
                assert hist[i, b].any(), (i, f, b)


def test_evaluate_monotone_with_bounds():
    k = 5
    rng = np.random.RandomState(1)
    mono = np.array([1, -1, 1, -1, 0, 1, -1, 0, 1, -1], np.int8)
    lo = -np.abs(rng.randn(k)) * 2.0
    bounds = np.stack([lo, lo + np.abs(rng.randn(k)) * 3.0], axis=1)
    _check(k, monotone=mono, bounds=bounds)


def test_evaluate_per_node_mask():
    k = 5
    rng = np.random.RandomState(2)
    mask = (rng.rand(k, _F) < 0.5).astype(np.uint8)
    mask[:, 3] = 1
    gain, bins, *_ = _check(k, mask=mask, mask_stride=_F)
    assert np.all(bins[mask == 0] == -1)
    assert np.all(gain.view(np.float64)[mask == 0] == -np.inf)


def test_evaluate_broadcast_mask_row():
    mask = np.array([[1, 0, 1, 1, 0, 1, 0, 1, 1, 0]], np.uint8)
    gain, bins, *_ = _check(5, mask=mask, mask_stride=0)
    assert np.all(bins[:, mask[0] == 0] == -1)


def test_evaluate_categorical_feature():
    cat = np.zeros(_F, np.uint8)
    cat[4] = 1  # 65 categories, one-vs-rest
    # min_child_weight stays at its default of 1, so the oracle's one-hot
    # branch rejects the same empty-side candidates as the kernels do
    _check(5, params={"max_cat_to_onehot": 128}, cat=cat)


def test_evaluate_regularized():
    _check(5, params={"reg_alpha": 0.3, "max_delta_step": 0.7,
                      "min_child_weight": 2.5, "reg_lambda": 1.5})


def test_evaluate_device_scales_match_host_scales():
    from xgboost_amd import ops
    lib = ops.load()
    k = 5
    hist, parents = _hists(k)
    p = make_train_param({"max_depth": 6})
    maxabs = np.array([3.7, 0.9], np.float32)
    scales = tuple(_QS / float(m) for m in maxabs)
    dev_new = _launch(lib.gbt_evaluate_masked, hist, parents, k, p,
                      maxabs=maxabs, scales=(0.0, 0.0))
    dev_ref = _launch(lib.gbt_evaluate_ref, hist, parents, k, p,
                      maxabs=maxabs, scales=(0.0, 0.0))
    host_new = _launch(lib.gbt_evaluate_masked, hist, parents, k, p,
                       scales=scales)
    for a, b, c in zip(dev_new, dev_ref, host_new):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.any(dev_new[1] >= 0)


def test_evaluate_k_dev_leaves_later_slots_untouched():
    k, live = 130, 77
    new = _check(k, oracle=False, k_dev=live)
    full = _check(k, oracle=False)
    gain, bins, dirs, lsum, best = new
    assert np.all(gain[live:] == _SENTINEL) and np.all(bins[live:] == _SENTINEL)
    assert np.all(dirs[live:] == 200) and np.all(lsum[live:] == _SENTINEL)
    assert np.all(best[live:] == _SENTINEL)
    for a, b in zip(new, full):
        assert np.array_equal(a[:live], b[:live])

