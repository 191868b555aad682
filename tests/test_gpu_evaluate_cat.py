"""Sorted-partition categorical split evaluation on the device
(ops/cpp/evaluate_cat.hip) against the numpy oracle
splits.evaluate_splits_np, exactly: gain bits, feature, direction,
quantised child sums and the go-right category set."""
import types

import numpy as np
import pytest
import torch

import eval_cases as ec
import xgboost_amd as xgb
from xgboost_amd.params import make_train_param
from xgboost_amd.splits import evaluate_splits_np

pytestmark = pytest.mark.gpu

_QUANT = types.SimpleNamespace(g_scale=ec.G_SCALE, h_scale=ec.H_SCALE)


def _cap():
    from xgboost_amd import ops
    return int(ops.load().gbt_evaluate_cat_max_width())


def _ops(widths, types_):
    """A GpuOps over cuts of the given widths; only its evaluator is used,
    so the bin matrix is one dummy row."""
    from xgboost_amd.backend.gpu import GpuOps
    from xgboost_amd.data import QuantizedMatrix
    from xgboost_amd.quantile import HistogramCuts
    ptrs = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    cuts = HistogramCuts(values=np.zeros(ptrs[-1], np.float32), ptrs=ptrs,
                         min_vals=np.zeros(len(widths), np.float32),
                         feature_types=list(types_))
    gidx = torch.zeros((1, len(widths)), dtype=torch.uint8, device="cuda")
    return GpuOps(QuantizedMatrix(gidx, cuts, False), col_copy=False), ptrs


def _hists(widths, k, seed):
    """int64 [k, n_bins, 2] category histograms and [k, 2] parents.  About
    a fifth of the categories of a node are absent; categories 0 and 1 of
    node 0's first feature are present with one (G, H); node 1 (k >= 3)
    has a single present category in its first feature; even nodes have
    missing rows (parent above every feature total), odd nodes none."""
    rng = np.random.RandomState(seed)
    ptrs = np.concatenate([[0], np.cumsum(widths)])
    nb = int(ptrs[-1])
    hist = np.zeros((k, nb, 2), np.int64)
    hist[:, :, 0] = rng.randint(-ec.BIN_MAX, ec.BIN_MAX, (k, nb))
    hist[:, :, 1] = rng.randint(1, ec.BIN_MAX, (k, nb))
    hist[rng.rand(k, nb) < 0.2] = 0
    hist[0, 0] = hist[0, 1] = (12345 << 20, 777 << 20)
    if k >= 3:
        hist[1, 1:widths[0]] = 0
        hist[1, 0] = (-(5 << 30), 9 << 30)
    tot = np.stack([hist[:, ptrs[f]:ptrs[f + 1]].sum(1)
                    for f in range(len(widths))], axis=1)   # [k, F, 2]
    parents = tot.max(1)
    parents[::2, 0] += rng.randint(-ec.BIN_MAX, ec.BIN_MAX, len(parents[::2]))
    parents[::2, 1] += rng.randint(1, ec.BIN_MAX, len(parents[::2]))
    for i in range(1, k, 2):  # top a present category up to the parent
        for f in range(len(widths)):
            b = ptrs[f] + int(np.argmax(hist[i, ptrs[f]:ptrs[f + 1], 1]))
            hist[i, b] += parents[i] - tot[i, f]
    return hist, parents


def _evaluate(widths, types_, hist, parents, params, feature_sets=None):
    """-> (GpuOps entries, oracle entries) of one evaluate call."""
    gops, ptrs = _ops(widths, types_)
    k = len(hist)
    p = make_train_param(dict({"max_depth": 6}, **params))
    cat = np.array([t == "c" for t in types_])
    psums = [tuple(int(v) for v in r) for r in parents]
    got = gops.evaluate_splits(torch.from_numpy(hist).cuda(), _QUANT, psums,
                               list(range(k)), p, feature_sets=feature_sets,
                               cat_mask=cat)
    want = evaluate_splits_np(hist, psums, ec.G_SCALE, ec.H_SCALE,
                              list(range(k)), ptrs, p,
                              feature_sets=feature_sets, cat_mask=cat)
    return got, want


def _assert_same(got, want):
    n_sorted = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.feature == w.feature, (i, g, w)
        if w.feature < 0:
            continue
        assert np.float64(g.gain).tobytes() == np.float64(w.gain).tobytes(), \
            (i, g.gain, w.gain)
        assert (g.default_left, g.is_cat, g.split_bin) == \
            (w.default_left, w.is_cat, w.split_bin), (i, g, w)
        assert (g.left_gq, g.left_hq, g.right_gq, g.right_hq) == \
            (w.left_gq, w.left_hq, w.right_gq, w.right_hq), (i, g, w)
        if w.is_cat:
            assert g.cat_bits.dtype == np.int32
            assert np.array_equal(g.cat_bits, w.cat_bits), (i, g, w)
            n_sorted += 1
    return n_sorted


def _no_host_route(monkeypatch):
    from xgboost_amd.backend.gpu import GpuOps

    def boom(*a, **kw):
        raise AssertionError("wide feature took the host route")
    monkeypatch.setattr(GpuOps, "_host_sorted_cat", boom)


# every feature is a wide categorical one, so each chosen split is a
# sorted-partition split and its gain is the oracle's expression bit for bit
@pytest.mark.parametrize("k", [1, 3, 130])
@pytest.mark.parametrize("width", [2, 5, 64, 65, 256, 257, "cap", "cap+1"])
def test_kernel_matches_oracle(width, k, monkeypatch):
    w = {"cap": _cap(), "cap+1": _cap() + 1}.get(width, width)
    if w <= _cap():
        _no_host_route(monkeypatch)  # cap + 1 mixes both routes in one call
    widths = [w, 37]
    hist, parents = _hists(widths, k, seed=w + k)
    got, want = _evaluate(widths, "cc", hist, parents,
                          {"max_cat_to_onehot": 1})
    n_sorted = _assert_same(got, want)
    assert n_sorted == k
    if width == "cap+1" and k >= 3:  # each route wins somewhere
        assert {e.feature for e in got} == {0, 1}


@pytest.mark.parametrize("params", [
    {"max_cat_threshold": 1}, {"max_cat_threshold": 3}, {"reg_alpha": 0.3},
    {"max_delta_step": 0.7}, {"min_child_weight": 9000.0},
    {"reg_lambda": 0.0}, ec.REGULARIZED], ids=str)
def test_kernel_training_parameters(params, monkeypatch):
    _no_host_route(monkeypatch)
    widths = [100, 37]
    hist, parents = _hists(widths, 3, seed=5)
    got, want = _evaluate(widths, "cc", hist, parents, params)
    assert _assert_same(got, want) >= 2
    if "max_cat_threshold" in params:
        for e in want:  # the left prefix is at most threshold + 1 long
            n_left = widths[e.feature] - len(e.cat_bits)
            assert n_left <= params["max_cat_threshold"] + 1


def test_duplicate_wide_column_lower_index_wins(monkeypatch):
    _no_host_route(monkeypatch)
    hist, parents = _hists([70], 3, seed=11)
    got, want = _evaluate([70, 70], "cc", np.concatenate([hist, hist], 1),
                          parents, {})
    # node 1 has one present category in either copy: no split at all
    assert _assert_same(got, want) == 2
    assert [e.feature for e in got] == [0, -1, 0]


def test_numeric_candidate_keeps_a_tie(monkeypatch):
    """A numeric column and a two-category column with the same bins.  All
    sums are small integers over power-of-two hessians and lambda is 0, so
    every product in either gain expression is exact and the two columns'
    best gains are equal: the numeric one stands."""
    _no_host_route(monkeypatch)
    one = np.array([[-3, 2], [5, 2]], np.int64) << 30   # (G, H) per bin
    hist = np.concatenate([one, one])[None]
    parents = one.sum(0)[None]
    gops, ptrs = _ops([2, 2], "qc")
    p = make_train_param({"max_depth": 6, "max_cat_to_onehot": 1,
                          "reg_lambda": 0.0})
    quant = types.SimpleNamespace(g_scale=float(1 << 30),
                                  h_scale=float(1 << 30))
    cat = np.array([False, True])
    psums = [tuple(int(v) for v in parents[0])]
    got = gops.evaluate_splits(torch.from_numpy(hist).cuda(), quant, psums,
                               [0], p, cat_mask=cat)
    want = evaluate_splits_np(hist, psums, quant.g_scale, quant.h_scale, [0],
                              ptrs, p, cat_mask=cat)
    _assert_same(got, want)
    assert got[0].feature == 0 and not got[0].is_cat and got[0].gain > 0
    # the wide column alone reaches the same gain
    alone = gops.evaluate_splits(torch.from_numpy(hist).cuda(), quant, psums,
                                 [0], p, cat_mask=cat, feature_sets=[[1]])
    assert alone[0].feature == 1 and alone[0].gain == got[0].gain


def test_per_node_feature_sets(monkeypatch):
    _no_host_route(monkeypatch)
    widths = [70, 37]
    hist, parents = _hists(widths, 5, seed=13)
    sets = [None, np.array([1]), np.array([0]), np.array([0, 1]),
            np.array([1])]
    got, want = _evaluate(widths, "cc", hist, parents, {}, feature_sets=sets)
    assert _assert_same(got, want) == 5
    assert [e.feature for e in got][1:3] == [1, 0] and got[4].feature == 1


# ---------------------------------------------------------------------------
# public path


def _public_data():
    rng = np.random.RandomState(3)
    n = 4000
    c5, c70, c300 = (rng.randint(0, c, n) for c in (5, 70, 300))
    xn = rng.randn(n, 2).astype(np.float32)
    y = (np.isin(c70 % 7, [1, 4]) * 2.0 + (c300 % 3 == 0) * 1.5
         + (c5 == 2) + 0.5 * xn[:, 0] + 0.3 * rng.randn(n)).astype(np.float32)
    xn[rng.rand(n, 2) < 0.1] = np.nan
    X = np.column_stack([c5, c70, c300, xn]).astype(np.float32)
    return X, y, ["c", "c", "c", "q", "q"]


_trained = {}


def _train(device, key=None):
    if key in _trained:
        return _trained[key]
    X, y, ft = _public_data()
    d = xgb.DMatrix(X, label=y, feature_types=ft)
    params = {"objective": "reg:squarederror", "max_depth": 5, "max_bin": 64,
              "max_cat_to_onehot": 4, "seed": 0, "device": device}
    bst = xgb.train(params, d, 4, verbose_eval=False)
    out = bst, bst.predict(d)
    if key is not None:
        _trained[key] = out
    return out


@pytest.mark.parametrize("cat_hip", ["1", "0"])
def test_train_matches_cpu(cat_hip, monkeypatch):
    monkeypatch.setenv("XGB_AMD_CAT_HIP", cat_hip)
    if cat_hip == "1":
        _no_host_route(monkeypatch)
    bc, pc = _train("cpu", key="cpu")  # the reference, trained once
    bg, pg = _train("cuda")
    n_sorted = 0
    for tg, tc in zip(bg.trees, bc.trees):
        n = tc.n_nodes
        assert tg.n_nodes == n
        for name in ("left", "right", "split_index", "split_type",
                     "default_left"):
            assert np.array_equal(getattr(tg, name)[:n],
                                  getattr(tc, name)[:n]), name
        assert tg.cat_segments.keys() == tc.cat_segments.keys()
        for nid, cats in tc.cat_segments.items():
            assert np.array_equal(tg.cat_segments[nid], cats), nid
            n_sorted += int(tc.split_index[nid] in (1, 2))
    assert n_sorted > 0, "no sorted-partition split on the wide columns"
    # equal trees; the two predictors add four fp32 leaf values of
    # magnitude <= 4 in different orders: a few ulps of 2^-22
    np.testing.assert_allclose(pg, pc, atol=4e-6)
