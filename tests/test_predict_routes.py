"""Host prediction routes of the Booster: margins, the DART drop-set
helper and leaf ids for dense, sparse CSR and external-memory matrices,
against oracles written out here (host leaf ids, then explicit per-tree
fp32 adds in tree order).  Everything is compared with exact equality."""
import numpy as np
import pytest
import scipy.sparse as sp

import xgboost_amd as xgb
from xgboost_amd.extmem import DataIter, ExtMemQuantileDMatrix

N, F = 300, 5
MAX_BIN = 32


class _Iter(DataIter):
    def __init__(self, Xs):
        super().__init__()
        self.Xs, self.i = Xs, 0

    def reset(self):
        self.i = 0

    def next(self, input_data) -> bool:
        if self.i >= len(self.Xs):
            return False
        input_data(data=self.Xs[self.i])
        self.i += 1
        return True


def _rows():
    rng = np.random.RandomState(7)
    X = rng.randn(N, F).astype(np.float32)
    X[rng.rand(N, F) < 0.3] = np.nan
    W = rng.randn(F, 3)
    Y = (np.nan_to_num(X) @ W + 0.1 * rng.randn(N, 3)).astype(np.float32)
    return X, Y


def _train(kind, X, Y):
    params = {"max_depth": 3, "eta": 0.3, "max_bin": MAX_BIN,
              "objective": "reg:squarederror"}
    label = Y[:, 0]
    if kind == "vector":
        params["multi_strategy"] = "multi_output_tree"
        label = Y
    elif kind == "dart":
        params.update(booster="dart", rate_drop=0.5, seed=3)
    bst = xgb.train(params, xgb.DMatrix(X, label=label), 6,
                    verbose_eval=False)
    if kind == "vector":
        assert all(t.leaf_values is not None for t in bst.trees)
    if kind == "dart":
        assert any(w != 1.0 for w in bst.weight_drop)
    return bst


@pytest.fixture(scope="module")
def case():
    """Rows, the three forests and, per forest, the host leaf ids of every
    tree on the raw rows.  Shared by all tests and never modified."""
    X, Y = _rows()
    forests = {}
    for kind in ("scalar", "vector", "dart"):
        bst = _train(kind, X, Y)
        leaf = np.stack([t.predict_leaf_np(X) for t in bst.trees], axis=1)
        forests[kind] = (bst, leaf)
    return X, Y, forests


def _matrix(kind, X, Y):
    if kind == "dense":
        return xgb.DMatrix(X)
    if kind == "csr":  # missing entries are absent, not stored
        mask = ~np.isnan(X)
        csr = sp.coo_matrix((X[mask], np.nonzero(mask)), shape=X.shape)
        csr = csr.tocsr()
        assert csr.nnz == int(mask.sum()) < X.size
        return xgb.DMatrix(csr)
    # two pages, one of them empty; the cuts of the training matrix, so
    # that every split condition is a cut value and the bin walk is exact
    ref = xgb.DMatrix(X, label=Y[:, 0])
    ref.quantized(MAX_BIN)
    d = ExtMemQuantileDMatrix(_Iter([X[:0], X]), max_bin=MAX_BIN, ref=ref)
    assert d.page_offsets == [0, 0, N]
    return d


def _oracle(bst, leaf, trees, start):
    """out[:, g] += float32(leaf) * float32(w), tree by tree."""
    out = np.full((leaf.shape[0], bst.n_outputs), start, np.float32)
    for t in trees:
        tree = bst.trees[t]
        w = np.float32(bst._tw(t))
        if tree.leaf_values is not None:
            out += (tree.leaf_values[:tree.n_nodes][leaf[:, t]]
                    .astype(np.float32) * w)
        else:
            out[:, bst.tree_info[t]] += (
                tree.split_cond[:tree.n_nodes][leaf[:, t]]
                .astype(np.float32) * w)
    return out


MATRICES = ["dense", "csr", "extmem"]
FORESTS = ["scalar", "vector", "dart"]


@pytest.mark.parametrize("forest", FORESTS)
@pytest.mark.parametrize("matrix", MATRICES)
def test_host_margins_match_per_tree_adds(case, matrix, forest):
    X, Y, forests = case
    bst, leaf = forests[forest]
    d = _matrix(matrix, X, Y)
    n_trees = len(bst.trees)
    got = bst._predict_margin(d).cpu().numpy()
    want = _oracle(bst, leaf, range(n_trees), bst._base_margin_value())
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want)
    lo, hi = bst._tree_range((1, 3))
    got = bst._predict_margin(d, (1, 3)).cpu().numpy()
    assert np.array_equal(
        got, _oracle(bst, leaf, range(lo, hi), bst._base_margin_value()))
    idxs = [0, 2, 3, n_trees - 1]
    got = bst._predict_tree_subset(d, idxs).cpu().numpy()
    assert np.array_equal(got, _oracle(bst, leaf, idxs, 0.0))
    got = bst._predict_tree_subset(d, []).cpu().numpy()
    assert np.array_equal(got, np.zeros((N, bst.n_outputs), np.float32))


def test_empty_tree_set_reads_no_page(case, monkeypatch):
    """The margin of a booster that has no tree yet (the first round of
    training) expands no external-memory page."""
    from xgboost_amd.data import QuantizedMatrix

    def boom(*a, **k):
        raise AssertionError("page expanded for an empty tree set")

    X, Y, forests = case
    bst, _ = forests["scalar"]
    d = _matrix("extmem", X, Y)
    monkeypatch.setattr(QuantizedMatrix, "global_gidx", boom)
    got = bst._predict_tree_subset(d, []).cpu().numpy()
    assert np.array_equal(got, np.zeros((N, 1), np.float32))
    assert bst._predict_leaf(d, 2, 2).shape == (N, 0)


@pytest.mark.parametrize("forest", FORESTS)
@pytest.mark.parametrize("matrix", MATRICES)
def test_host_leaf_ids_match_per_tree_walk(case, matrix, forest):
    X, Y, forests = case
    bst, leaf = forests[forest]
    d = _matrix(matrix, X, Y)
    n_trees = len(bst.trees)
    got = bst._predict_leaf(d, 0, n_trees)
    assert got.shape == (N, n_trees)
    assert np.array_equal(got, leaf)
    assert np.array_equal(bst._predict_leaf(d, 2, 5), leaf[:, 2:5])
