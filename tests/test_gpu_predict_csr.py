"""Sparse CSR GPU predictor (predict_csr.hip): margins, leaf ids, eval
sets and DART drop sets.  The oracle is always a CPU booster reloaded
from the same model JSON, predicting the same rows as a dense matrix
with NaN for every absent entry; margins and leaf ids are compared with
exact equality (the kernel adds leaves in tree order with plain fp32
adds, like the host loops), DART weights excepted."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import xgboost_amd as xgb
from xgboost_amd.tree_model import RegTree

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _reload(bst, device):
    out = xgb.Booster({"device": device})
    out.load_model(bytes(bst.save_raw("json")))
    return out


def _boom(*a, **k):
    raise AssertionError("host tree walk used on the device path")


@contextlib.contextmanager
def _device_only(monkeypatch):
    """Every host traversal raises while the block runs."""
    with monkeypatch.context() as m:
        m.setattr(RegTree, "predict_leaf_np", _boom)
        m.setattr(RegTree, "predict_leaf_bins", _boom)
        yield


def _dense_nan(csr, width=None):
    """Absent entries become NaN; stored entries (zeros too) stay."""
    coo = csr.tocoo()
    X = np.full((csr.shape[0], width or csr.shape[1]), np.nan, np.float32)
    X[coo.row, coo.col] = coo.data
    return X


def _sparse_rows(seed, n, f, density=0.4):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, f).astype(np.float32)
    X[rng.rand(n, f) >= density] = 0.0
    return rng, X, sp.csr_matrix(X)


# -- 1. kernel against host leaf ids on a hand-built forest ---------------

class _Forest:
    """The part of a Booster that _ForestQ reads."""

    def __init__(self, trees):
        self.trees = trees
        self.tree_info = [0] * len(trees)
        self.n_outputs = 1

    def _tw(self, t):
        return 1.0


_CATS = [1, 5, 33, 40]  # crosses the first 32-bit word
_LONE = 4               # a column only the full row holds
_HOT = [0, 1, 2, 3, 5]  # half-full columns at either width


def _split(tree, nid, f, cond, default_left, cats=None):
    return tree.add_split(nid, f, cond, default_left, 1.0, 0.0,
                          0.125 * (nid + 1), -0.25 * (nid + 1), 1.0, 0.5,
                          0.5, categories_go_right=cats)


def _hand_forest(F, rng):
    a = RegTree(F)  # both default directions, one categorical node
    l, r = _split(a, 0, 0, 0.0, True)
    _split(a, l, F - 1, 0.25, False)
    l2, _ = _split(a, r, 1, 0.0, True, cats=np.asarray(_CATS))
    _split(a, l2, 2, -0.5, False)
    b = RegTree(F)  # a column that (almost) no row holds
    l, r = _split(b, 0, _LONE, 0.0, False)
    _split(b, l, 3, 0.1, True)
    _split(b, r, 3, -0.1, False)
    c = RegTree(F)  # a feature past the matrix' width
    l, r = _split(c, 0, F + 5, 0.0, True)
    _split(c, l, 0, 0.5, False)
    l, r = _split(c, r, F + 1, 0.0, False)
    _split(c, r, 2, 0.0, True)
    stump = RegTree(F)
    stump.set_leaf(0, 0.25)
    trees = [a, b, c, stump]
    for _ in range(4):  # deeper random trees over every column
        t = RegTree(F)
        frontier = [0]
        for _ in range(5):
            nxt = []
            for nid in frontier:
                if nid != 0 and rng.rand() < 0.2:
                    continue
                f = int(rng.choice(_HOT) if rng.rand() < 0.8
                        else rng.randint(F))
                if f == 1:
                    nxt += _split(t, nid, 1, 0.0, bool(rng.rand() < 0.5),
                                  cats=rng.choice(46, 9, replace=False))
                else:
                    nxt += _split(t, nid, f, float(rng.randn() * 0.5),
                                  bool(rng.rand() < 0.5))
            frontier = nxt
        trees.append(t)
    return _Forest(trees)


def _hand_rows(F, rng, n=1000):
    X = rng.randn(n, F).astype(np.float32)
    X[:, 1] = rng.randint(0, 46, n)  # categories
    keep = rng.rand(n, F) < 0.05
    keep[:, _HOT] = rng.rand(n, len(_HOT)) < 0.5
    keep[:, _LONE] = False
    keep[0] = keep[n - 1] = False    # empty first and last rows
    keep[1] = True                   # one row with every column
    X[rng.rand(n, F) < 0.05] = 0.0   # explicit zeros
    X[2, 0] = X[3, 3] = X[1, 2] = np.nan  # stored NaNs
    keep[2, 0] = keep[3, 3] = True
    rows, cols = np.nonzero(keep)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    csr = sp.csr_matrix((X[rows, cols], cols.astype(np.int32), indptr),
                        shape=(n, F))
    assert csr.nnz == keep.sum() and csr.has_sorted_indices
    assert indptr[1] == 0 and indptr[n] == indptr[n - 1]
    assert indptr[2] - indptr[1] == F
    return csr


def _host_margin(forest, leaf):
    """Sequential fp32 adds in tree order, from host leaf ids."""
    out = np.zeros((leaf.shape[0], 1), np.float32)
    for t, tree in enumerate(forest.trees):
        out[:, 0] += tree.split_cond[:tree.n_nodes][leaf[:, t]]
    return out


def _run_kernel(forest, csr, **knobs):
    from xgboost_amd.backend.gpu import (_ForestQ, _launch_predict_csr,
                                         _upload_csr)
    dev = torch.device(DEV)
    fa = _ForestQ(forest, range(len(forest.trees)), dev, None)
    indptr, indices, values = _upload_csr(csr, dev)
    n = csr.shape[0]
    out = torch.zeros((n, 1), dtype=torch.float32, device=DEV)
    leaf = torch.full((n, len(forest.trees)), -7, dtype=torch.int32,
                      device=DEV)
    _launch_predict_csr(fa, indptr, indices, values, csr.shape[1], out, leaf,
                        **knobs)
    return leaf.cpu().numpy(), out.cpu().numpy()


# LDS-dense rows up to 64 columns, binary search past them
@pytest.mark.parametrize("F", [6, 64, 65, 300])
def test_kernel_matches_host_leaf_ids(F):
    rng = np.random.RandomState(F)
    forest = _hand_forest(F, rng)
    csr = _hand_rows(F, rng)
    dense = _dense_nan(csr, width=F + 8)  # features past F: missing
    want_leaf = np.stack([t.predict_leaf_np(dense) for t in forest.trees],
                         axis=1)
    assert len(np.unique(want_leaf[:, 0])) == 5  # every leaf of tree a
    assert all(len(np.unique(want_leaf[:, t])) >= 4 for t in range(4, 8))
    want = _host_margin(forest, want_leaf)
    runs = [{}, {"grid_cap": 2}]
    if F == 6:
        runs += [{"force_search": 1}, {"force_search": 1, "grid_cap": 2}]
    for knobs in runs:
        leaf, out = _run_kernel(forest, csr, **knobs)
        assert (leaf != -7).all(), knobs
        assert np.array_equal(leaf, want_leaf), knobs
        assert np.array_equal(out, want), knobs


# -- 2. output-column schemes ---------------------------------------------

@pytest.mark.parametrize("kind,n_out", [("scalar", 1), ("scalar", 3),
                                        ("scalar", 6), ("vector", 3),
                                        ("vector", 6)])
def test_output_columns(monkeypatch, kind, n_out):
    rng, X, csr = _sparse_rows(n_out, 300, 8)
    if kind == "vector":
        y = (X @ rng.randn(8, n_out)).astype(np.float32)
        params = {"objective": "reg:squarederror",
                  "multi_strategy": "multi_output_tree"}
    elif n_out == 1:
        y = (X[:, 0] - X[:, 1]).astype(np.float32)
        params = {"objective": "reg:squarederror"}
    else:
        y = rng.randint(0, n_out, 300).astype(np.float32)
        params = {"objective": "multi:softprob", "num_class": n_out}
    trained = xgb.train(dict(params, max_depth=3, max_bin=32),
                        xgb.DMatrix(csr, label=y), 3, verbose_eval=False)
    assert all((t.leaf_values is not None) == (kind == "vector")
               for t in trained.trees)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    assert gpu.n_outputs == n_out
    bm = (0.5 * rng.randn(300)).astype(np.float32)
    want = cpu.predict(xgb.DMatrix(_dense_nan(csr), base_margin=bm),
                       output_margin=True)
    with _device_only(monkeypatch):
        got = gpu.predict(xgb.DMatrix(csr, base_margin=bm),
                          output_margin=True)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


# -- 3. public API end to end ---------------------------------------------

def test_end_to_end(monkeypatch):
    rng, X, csr = _sparse_rows(0, 400, 6)
    y = (X[:, 0] - X[:, 1] > 0).astype(np.float32)
    trained = xgb.train({"objective": "binary:logistic", "max_depth": 3,
                         "max_bin": 32}, xgb.DMatrix(csr, label=y), 3,
                        verbose_eval=False)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)

    def dense():
        return xgb.DMatrix(_dense_nan(csr))

    want = cpu.predict(dense())
    want_margin = cpu.predict(dense(), output_margin=True)
    leaf_kw = ({}, {"strict_shape": True}, {"iteration_range": (1, 2)})
    want_leaf = [cpu.predict(dense(), pred_leaf=True, **kw)
                 for kw in leaf_kw]
    with _device_only(monkeypatch):
        got = gpu.predict(xgb.DMatrix(csr))
        got_margin = gpu.predict(xgb.DMatrix(csr), output_margin=True)
        got_leaf = [gpu.predict(xgb.DMatrix(csr), pred_leaf=True, **kw)
                    for kw in leaf_kw]
        got_inplace = gpu.inplace_predict(csr)
        got_inplace_margin = gpu.inplace_predict(csr, predict_type="margin")
    # the sigmoid runs in torch on either device: last-bit differences
    assert np.allclose(got, want, rtol=0, atol=1e-6)
    assert np.array_equal(got_margin, want_margin)
    for g, w in zip(got_leaf, want_leaf):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g, w)
    assert np.allclose(got_inplace, want, rtol=0, atol=1e-6)
    assert np.array_equal(got_inplace_margin, want_margin)


# -- 4. eval set during training ------------------------------------------

def test_training_with_csr_eval_set(monkeypatch):
    from xgboost_amd.backend import gpu as gpu_backend
    rng, X, csr = _sparse_rows(21, 600, 10)
    y = (X[:, 0] - X[:, 1] + 0.5 * X[:, 2] > 0).astype(np.float32)
    _, Xe, csr_e = _sparse_rows(22, 333, 10)
    ye = (Xe[:, 0] - Xe[:, 1] + 0.5 * Xe[:, 2] > 0).astype(np.float32)
    params = {"objective": "binary:logistic", "max_depth": 4, "eta": 0.3,
              "max_bin": 32, "eval_metric": "logloss"}
    uploads = []
    upload = gpu_backend._upload_csr

    def counted(m, device):
        uploads.append(m.shape[0])
        return upload(m, device)

    logs = {}
    for device in (DEV, "cpu"):
        d = xgb.DMatrix(csr, label=y)
        de = xgb.DMatrix(csr_e, label=ye)
        logs[device] = {}
        if device == "cpu":
            xgb.train(dict(params, device=device), d, 3, evals=[(de, "ev")],
                      evals_result=logs[device], verbose_eval=False)
            continue
        with _device_only(monkeypatch) as _, monkeypatch.context() as m:
            m.setattr(gpu_backend, "_upload_csr", counted)
            xgb.train(dict(params, device=device), d, 3, evals=[(de, "ev")],
                      evals_result=logs[device], verbose_eval=False)
    assert uploads.count(333) == 1, uploads  # once, not once per round
    got, want = logs[DEV]["ev"]["logloss"], logs["cpu"]["ev"]["logloss"]
    assert len(got) == len(want) == 3
    # tolerance of tests/test_sparse.py::test_sparse_gpu_matches_cpu
    assert np.allclose(got, want, rtol=1e-4, atol=1e-6), (got, want)


# -- 5. DART drop sets ----------------------------------------------------

def test_dart_on_csr(monkeypatch):
    rng = np.random.RandomState(9)
    csr = sp.random(800, 50, density=0.1, format="csr", dtype=np.float32,
                    random_state=rng)
    y = np.asarray(csr @ rng.randn(50)).ravel().astype(np.float32)
    d = xgb.DMatrix(csr, label=y)
    with _device_only(monkeypatch):
        gpu = xgb.train({"booster": "dart", "max_depth": 3, "eta": 0.3,
                         "rate_drop": 0.5, "seed": 5, "max_bin": 32,
                         "device": DEV}, d, 4, verbose_eval=False)
        cached, _ = gpu._cache[id(d)]
        fresh = gpu._predict_margin(d)
        got = gpu.predict(d, output_margin=True)
    assert len(gpu.weight_drop) == 4
    assert any(w != 1.0 for w in gpu.weight_drop)
    # tolerances of tests/test_gpu_predict_q.py::test_dart_extmem
    assert torch.allclose(cached, fresh, atol=1e-3), \
        (cached - fresh).abs().max()
    cpu = _reload(gpu, "cpu")
    assert cpu.weight_drop == pytest.approx(gpu.weight_drop)
    want = cpu.predict(xgb.DMatrix(_dense_nan(csr)), output_margin=True)
    assert np.allclose(got, want, atol=2e-3), np.abs(got - want).max()
