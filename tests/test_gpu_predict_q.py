"""Packed-node GPU predictor (predict_bins.hip): quantized pages, raw
floats with vector leaves, leaf indices.  The oracle is always the CPU
booster loaded from the same model JSON; margins and leaf ids are
compared with exact equality (the kernel adds leaves in tree order with
plain fp32 adds, like the host loops), DART weights excepted.  The
tests at the end go through the public path for dense matrices with
scalar leaves, whichever kernel serves it (today gbt_predict)."""
import contextlib

import numpy as np
import pytest
import torch

import xgboost_amd as xgb
from xgboost_amd.data import QuantizedMatrix, quantize_dense
from xgboost_amd.extmem import DataIter, ExtMemQuantileDMatrix
from xgboost_amd.tree_model import RegTree

pytestmark = pytest.mark.gpu

DEV = "cuda"


class _Iter(DataIter):
    def __init__(self, Xs, ys=None, cache_prefix=None, feature_types=None):
        super().__init__(cache_prefix=cache_prefix)
        self.Xs, self.ys, self.ft, self.i = Xs, ys, feature_types, 0

    def reset(self):
        self.i = 0

    def next(self, input_data) -> bool:
        if self.i >= len(self.Xs):
            return False
        kw = {"data": self.Xs[self.i]}
        if self.ys is not None:
            kw["label"] = self.ys[self.i]
        if self.ft is not None:
            kw["feature_types"] = self.ft
        input_data(**kw)
        self.i += 1
        return True


def _split(a, sizes):
    return np.split(a, np.cumsum(sizes)[:-1])


def _reload(bst, device):
    out = xgb.Booster({"device": device})
    out.load_model(bytes(bst.save_raw("json")))
    return out


def _boom(*a, **k):
    raise AssertionError("host tree walk used on the device path")


@contextlib.contextmanager
def _device_only(monkeypatch, no_global_gidx=False):
    """Every host traversal raises while the block runs."""
    with monkeypatch.context() as m:
        m.setattr(RegTree, "predict_leaf_np", _boom)
        m.setattr(RegTree, "predict_leaf_bins", _boom)
        if no_global_gidx:
            m.setattr(QuantizedMatrix, "global_gidx", _boom)
        yield


def _host_margin(bst, leaf, n_out):
    """Sequential fp32 adds in tree order, from host leaf ids."""
    out = np.zeros((leaf.shape[0], n_out), np.float32)
    for t, tree in enumerate(bst.trees):
        if tree.leaf_values is not None:
            out += tree.leaf_values[:tree.n_nodes][leaf[:, t]]
        else:
            out[:, bst.tree_info[t]] += \
                tree.split_cond[:tree.n_nodes][leaf[:, t]]
    return out


def _run_kernel(bst, X, cuts):
    """Launch gbt_predict_q on X (bins when cuts is given, else floats)."""
    from xgboost_amd.backend.gpu import _ForestQ, _launch_predict_q
    fa = _ForestQ(bst, range(len(bst.trees)), torch.device(DEV), cuts)
    n = X.shape[0]
    out = torch.zeros((n, bst.n_outputs), dtype=torch.float32, device=DEV)
    leaf = torch.full((n, len(bst.trees)), -7, dtype=torch.int32,
                      device=DEV)
    _launch_predict_q(fa, X.to(DEV).contiguous(), float("nan"), out, leaf)
    return leaf.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("max_bin,dtype", [(16, torch.uint8),
                                           (512, torch.int16)])
def test_kernel_matches_predict_leaf_bins(max_bin, dtype, missing):
    rng = np.random.RandomState(max_bin + int(missing))
    X = rng.randn(1000, 5).astype(np.float32)
    if missing:
        X[rng.rand(1000, 5) < 0.1] = np.nan
    y = (np.nan_to_num(X[:, 0]) * np.nan_to_num(X[:, 1])
         + np.nan_to_num(X[:, 2])).astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"max_depth": 5, "max_bin": max_bin, "eta": 0.5}, d, 3,
                    verbose_eval=False)
    stump = RegTree(5)  # root-only tree
    stump.set_leaf(0, 0.25)
    assert stump.n_nodes == 1
    bst.trees.insert(1, stump)
    bst.tree_info.insert(1, 0)
    bst.iteration_indptr.append(bst.iteration_indptr[-1] + 1)
    cuts = d.quantized(max_bin).cuts
    if dtype == torch.int16:
        assert cuts.max_n_bins() > 255
    for n in (1, 257, 1000):
        qm = quantize_dense(X[:n], cuts)
        assert qm.gidx.dtype == dtype
        gg = qm.global_gidx().numpy()
        want_leaf = np.stack([t.predict_leaf_bins(gg, cuts)
                              for t in bst.trees], axis=1)
        leaf, out = _run_kernel(bst, qm.gidx, cuts)
        assert np.array_equal(leaf, want_leaf), n
        assert np.array_equal(out, _host_margin(bst, want_leaf, 1)), n


def test_kernel_categorical_bins_and_raw():
    rng = np.random.RandomState(21)
    n = 700
    cat = rng.randint(0, 40, n).astype(np.float32)
    Xn = rng.randn(n, 3).astype(np.float32)
    X = np.concatenate([cat[:, None], Xn], axis=1)
    X[rng.rand(n, 4) < 0.08] = np.nan
    good = [1, 5, 7, 12, 19, 22, 28, 33, 36, 39]
    y = (np.isin(cat, good) * 2.0 + 0.5 * np.nan_to_num(Xn[:, 0])
         + 0.1 * rng.randn(n)).astype(np.float32)
    d = xgb.DMatrix(X, label=y, feature_types=["c", "q", "q", "q"])
    bst = xgb.train({"max_depth": 4, "max_bin": 16, "max_cat_to_onehot": 1,
                     "eta": 0.5}, d, 4, verbose_eval=False)
    # a set split whose bitset crosses the first 32-bit word
    assert any(len(c) > 1 and int(c.max()) >= 32 for t in bst.trees
               for c in t.cat_segments.values())
    cuts = d.quantized(16).cuts
    qm = quantize_dense(X, cuts)
    gg = qm.global_gidx().numpy()
    want_bins = np.stack([t.predict_leaf_bins(gg, cuts) for t in bst.trees],
                         axis=1)
    leaf, out = _run_kernel(bst, qm.gidx, cuts)
    assert np.array_equal(leaf, want_bins)
    assert np.array_equal(out, _host_margin(bst, want_bins, 1))
    want_raw = np.stack([t.predict_leaf_np(X) for t in bst.trees], axis=1)
    leaf, out = _run_kernel(bst, torch.from_numpy(X), None)
    assert np.array_equal(leaf, want_raw)
    assert np.array_equal(out, _host_margin(bst, want_raw, 1))


def _vector_data(seed=5, n=300, f=6):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, f).astype(np.float32)
    X[rng.rand(n, f) < 0.05] = np.nan
    W = rng.randn(f, 3)
    Y = (np.nan_to_num(X) @ W + 0.1 * rng.randn(n, 3)).astype(np.float32)
    return X, Y


def test_vector_leaves_dense_raw(monkeypatch):
    X, Y = _vector_data()
    trained = xgb.train({"objective": "reg:squarederror", "max_depth": 4,
                         "multi_strategy": "multi_output_tree", "eta": 0.3,
                         "max_bin": 32}, xgb.DMatrix(X, label=Y), 5,
                        verbose_eval=False)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    assert all(t.leaf_values is not None for t in gpu.trees)
    d = xgb.DMatrix(X)
    want = cpu.predict(d)
    want_margin = cpu.predict(d, output_margin=True)
    want_range = cpu.predict(d, iteration_range=(1, 3))
    with _device_only(monkeypatch):
        got = gpu.predict(xgb.DMatrix(X))
        got_margin = gpu.predict(xgb.DMatrix(X), output_margin=True)
        got_range = gpu.predict(xgb.DMatrix(X), iteration_range=(1, 3))
        got_inplace = gpu.inplace_predict(torch.from_numpy(X).to(DEV))
    assert got.shape == (300, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(got_margin, want_margin)
    assert np.array_equal(got_range, want_range)
    assert np.array_equal(got_inplace, want)


def test_mixed_scalar_and_vector_forest(monkeypatch):
    X, Y = _vector_data(seed=8)
    d = xgb.DMatrix(X, label=Y)
    a = xgb.train({"multi_strategy": "multi_output_tree", "max_depth": 3,
                   "max_bin": 32}, d, 2, verbose_eval=False)
    mixed = xgb.train({"multi_strategy": "one_output_per_tree",
                       "max_depth": 3, "max_bin": 32}, d, 2, xgb_model=a,
                      verbose_eval=False)
    kinds = [t.leaf_values is not None for t in mixed.trees]
    assert any(kinds) and not all(kinds)
    cpu, gpu = _reload(mixed, "cpu"), _reload(mixed, DEV)
    want = cpu.predict(xgb.DMatrix(X))
    want_leaf = cpu.predict(xgb.DMatrix(X), pred_leaf=True)
    sizes = [120, 1, 179]
    d_ext = ExtMemQuantileDMatrix(_Iter(_split(X, sizes)), max_bin=32, ref=d)
    with _device_only(monkeypatch, no_global_gidx=True):
        got = gpu.predict(xgb.DMatrix(X))
        got_ext = gpu.predict(d_ext)
        got_leaf = gpu.predict(d_ext, pred_leaf=True)
    assert np.array_equal(got, want)
    assert np.array_equal(got_ext, want)
    assert np.array_equal(got_leaf, want_leaf)


@pytest.mark.parametrize("spill", [False, True])
def test_extmem_end_to_end(monkeypatch, tmp_path, spill):
    rng = np.random.RandomState(17)
    sizes = [401, 1, 198]
    X = rng.randn(600, 5).astype(np.float32)
    X[rng.rand(600, 5) < 0.1] = np.nan
    y = (np.nan_to_num(X[:, 0]) - 0.5 * np.nan_to_num(X[:, 1])
         + 0.1 * rng.randn(600)).astype(np.float32)
    Xe = rng.randn(333, 5).astype(np.float32)
    ye = (Xe[:, 0] - 0.5 * Xe[:, 1]).astype(np.float32)
    esizes = [100, 232, 1]

    def mats():
        kw = {}
        pre = [None, None]
        if spill:  # only page 0 fits the budget: later pages go to disk
            kw = {"max_host_cache_bytes": 1}
            pre = [str(tmp_path / "tr"), str(tmp_path / "ev")]
        dt = ExtMemQuantileDMatrix(
            _Iter(_split(X, sizes), _split(y, sizes), cache_prefix=pre[0]),
            max_bin=32, **kw)
        de = ExtMemQuantileDMatrix(
            _Iter(_split(Xe, esizes), _split(ye, esizes),
                  cache_prefix=pre[1]), max_bin=32, ref=dt, **kw)
        if spill:
            assert dt.store.is_disk(1) and de.store.is_disk(2)
        return dt, de

    rounds = 4
    params = {"objective": "reg:squarederror", "max_depth": 4, "eta": 0.3,
              "max_bin": 32, "eval_metric": "rmse"}
    dt, de = mats()
    log = {}
    with _device_only(monkeypatch, no_global_gidx=True):
        gpu = xgb.train(dict(params, device=DEV), dt, rounds,
                        evals=[(de, "ev")], evals_result=log,
                        verbose_eval=False)
        got = gpu.predict(de)
        got_train = gpu.predict(dt)
        got_rounds = [gpu.predict(de, iteration_range=(0, i + 1))
                      for i in range(rounds)]
    cpu = _reload(gpu, "cpu")
    dt_c, de_c = mats()
    assert np.array_equal(got, cpu.predict(de_c))
    assert np.array_equal(got_train, cpu.predict(dt_c))
    for i in range(rounds):
        want = cpu.predict(de_c, iteration_range=(0, i + 1))
        assert np.array_equal(got_rounds[i], want), i
        # the log keeps five decimals of a device fp32 reduction over the
        # same margins: it equals the host value to that resolution
        rmse = float(np.sqrt(np.mean((want.astype(np.float64) - ye) ** 2)))
        assert log["ev"]["rmse"][i] == pytest.approx(rmse, abs=1e-5), i


def test_dart_extmem(monkeypatch):
    rng = np.random.RandomState(31)
    sizes = [300, 150, 450]
    X = rng.randn(900, 5).astype(np.float32)
    y = (X[:, 0] * 1.2 - X[:, 1] + 0.1 * rng.randn(900)).astype(np.float32)
    params = {"max_depth": 3, "eta": 0.3, "rate_drop": 0.5, "seed": 3,
              "max_bin": 32}
    d = ExtMemQuantileDMatrix(_Iter(_split(X, sizes), _split(y, sizes)),
                              max_bin=32)
    with _device_only(monkeypatch, no_global_gidx=True):
        gpu = xgb.train(dict(params, device=DEV), d, 6, verbose_eval=False)
        cached, _ = gpu._cache[id(d)]
        fresh = gpu._predict_margin(d)
        got = gpu.predict(d, output_margin=True)
    assert len(gpu.weight_drop) == 6
    assert any(w != 1.0 for w in gpu.weight_drop)
    # tolerances of tests/test_gpu.py::test_dart_on_device
    assert torch.allclose(cached, fresh, atol=1e-3), \
        (cached - fresh).abs().max()
    cpu = _reload(gpu, "cpu")
    assert cpu.weight_drop == pytest.approx(gpu.weight_drop)
    d_c = ExtMemQuantileDMatrix(_Iter(_split(X, sizes), _split(y, sizes)),
                                max_bin=32)
    want = cpu.predict(d_c, output_margin=True)
    assert np.allclose(got, want, atol=2e-3), np.abs(got - want).max()


def test_pred_leaf_on_device(monkeypatch):
    rng = np.random.RandomState(4)
    X = rng.randn(500, 6).astype(np.float32)
    X[rng.rand(500, 6) < 0.05] = np.nan
    y = rng.randint(0, 3, 500).astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    trained = xgb.train({"objective": "multi:softprob", "num_class": 3,
                         "num_parallel_tree": 2, "max_depth": 3,
                         "max_bin": 32}, d, 3, verbose_eval=False)
    assert len(trained.trees) == 18
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    cpu.set_param({"num_parallel_tree": 2})
    gpu.set_param({"num_parallel_tree": 2})
    sizes = [250, 1, 249]
    d_ext = ExtMemQuantileDMatrix(_Iter(_split(X, sizes)), max_bin=32, ref=d)
    want = cpu.predict(xgb.DMatrix(X), pred_leaf=True)
    want_strict = cpu.predict(xgb.DMatrix(X), pred_leaf=True,
                              strict_shape=True)
    want_range = cpu.predict(xgb.DMatrix(X), pred_leaf=True,
                             iteration_range=(1, 2))
    assert want_strict.shape == (500, 3, 3, 2)
    with _device_only(monkeypatch, no_global_gidx=True):
        for dm in (xgb.DMatrix(X), d_ext):
            got = gpu.predict(dm, pred_leaf=True)
            assert got.dtype == want.dtype and got.shape == (500, 18)
            assert np.array_equal(got, want)
            got = gpu.predict(dm, pred_leaf=True, strict_shape=True)
            assert got.shape == want_strict.shape
            assert np.array_equal(got, want_strict)
            got = gpu.predict(dm, pred_leaf=True, iteration_range=(1, 2))
            assert np.array_equal(got, want_range)
        # margins of the same multiclass forest from the pages
        got_margin = gpu.predict(d_ext, output_margin=True)
    assert np.array_equal(got_margin,
                          cpu.predict(xgb.DMatrix(X), output_margin=True))


def test_host_fallbacks_still_predict():
    """Sparse CSR input and a re-aligned categorical frame keep their
    host paths under device="cuda"."""
    import pandas as pd
    import scipy.sparse as sp
    rng = np.random.RandomState(0)
    X = rng.randn(400, 6).astype(np.float32)
    X[rng.rand(400, 6) < 0.6] = 0.0
    y = (X[:, 0] - X[:, 1] > 0).astype(np.float32)
    csr = sp.csr_matrix(X)
    trained = xgb.train({"objective": "binary:logistic", "max_depth": 3,
                         "max_bin": 32}, xgb.DMatrix(csr, label=y), 3,
                        verbose_eval=False)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    # the sigmoid runs in torch on either device: last-bit differences
    assert np.allclose(gpu.predict(xgb.DMatrix(csr)),
                       cpu.predict(xgb.DMatrix(csr)), rtol=0, atol=1e-6)
    assert np.array_equal(
        gpu.predict(xgb.DMatrix(csr), output_margin=True),
        cpu.predict(xgb.DMatrix(csr), output_margin=True))

    n = 600
    colors = rng.choice(["red", "green", "blue"], n)
    df = pd.DataFrame({"color": pd.Categorical(colors),
                       "x": rng.randn(n).astype(np.float32)})
    yc = ((colors == "red") * 2.0).astype(np.float32)
    d = xgb.DMatrix(df, label=yc, enable_categorical=True)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 3,
                     "device": DEV}, d, 4, verbose_eval=False)
    p_train = bst.predict(d)
    df2 = df.copy()
    df2["color"] = pd.Categorical(colors,
                                  categories=["blue", "red", "green"])
    d2 = xgb.DMatrix(df2, enable_categorical=True)
    assert np.allclose(bst.predict(d2), p_train, atol=1e-6)


# -- dense matrices, scalar leaves: the public prediction path -------------

def _scalar_model(n_out, missing):
    """CPU-trained scalar-leaf forest (5 features, depth 4, 3 rounds) and
    its rows; missing entries carry `missing` (NaN or a finite sentinel)."""
    rng = np.random.RandomState(50 + n_out)
    X = rng.randn(1000, 5).astype(np.float32)
    X[rng.rand(1000, 5) < 0.15] = missing
    Xz = np.where(X == missing, 0.0, np.nan_to_num(X))
    params = {"max_depth": 4, "eta": 0.5, "max_bin": 32}
    if n_out == 1:
        y = (Xz[:, 0] * Xz[:, 1] + Xz[:, 2]).astype(np.float32)
        params["objective"] = "reg:squarederror"
    else:
        y = np.argmax(Xz[:, :n_out] + 0.3 * rng.randn(1000, n_out)[:, :5],
                      axis=1).astype(np.float32)
        params.update(objective="multi:softprob", num_class=n_out)
    bst = xgb.train(params, xgb.DMatrix(X, label=y, missing=missing), 3,
                    verbose_eval=False)
    assert bst.n_outputs == n_out and len(bst.trees) == 3 * n_out
    assert all(t.leaf_values is None for t in bst.trees)
    bm = rng.randn(1000, n_out).astype(np.float32)
    return bst, X, bm


@pytest.mark.parametrize("missing", [np.nan, -1.0])
@pytest.mark.parametrize("n_out", [1, 3, 5])
def test_dense_scalar_public_path(monkeypatch, n_out, missing):
    """bst.predict / inplace_predict on a dense matrix with a scalar-leaf
    forest equal the CPU booster exactly: 1, 3 and 5 output columns, NaN
    and finite-sentinel missing values, a non-zero base_margin."""
    trained, X, bm = _scalar_model(n_out, missing)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    if not np.isnan(missing):
        assert (X == missing).any()
    for n in (1, 257, 1000):
        def dm():
            return xgb.DMatrix(X[:n], missing=missing, base_margin=bm[:n])
        for rng_ in ((0, 0), (1, 3)):
            want = cpu.predict(dm(), output_margin=True,
                               iteration_range=rng_)
            with _device_only(monkeypatch):
                got = gpu.predict(dm(), output_margin=True,
                                  iteration_range=rng_)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (n, rng_)
        want = cpu.predict(dm(), output_margin=True)
        want_plain = cpu.predict(xgb.DMatrix(X[:n], missing=missing),
                                 output_margin=True)
        assert not np.array_equal(want, want_plain)
        Xd = torch.from_numpy(X[:n]).to(DEV)
        with _device_only(monkeypatch):
            got = gpu.inplace_predict(Xd, missing=missing,
                                      predict_type="margin",
                                      base_margin=bm[:n])
            got_plain = gpu.inplace_predict(Xd, missing=missing,
                                            predict_type="margin")
        assert np.array_equal(got, want), n
        assert np.array_equal(got_plain, want_plain), n


def test_dense_categorical_public_path(monkeypatch):
    """A set split that crosses the first 32-bit bitset word, walked on
    raw floats through bst.predict."""
    rng = np.random.RandomState(21)
    n = 700
    cat = rng.randint(0, 40, n).astype(np.float32)
    Xn = rng.randn(n, 3).astype(np.float32)
    X = np.concatenate([cat[:, None], Xn], axis=1)
    X[rng.rand(n, 4) < 0.08] = np.nan
    good = [1, 5, 7, 12, 19, 22, 28, 33, 36, 39]
    y = (np.isin(cat, good) * 2.0 + 0.5 * np.nan_to_num(Xn[:, 0])
         + 0.1 * rng.randn(n)).astype(np.float32)
    ft = ["c", "q", "q", "q"]
    trained = xgb.train({"max_depth": 4, "max_bin": 16,
                         "max_cat_to_onehot": 1, "eta": 0.5},
                        xgb.DMatrix(X, label=y, feature_types=ft), 4,
                        verbose_eval=False)
    assert any(len(c) > 1 and int(c.max()) >= 32 for t in trained.trees
               for c in t.cat_segments.values())
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    want = cpu.predict(xgb.DMatrix(X, feature_types=ft), output_margin=True)
    want_leaf = cpu.predict(xgb.DMatrix(X, feature_types=ft), pred_leaf=True)
    with _device_only(monkeypatch):
        got = gpu.predict(xgb.DMatrix(X, feature_types=ft),
                          output_margin=True)
        got_leaf = gpu.predict(xgb.DMatrix(X, feature_types=ft),
                               pred_leaf=True)
    assert np.array_equal(got, want)
    assert np.array_equal(got_leaf, want_leaf)


def test_dart_drop_set_dense(monkeypatch):
    """_predict_tree_subset and _predict_margin of a cuda DART booster on
    a dense matrix against explicit per-tree fp32 adds of w * leaf."""
    rng = np.random.RandomState(33)
    X = rng.randn(700, 4).astype(np.float32)
    X[rng.rand(700, 4) < 0.05] = np.nan
    y = (np.nan_to_num(X[:, 0]) * 1.2 - np.nan_to_num(X[:, 1])
         + 0.1 * rng.randn(700)).astype(np.float32)
    trained = xgb.train({"booster": "dart", "max_depth": 3, "eta": 0.3,
                         "rate_drop": 0.5, "seed": 3, "max_bin": 32},
                        xgb.DMatrix(X, label=y), 8, verbose_eval=False)
    gpu = _reload(trained, DEV)
    assert len(gpu.weight_drop) == 8
    idxs = [1, 2, 4, 7]
    assert any(gpu.weight_drop[t] != 1.0 for t in idxs)
    leaf = np.stack([t.predict_leaf_np(X) for t in gpu.trees], axis=1)

    def oracle(start, trees):
        out = np.full((700, 1), start, np.float32)
        for t in trees:
            tree = gpu.trees[t]
            vals = tree.split_cond[:tree.n_nodes][leaf[:, t]]
            out[:, gpu.tree_info[t]] += (vals.astype(np.float32)
                                         * np.float32(gpu.weight_drop[t]))
        return out

    d = xgb.DMatrix(X)
    with _device_only(monkeypatch):
        got_sub = gpu._predict_tree_subset(d, idxs).cpu().numpy()
        got_all = gpu._predict_margin(d).cpu().numpy()
    assert np.array_equal(got_sub, oracle(0.0, idxs))
    assert np.array_equal(got_all,
                          oracle(gpu._base_margin_value(), range(8)))


def test_vector_leaf_drop_set_dense(monkeypatch):
    """The drop-set helper on a dense matrix with vector leaves walks on
    the device like the margin does."""
    X, Y = _vector_data(seed=9)
    trained = xgb.train({"objective": "reg:squarederror", "max_depth": 4,
                         "multi_strategy": "multi_output_tree", "eta": 0.3,
                         "max_bin": 32}, xgb.DMatrix(X, label=Y), 5,
                        verbose_eval=False)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    want = cpu._predict_tree_subset(xgb.DMatrix(X), [0, 2, 3]).numpy()
    assert want.shape == (300, 3) and np.abs(want).max() > 0
    with _device_only(monkeypatch):
        got = gpu._predict_tree_subset(xgb.DMatrix(X), [0, 2, 3])
    assert np.array_equal(got.cpu().numpy(), want)
