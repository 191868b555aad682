"""SHAP on sparse CSR input, device path: the gather kernel
(shap_csr.hip) alone, then pred_contribs / pred_interactions through the
public API.  Boosters are built on the CPU and reloaded on the device.
The oracle is the same booster on the same rows as a dense matrix with
NaN for every absent entry: the device result on it (the same kernels on
the same values in the same order, so equal after its fp64 output is
rounded to the float32 the CSR route returns) and the CPU booster
(within the bounds tests/test_gpu.py uses).  While the device assertions
run the host recursion raises, so a silent fallback fails the test."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import shap_cases as sc
import xgboost_amd as xgb
from xgboost_amd.tree_model import RegTree
from test_shap_csr import (_categorical_forest, _comb, _dense_nan,
                           _hand_booster, _missing_case, _reload,
                           _sparse_rows, _split, _three_column_forest,
                           _train, _wide_rows)

pytestmark = pytest.mark.gpu

DEV = "cuda"


@contextlib.contextmanager
def _device_only(monkeypatch, chunk_rows=None):
    """The host recursion raises while the block runs; yields the row
    counts of the chunks the gather kernel staged."""
    from xgboost_amd import shap
    from xgboost_amd.backend import gpu as gpu_backend
    gather = gpu_backend._gather_csr_columns
    chunks = []

    def counted(csr_dev, row_begin, col_map, tile):
        chunks.append((row_begin, tile.shape[1]))
        return gather(csr_dev, row_begin, col_map, tile)

    with sc.host_recursion_raises(monkeypatch, shap) as m:
        m.setattr(gpu_backend, "_gather_csr_columns", counted)
        m.setattr(gpu_backend, "_SHAP_CSR_CHUNK_ROWS", chunk_rows)
        yield chunks


def _dense_device(gpu, csr, monkeypatch, **mode):
    """The device result on the dense-NaN matrix, as float32."""
    with _device_only(monkeypatch):
        out = gpu.predict(xgb.DMatrix(_dense_nan(csr)), **mode)
    return out.astype(np.float32)


# -- 1. the gather kernel alone -------------------------------------------

def _gather_case():
    """300 rows over 41 columns; col_map covers 40 of them and maps 5."""
    n, F = 300, 40
    rng = np.random.RandomState(0)
    used = np.array([2, 9, 17, 30, 39])
    keep = rng.rand(n, F + 1) < 0.3
    keep[:, F] = False
    keep[0] = False          # empty row
    keep[1, :F] = True       # full row
    keep[7, F] = True        # a column index >= n_col_map
    X = rng.randn(n, F + 1).astype(np.float32)
    X[3, 9] = np.nan
    X[4, 17] = 0.0
    keep[3, 9] = keep[4, 17] = True
    rows, cols = np.nonzero(keep)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    csr = sp.csr_matrix((X[rows, cols], cols.astype(np.int32), indptr),
                        shape=(n, F + 1))
    assert keep[:, np.setdiff1d(np.arange(F), used)].any()
    col_map = np.full(F, -1, np.int32)
    col_map[used] = np.arange(5, dtype=np.int32)
    want = np.full((5, n), np.nan, np.float32)  # numpy scatter
    for u, c in enumerate(used):
        want[u, keep[:, c]] = X[keep[:, c], c]
    return csr, col_map, want


@pytest.mark.parametrize("row_begin,rows", [(0, 300), (113, 187), (64, 65),
                                            (299, 1)])
def test_gather_kernel(row_begin, rows):
    from xgboost_amd.backend.gpu import _gather_csr_columns, _upload_csr
    csr, col_map, want = _gather_case()
    dev = torch.device(DEV)
    tile = torch.zeros((5, rows), dtype=torch.float32, device=dev)
    _gather_csr_columns(_upload_csr(csr, dev), row_begin,
                        torch.from_numpy(col_map).to(dev), tile)
    got = tile.cpu().numpy()
    want = want[:, row_begin:row_begin + rows]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, want, equal_nan=True)
    if row_begin == 0:
        assert np.isnan(got[:, 0]).all() and not np.isnan(got[:, 1]).any()
        assert got[2, 4] == 0.0 and np.isnan(got[1, 3])


# -- 2. numeric forest, path length <= 8 ----------------------------------

@pytest.mark.parametrize("n,chunk_rows,n_chunks", [
    (300, 100, 3), (300, 128, 3), (300, None, 1), (1, None, 1)])
def test_contribs_numeric(monkeypatch, n, chunk_rows, n_chunks):
    trained = _train(6)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    csr = _sparse_rows(3, 300, 6)[300 - n:]
    want_cpu = cpu.predict(xgb.DMatrix(_dense_nan(csr)), pred_contribs=True)
    want_dev = _dense_device(gpu, csr, monkeypatch, pred_contribs=True)
    d = xgb.DMatrix(csr)
    with _device_only(monkeypatch, chunk_rows) as chunks:
        got = gpu.predict(d, pred_contribs=True)
        margin = gpu.predict(d, output_margin=True)
    assert len(chunks) == n_chunks and sum(c[1] for c in chunks) == n
    assert got.dtype == np.float32 and got.shape == (n, 7)
    assert np.array_equal(got, want_dev)
    assert np.allclose(got, want_cpu, rtol=0, atol=1e-4), \
        np.abs(got - want_cpu).max()
    # 8. contributions sum to the device CSR margin
    assert np.allclose(got.sum(axis=1), margin, rtol=0, atol=1e-3)
    # 9. one device copy of the CSR, however many calls
    assert len(d._device_csr_cache) == 1


# -- 3. path length 9-16 ---------------------------------------------------

def test_contribs_paths16_wide(monkeypatch):
    from xgboost_amd.backend import gpu as gpu_backend
    F = 2000
    feats = np.linspace(5, 1990, 12).astype(int)
    bst = _hand_booster([_comb(F, feats)]
                        + _three_column_forest(F, feats[[1, 5, 9]]), F)
    cpu, gpu = _reload(bst, "cpu"), _reload(bst, DEV)
    csr = _wide_rows(2, 70, F, feats)
    want_cpu = cpu.predict(xgb.DMatrix(_dense_nan(csr)), pred_contribs=True)
    want_dev = _dense_device(gpu, csr, monkeypatch, pred_contribs=True)
    launch = gpu_backend._launch_shap_paths
    seen = []

    def spy(tab, Xt, n, n_features, *rest):
        seen.append((tab.max_elems, n_features))
        return launch(tab, Xt, n, n_features, *rest)

    with _device_only(monkeypatch), monkeypatch.context() as m:
        m.setattr(gpu_backend, "_launch_shap_paths", spy)
        got = gpu.predict(xgb.DMatrix(csr), pred_contribs=True)
    assert seen == [(12, 12)]  # gbt_shap_paths16 in compact space
    assert got.shape == (70, F + 1)
    assert np.array_equal(got, want_dev)
    assert np.allclose(got, want_cpu, rtol=0, atol=1e-4), \
        np.abs(got - want_cpu).max()
    assert not got[:, np.setdiff1d(np.arange(F), feats)].any()


# -- 4. path length 17: the host fallback ----------------------------------

def test_contribs_path17_falls_back(monkeypatch):
    F = 2000
    feats = np.linspace(5, 1990, 17).astype(int)
    bst = _hand_booster([_comb(F, feats)], F)
    cpu, gpu = _reload(bst, "cpu"), _reload(bst, DEV)
    csr = _wide_rows(4, 5, F, feats)
    with _device_only(monkeypatch), pytest.raises(AssertionError,
                                                  match="host SHAP"):
        gpu.predict(xgb.DMatrix(csr), pred_contribs=True)
    got = gpu.predict(xgb.DMatrix(csr), pred_contribs=True)
    assert np.array_equal(got, cpu.predict(xgb.DMatrix(csr),
                                           pred_contribs=True))
    assert np.array_equal(
        got, cpu.predict(xgb.DMatrix(_dense_nan(csr)), pred_contribs=True))


def test_bug_in_device_code_is_not_swallowed(monkeypatch):
    from xgboost_amd.backend import gpu as gpu_backend
    gpu = _reload(_train(6), DEV)
    csr = _sparse_rows(3, 20, 6)

    def broken(*a, **k):
        raise AttributeError("a bug, not a limit")

    monkeypatch.setattr(gpu_backend, "_gather_csr_columns", broken)
    for mode in ({"pred_contribs": True}, {"pred_interactions": True}):
        with pytest.raises(AttributeError, match="a bug"):
            gpu.predict(xgb.DMatrix(csr), **mode)


# -- 5. multiclass and interactions ----------------------------------------

@pytest.mark.parametrize("chunk_rows", [100, None])
def test_contribs_multiclass(monkeypatch, chunk_rows):
    trained = _train(6, n_class=3, rounds=2)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    csr = _sparse_rows(5, 300, 6)
    want_cpu = cpu.predict(xgb.DMatrix(_dense_nan(csr)), pred_contribs=True)
    want_dev = _dense_device(gpu, csr, monkeypatch, pred_contribs=True)
    with _device_only(monkeypatch, chunk_rows):
        got = gpu.predict(xgb.DMatrix(csr), pred_contribs=True)
        margin = gpu.predict(xgb.DMatrix(csr), output_margin=True)
    assert got.shape == (300, 3, 7)
    assert np.array_equal(got, want_dev)
    assert np.allclose(got, want_cpu, rtol=0, atol=1e-4), \
        np.abs(got - want_cpu).max()
    assert np.allclose(got.sum(axis=2), margin, rtol=0, atol=1e-3)


@pytest.mark.parametrize("n_class", [1, 3])
def test_interactions(monkeypatch, n_class):
    trained = _train(6, n_class=n_class, rounds=2)
    cpu, gpu = _reload(trained, "cpu"), _reload(trained, DEV)
    csr = _sparse_rows(6, 130, 6)
    want_cpu = cpu.predict(xgb.DMatrix(_dense_nan(csr)),
                           pred_interactions=True)
    want_dev = _dense_device(gpu, csr, monkeypatch, pred_interactions=True)
    with _device_only(monkeypatch, 64) as chunks:
        got = gpu.predict(xgb.DMatrix(csr), pred_interactions=True)
    assert [c[1] for c in chunks] == [64, 64, 2]
    assert got.dtype == np.float32 and got.shape == want_cpu.shape
    assert np.array_equal(got, want_dev)
    assert np.allclose(got, want_cpu, rtol=0, atol=2e-4), \
        np.abs(got - want_cpu).max()


def test_interactions_wide_run_in_compact_space(monkeypatch):
    F, n = 2000, 9
    feats = np.array([3, 700, 1200, 1999])
    bst = _hand_booster([_comb(F, feats)]
                        + _three_column_forest(F, feats[[0, 1, 3]]), F)
    cpu, gpu = _reload(bst, "cpu"), _reload(bst, DEV)
    csr = _wide_rows(8, n, F, feats)
    want_cpu = cpu.predict(xgb.DMatrix(csr), pred_interactions=True)
    d = xgb.DMatrix(csr)
    with _device_only(monkeypatch):
        gpu.predict(d, pred_contribs=True)  # CSR and tables uploaded
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        got = gpu.predict(d, pred_interactions=True)
        peak = torch.cuda.max_memory_allocated() - before
    # the full-width cube is n * (F + 1)^2 * 8 = 288 MB
    assert peak < (8 << 20), peak
    assert got.shape == (n, F + 1, F + 1)
    assert np.allclose(got, want_cpu, rtol=0, atol=2e-4), \
        np.abs(got - want_cpu).max()
    unused = np.setdiff1d(np.arange(F), feats)
    assert not got[:, unused, :].any() and not got[:, :, unused].any()
    assert got[:, feats, :][:, :, feats].any()


# -- 6. categorical forest on a wide matrix --------------------------------

@pytest.mark.parametrize("F", [50, 2000])
def test_contribs_categorical(monkeypatch, F):
    from xgboost_amd.backend import gpu as gpu_backend
    cols = [int(c * (F - 1) / 49) for c in (0, 7, 20, 33, 41, 49)]
    cat_col = int(12 * (F - 1) / 49)
    bst = _hand_booster(_categorical_forest(F, cols, cat_col), F)
    cpu, gpu = _reload(bst, "cpu"), _reload(bst, DEV)
    csr = _wide_rows(9, 150, F, cols + [cat_col], cat_col=cat_col)
    cats = csr[:, cat_col].toarray().ravel()
    assert np.isin(cats, [1, 5, 33, 40]).any() and (cats > 32).any()
    want_cpu = cpu.predict(xgb.DMatrix(_dense_nan(csr)), pred_contribs=True)
    launch = gpu_backend._launch_shap_dfs
    seen = []

    def spy(fa, X, n, n_features, *rest):
        seen.append(n_features)
        return launch(fa, X, n, n_features, *rest)

    with _device_only(monkeypatch, 100), monkeypatch.context() as m:
        m.setattr(gpu_backend, "_launch_shap_dfs", spy)
        got = gpu.predict(xgb.DMatrix(csr), pred_contribs=True)
    assert seen == [7, 7]  # the DFS kernel, twice, over U = 7 columns
    assert got.shape == (150, F + 1)
    assert np.allclose(got, want_cpu, rtol=0, atol=1e-4), \
        np.abs(got - want_cpu).max()
    assert got[:, cat_col].any()
    if F + 1 <= 129:  # the dense route has the DFS kernel at this width
        want_dev = _dense_device(gpu, csr, monkeypatch, pred_contribs=True)
        assert np.array_equal(got, want_dev)


# -- 7. missing semantics ---------------------------------------------------

@pytest.mark.parametrize("mode", [{"pred_contribs": True},
                                  {"pred_interactions": True}],
                         ids=lambda m: "-".join(m))
def test_missing_semantics(monkeypatch, mode):
    bst, csr = _missing_case()
    gpu = _reload(bst, DEV)
    with _device_only(monkeypatch):
        got = gpu.predict(xgb.DMatrix(csr), **mode)
    assert np.array_equal(got[0], got[2])      # absent == stored NaN
    assert not np.array_equal(got[1], got[0])  # a stored 0.0 is a value
    want = _reload(bst, "cpu").predict(xgb.DMatrix(_dense_nan(csr)), **mode)
    assert np.allclose(got, want, rtol=0, atol=1e-4)


def test_out_of_width_split_raises():
    tree = RegTree(6)
    _split(tree, 0, 7, 0.0, True)
    gpu = _reload(_hand_booster([tree], 6), DEV)
    csr = _sparse_rows(11, 9, 6)
    for mode in ({"pred_contribs": True}, {"pred_interactions": True}):
        with pytest.raises(ValueError, match=r"feature 7\b.*\b6 columns"):
            gpu.predict(xgb.DMatrix(csr), **mode)
    assert gpu.predict(xgb.DMatrix(csr)).shape == (9,)
