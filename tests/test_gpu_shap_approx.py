"""approx_contribs (Saabas) on the device: shap_saabas.hip through the
public API, dense and CSR.  Boosters are built on the CPU and reloaded on
the device; the reference is the CPU booster on the same rows (the fp64
host loop shap._saabas).  While the device runs, the host loop raises.

Bound: both sides add the same fp64 terms in the same order, so they
differ by the fp64 rounding of the means and the final float32 cast: one
float32 ulp of the reference element plus 2^-40 * n_trees * 2 *
max|leaf value| for cancellation.  Rows sum to the margin within the 1e-3
the other device SHAP tests use."""
import numpy as np
import pytest
import torch

import shap_cases as sc
import xgboost_amd as xgb
from xgboost_amd.tree_model import RegTree
from test_shap_csr import (_categorical_forest, _comb, _dense_nan,
                           _hand_booster, _reload, _sparse_rows, _split,
                           _stump, _three_column_forest, _train, _wide_rows)

pytestmark = pytest.mark.gpu

DEV = "cuda"
APPROX = {"pred_contribs": True, "approx_contribs": True}


def _one_column():
    """Every split on column 3, twice on one path, and a stump."""
    a = RegTree(5)
    l, _ = _split(a, 0, 3, 0.0, True)
    _split(a, l, 3, -0.5, False)
    return _hand_booster([a, _stump(5)], 5), sc.rows(1, 65, 5)


def _missing(missing):
    trees = sc.random_forest(11, 6, 6, 4)
    dirs = np.concatenate([t.default_left[:t.n_nodes][t.left[:t.n_nodes] != -1]
                           for t in trees])
    assert dirs.any() and not dirs.all()  # both default directions
    return sc.booster(trees, 6), sc.rows(11, 65, 6, missing)


def _categorical(deep):
    """With `deep` a 17-level comb joins the forest: past the DFS
    kernel's depth cap, so exact SHAP leaves the device."""
    F, cols, cat_col = 50, [0, 7, 20, 33, 41, 49], 12
    trees = _categorical_forest(F, cols, cat_col)
    if deep:
        trees.append(_comb(F, np.arange(17) + 13))
    return (_hand_booster(trees, F),
            _wide_rows(9, 150, F, cols + [cat_col], cat_col=cat_col))


def _seven_columns():
    feats = np.array([2, 5, 11, 17, 23, 31, 39])
    trees = [_comb(40, feats)] + _three_column_forest(40, feats[[1, 3, 6]])
    return _hand_booster(trees, 40), _wide_rows(2, 70, 40, feats)


# name: (booster, rows as an array or a CSR matrix), keywords
CASES = {
    "rows1": (lambda: (_train(6), _sparse_rows(3, 300, 6)[299:]), {}),
    "rows63": (lambda: (_train(6), _sparse_rows(3, 300, 6)[:63]), {}),
    "rows65": (lambda: (_train(6), _sparse_rows(3, 300, 6)[:65]), {}),
    "tile+1": (lambda: (_train(6), _sparse_rows(3, 300, 6)), {"tile": 1}),
    "one-column-stump": (_one_column, {}),
    "feature-twice": (lambda: (
        _hand_booster(_three_column_forest(9, [1, 4, 7]), 9),
        sc.rows(2, 70, 9)), {}),
    "missing-nan": (lambda: _missing(np.nan), {}),
    "missing-sentinel": (lambda: _missing(sc.SENTINEL),
                         {"missing": sc.SENTINEL}),
    "categorical": (lambda: _categorical(False), {}),
    "categorical-deep": (lambda: _categorical(True), {"exact_limit": True}),
    "chain20": (lambda: (_hand_booster([_comb(24, np.arange(20))], 24),
                         sc.rows(5, 65, 24)), {}),
    "softprob": (lambda: (_train(6, n_class=3, rounds=6),
                          _sparse_rows(5, 300, 6)), {}),
    "window2": (_seven_columns, {"window": 2}),
    "window3": (_seven_columns, {"window": 3}),
}


def _assert_within(got, want, bst):
    leaf = max(float(np.abs(t.split_cond[:t.n_nodes][t.left[:t.n_nodes]
                                                     == -1]).max())
               for t in bst.trees)
    bound = (np.spacing(np.abs(want)).astype(np.float64)
             + 2.0 ** -40 * len(bst.trees) * 2 * leaf)
    err = np.abs(got.astype(np.float64) - want)
    print(f"max|err|={err.max():.3e} worst err/bound={(err / bound).max():.3f}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert (err <= bound).all()


@pytest.mark.parametrize("name", list(CASES))
def test_approx_contribs(monkeypatch, name):
    from xgboost_amd import ops, shap
    from xgboost_amd.backend import gpu as gpu_backend
    build, kw = CASES[name]
    bst, rows = build()
    csr = None if isinstance(rows, np.ndarray) else rows
    if "tile" in kw:  # one row past a block's tile
        csr = csr[:ops.load().gbt_shap_saabas_rows() + kw["tile"]]
    X = rows if csr is None else _dense_nan(csr)
    missing = kw.get("missing", np.nan)
    cpu, gpu = _reload(bst, "cpu"), _reload(bst, DEV)
    want = cpu.predict(xgb.DMatrix(X, missing=missing), **APPROX)
    assert np.ptp(want[..., :-1]) > 0
    with sc.host_recursion_raises(monkeypatch, shap) as m:
        if "window" in kw:
            m.setattr(gpu_backend, "_SHAP_APPROX_WINDOW", kw["window"])
        m.setattr(gpu_backend, "_SHAP_CSR_CHUNK_ROWS", 64)
        d = xgb.DMatrix(X, missing=missing)
        got = gpu.predict(d, **APPROX)
        margin = gpu.predict(d, output_margin=True)
        if csr is not None:
            got_csr = gpu.predict(xgb.DMatrix(csr), **APPROX)
        if kw.get("exact_limit"):
            with pytest.raises(AssertionError, match="host SHAP"):
                gpu.predict(d, pred_contribs=True)
    _assert_within(got, want, cpu)
    assert np.allclose(got.sum(axis=-1), margin, rtol=0, atol=1e-3)
    if csr is not None:
        assert np.array_equal(got_csr, got)
        _assert_within(got_csr, want, cpu)


def test_node_means_bit_for_bit():
    """The means kernel against the numpy loop of shap._saabas, on a
    forest with zero-cover internal nodes (the 1e-16 floor) and a stump."""
    from xgboost_amd.backend.gpu import _SaabasForest
    trees = [sc.zero_cover_tree(), _comb(3, [0, 1, 2, 1]), _stump(3)]
    gpu = sc.booster(trees, 3, device=DEV)
    want = []
    for tree in gpu.trees:
        mean_val = np.zeros(tree.n_nodes)
        for nid in range(tree.n_nodes - 1, -1, -1):
            if tree.is_leaf(nid):
                mean_val[nid] = float(tree.split_cond[nid])
            else:
                l, r = int(tree.left[nid]), int(tree.right[nid])
                hl, hr = float(tree.sum_hess[l]), float(tree.sum_hess[r])
                tot = max(hl + hr, 1e-16)
                mean_val[nid] = (mean_val[l] * hl + mean_val[r] * hr) / tot
        want.append(mean_val)
    assert any(float(t.sum_hess[l]) + float(t.sum_hess[r]) == 0.0
               for t in gpu.trees for l, r in zip(t.left[:t.n_nodes],
                                                  t.right[:t.n_nodes])
               if l != -1)
    sf = _SaabasForest(gpu, 0, 3, 3, torch.device(DEV))
    got = sf.mean.cpu().numpy()
    assert np.array_equal(got.view(np.int64),
                          np.concatenate(want).view(np.int64))
