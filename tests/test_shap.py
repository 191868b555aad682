"""SHAP correctness: efficiency axiom (sum of contributions == margin
prediction), interactions consistency (reference analog:
tests/cpp/predictor/test_shap.cc, python test_shap.py)."""
import numpy as np
import pytest

import xgboost_amd as xgb
from conftest import make_classification, make_regression


def _small_model(rounds=3, depth=3, n=150, f=4):
    X, y = make_regression(n, f)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": depth,
                     "eta": 0.5}, d, rounds, verbose_eval=False)
    return bst, d, X, y


def test_shap_sums_to_margin():
    bst, d, X, y = _small_model()
    contribs = bst.predict(d, pred_contribs=True)
    assert contribs.shape == (150, 5)
    margin = bst.predict(d, output_margin=True)
    assert np.allclose(contribs.sum(axis=1), margin, atol=1e-4)


def test_shap_missing_values():
    X, y = make_regression(100, 4)
    X[np.random.RandomState(0).rand(*X.shape) < 0.2] = np.nan
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 3},
                    d, 3, verbose_eval=False)
    contribs = bst.predict(d, pred_contribs=True)
    margin = bst.predict(d, output_margin=True)
    assert np.allclose(contribs.sum(axis=1), margin, atol=1e-4)


def test_shap_unused_feature_zero():
    rng = np.random.RandomState(0)
    X = rng.randn(200, 3).astype(np.float32)
    y = X[:, 0].astype(np.float32)  # only feature 0 matters
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 2,
                     "colsample_bytree": 1.0}, d, 3, verbose_eval=False)
    contribs = bst.predict(d, pred_contribs=True)
    used = set()
    for t in bst.trees:
        for nid in range(t.n_nodes):
            if not t.is_leaf(nid):
                used.add(int(t.split_index[nid]))
    for f in range(3):
        if f not in used:
            assert np.allclose(contribs[:, f], 0.0)


def test_approx_contribs_sum():
    bst, d, X, y = _small_model()
    contribs = bst.predict(d, pred_contribs=True, approx_contribs=True)
    margin = bst.predict(d, output_margin=True)
    assert np.allclose(contribs.sum(axis=1), margin, atol=1e-4)


def test_interactions_sum_to_shap():
    bst, d, X, y = _small_model(rounds=2, depth=3, n=60)
    inter = bst.predict(d, pred_interactions=True)
    assert inter.shape == (60, 5, 5)
    contribs = bst.predict(d, pred_contribs=True)
    # rows of the interaction matrix sum to the SHAP values
    assert np.allclose(inter.sum(axis=2), contribs, atol=1e-3)
    # symmetry
    assert np.allclose(inter, np.transpose(inter, (0, 2, 1)), atol=1e-5)


def test_multiclass_contribs():
    X, y = make_classification(200, 4, n_class=3)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "multi:softprob", "num_class": 3,
                     "max_depth": 3}, d, 2, verbose_eval=False)
    contribs = bst.predict(d, pred_contribs=True)
    assert contribs.shape == (200, 3, 5)
    margin = bst.predict(d, output_margin=True)
    assert np.allclose(contribs.sum(axis=2), margin, atol=1e-4)


def test_path_pair_decomposition_matches_exact_interactions():
    """Python mirror of the shap_ix.hip algorithm (extend once, unwind
    each element b, accumulate conditional pair terms) vs the exact
    conditioned-TreeSHAP CPU implementation — validates the math the
    GPU kernel runs — and both against the Shapley interaction index
    computed from its definition (shap_cases.shapley_interactions)."""
    import shap_cases as sc
    import xgboost_amd as xgb
    from xgboost_amd.shap import shap_interactions, shap_values
    from xgboost_amd.shap_paths import build_path_table, element_agrees

    def extend_pw(zs, ones):
        pw = [1.0]
        for j, (z, o) in enumerate(zip(zs, ones)):
            mm = j + 1
            pw.append(o * pw[mm - 1] * mm / (mm + 1))
            for i in range(mm - 1, 0, -1):
                pw[i] = (o * pw[i - 1] * i / (mm + 1)
                         + z * pw[i] * (mm - i) / (mm + 1))
            pw[0] = z * pw[0] * mm / (mm + 1)
        return pw

    def unwind_pw(pw, z, o, d):
        out = [0.0] * d
        n_ = pw[d]
        if o != 0:
            for j in range(d - 1, -1, -1):
                t = n_ * (d + 1) / ((j + 1) * o)
                out[j] = t
                n_ = pw[j] - t * z * (d - j) / (d + 1)
        else:
            for j in range(d - 1, -1, -1):
                out[j] = pw[j] * (d + 1) / (z * (d - j))
        return out

    def unwound_sum_pw(pw, z, o, d):
        total = 0.0
        n_ = pw[d]
        if o != 0:
            for j in range(d - 1, -1, -1):
                t = n_ * (d + 1) / ((j + 1) * o)
                total += t
                n_ = pw[j] - t * z * (d - j) / (d + 1)
        else:
            for j in range(d - 1, -1, -1):
                total += pw[j] * (d + 1) / (z * (d - j))
        return total

    rng = np.random.RandomState(11)
    n, f = 150, 5
    X = rng.randn(n, f).astype(np.float32)
    X[rng.rand(n, f) < 0.05] = np.nan
    y = (np.nan_to_num(X[:, 0] * X[:, 1] + X[:, 2]) > 0).astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"max_depth": 4, "eta": 0.5,
                     "objective": "binary:logistic"}, d, 4,
                    verbose_eval=False)
    ref = shap_interactions(bst, d).astype(np.float64)

    pp, pg, ef, elo, ehi, emiss, ez, pv, bias = build_path_table(
        bst.trees, bst.tree_info)
    base = shap_values(bst, d).astype(np.float64)
    C = f + 1
    out = np.zeros((n, C, C))
    for p in range(len(pg)):
        s, e = pp[p], pp[p + 1]
        M = e - s
        if M < 2 or pv[p] == 0.0:
            continue
        zs = list(ez[s:e])
        fs = ef[s:e]
        v = pv[p]
        for i in range(n):
            ones = []
            for j in range(M):
                ok = element_agrees(X[i, fs[j]], elo[s + j], ehi[s + j],
                                    emiss[s + j])
                ones.append(1.0 if ok else 0.0)
            pw = extend_pw(zs, ones)
            for b in range(M):
                mult = 0.25 * v * (ones[b] - zs[b])
                if mult == 0.0:
                    continue
                pwb = unwind_pw(pw, zs[b], ones[b], M)
                for a in range(M):
                    if a == b:
                        continue
                    U = unwound_sum_pw(pwb, zs[a], ones[a], M - 1)
                    w = mult * (ones[a] - zs[a]) * U
                    out[i, fs[a], fs[b]] += w
                    out[i, fs[b], fs[a]] += w
    for i_ in range(C):
        out[:, i_, i_] = base[:, i_] - (out[:, i_, :].sum(axis=-1)
                                        - out[:, i_, i_])
    assert np.allclose(out, ref, atol=1e-4), np.abs(out - ref).max()
    want = sc.with_base(
        sc.shapley_interactions(bst.trees, bst.tree_info, X), bst)[:, 0]
    # `out` is fp64 but for its diagonal, completed from the float32
    # contributions: 2^-23 S (k + 1) there, and for `ref`, cast once
    sc.assert_close(out.astype(np.float32), want, bst.trees, cube=True,
                    what="mirror")
    sc.assert_close(ref.astype(np.float32), want, bst.trees, cube=True,
                    what="host")
    off = ~np.eye(C, dtype=bool)
    assert np.abs(out[:, off] - want[:, off]).max() <= 1e-12 * sc.scale(want)


def test_contribs_strict_shape():
    """reference strict_shape: contribs (n, groups, ncol+1),
    interactions (n, groups, ncol+1, ncol+1)."""
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(30, 3).astype(np.float32)
    bst = xgb.train({"max_depth": 2},
                    xgb.DMatrix(X, label=X[:, 0]), 2)
    d = xgb.DMatrix(X)
    assert bst.predict(d, pred_contribs=True,
                       strict_shape=True).shape == (30, 1, 4)
    assert bst.predict(d, pred_interactions=True,
                       strict_shape=True).shape == (30, 1, 4, 4)
