"""Host SHAP against the Shapley definition (tests/shap_cases.py): the
fp64 recursion before its final cast, the public float32 outputs on
dense and CSR input, and the path table that the device kernels read,
evaluated in numpy.  The bounds are those of shap_cases.assert_close:
1e-12 * S for fp64, 2^-23 * S for a float32 cast, exact zeros by ==."""
import functools

import numpy as np
import pytest

import shap_cases as sc
import xgboost_amd as xgb
from xgboost_amd import shap
from xgboost_amd.shap_paths import (_unwound_sum, build_path_table,
                                    element_agrees)
from xgboost_amd.tree_model import RegTree

F = 8           # columns; 6 and 7 are split on by no tree
FEATS = range(6)
CAT = 4         # the categorical column of the categorical forests

CASES = {
    # name: (seed, trees, groups, missing, categorical)
    "nan-1g": (1, 4, 1, np.nan, False),
    "nan-3g": (2, 6, 3, np.nan, False),
    "sentinel-1g": (3, 4, 1, sc.SENTINEL, False),
    "sentinel-3g": (4, 6, 3, sc.SENTINEL, False),
    "cat-1g": (5, 4, 1, np.nan, True),
    "cat-3g": (6, 6, 3, sc.SENTINEL, True),
}


@functools.lru_cache(maxsize=None)
def _case(name, n=40):
    seed, n_trees, g, missing, cat = CASES[name]
    cats = (CAT,) if cat else ()
    trees = sc.random_forest(seed, F, n_trees, 5, FEATS, cats)
    if cat:  # the root of the first tree is categorical for certain
        first = RegTree(F)
        rng = np.random.RandomState(seed)
        l, r = sc._add(first, 0, CAT, 0.0, True, rng, 8.0,
                       cats=np.asarray(sc.CATS))
        sc._add(first, l, 0, 0.25, False, rng, float(first.sum_hess[l]))
        sc._add(first, r, CAT, 0.0, False, rng, float(first.sum_hess[r]),
                cats=np.asarray([0, 33, 45]))
        trees[0] = first
    groups = [i % g for i in range(n_trees)]
    X = sc.rows(seed + 100, n, F, missing, cats)
    sc.assert_edge_values(trees, X, missing)
    assert max(t.max_depth() for t in trees) == 5
    return trees, groups, g, missing, X


@functools.lru_cache(maxsize=None)
def _refs(name):
    trees, groups, g, missing, X = _case(name)
    return (sc.shapley(trees, groups, X, missing, g),
            sc.shapley_interactions(trees, groups, X, missing, g))


# -- 1. the fp64 recursion before its cast ----------------------------------

@functools.lru_cache(maxsize=None)
def _host_phi(name):
    trees, groups, g, missing, X = _case(name)
    phi = np.zeros((X.shape[0], g, F + 1))
    shap._host_contribs(trees, groups, X, phi, missing, False)
    return phi


@pytest.mark.parametrize("name", CASES)
def test_host_contribs_fp64(name):
    trees = _case(name)[0]
    ref = _refs(name)[0]
    assert sc.scale(ref) > 0.3
    sc.assert_close(_host_phi(name), ref, trees, what=name)


@pytest.mark.parametrize("name", CASES)
def test_host_interactions_fp64(name):
    trees, groups, g, missing, X = _case(name)
    ref = _refs(name)[1]
    n = 12  # 2 |N| conditioned recursions per (tree, row)
    got = shap._host_interactions(trees, groups, X[:n], _host_phi(name)[:n],
                                  missing)
    off = ref[:n][..., ~np.eye(F + 1, dtype=bool)]
    assert np.abs(off).max() > 0.01  # there are interactions to get wrong
    sc.assert_close(got, ref[:n], trees, cube=True, what=name)


def test_interaction_reference_is_consistent():
    """Rows of the reference cube sum to the reference contributions and
    the cube is symmetric: the two definitions agree with each other."""
    phi, cube = _refs("nan-3g")
    assert np.abs(cube.sum(axis=-1) - phi).max() <= 1e-14 * sc.scale(phi)
    assert np.array_equal(cube, np.swapaxes(cube, -1, -2))


# -- 2. the public outputs ---------------------------------------------------

def _public(name, mode, sparse, it_range=None, n=None):
    trees, groups, g, missing, X = _case(name)
    X = X[:n]
    bst = sc.booster(trees, F, g)
    if sparse:
        assert np.isnan(missing)
        d = xgb.DMatrix(sc.to_csr(X))
    else:
        d = xgb.DMatrix(X, missing=missing)
    kw = {} if it_range is None else {"iteration_range": it_range}
    got = bst.predict(d, strict_shape=True, **mode, **kw)
    lo, hi = (0, len(trees) // g) if it_range is None else it_range
    sub = trees[lo * g:hi * g]
    fn = (sc.shapley_interactions if "pred_interactions" in mode
          else sc.shapley)
    ref = sc.with_base(fn(sub, groups[lo * g:hi * g], X, missing, g), bst)
    return got, ref, sub


# a CSR matrix has no numeric missing value: absent or NaN is missing
@pytest.mark.parametrize("name,sparse", [
    (name, sparse) for name in CASES for sparse in (False, True)
    if not sparse or np.isnan(CASES[name][3])],
    ids=lambda v: v if isinstance(v, str) else ("csr" if v else "dense"))
def test_pred_contribs(name, sparse):
    got, ref, trees = _public(name, {"pred_contribs": True}, sparse)
    assert got.dtype == np.float32
    sc.assert_close(got, ref, trees, what=name)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("name", ["nan-1g", "nan-3g", "cat-1g"])
def test_pred_interactions(name, sparse):
    got, ref, trees = _public(name, {"pred_interactions": True}, sparse,
                              n=10)
    assert got.dtype == np.float32
    sc.assert_close(got, ref, trees, cube=True, what=name)


def test_pred_interactions_numeric_missing():
    got, ref, trees = _public("sentinel-3g", {"pred_interactions": True},
                              False, n=10)
    sc.assert_close(got, ref, trees, cube=True, what="sentinel-3g")


@pytest.mark.parametrize("mode", [{"pred_contribs": True},
                                  {"pred_interactions": True}],
                         ids=lambda m: "-".join(m))
@pytest.mark.parametrize("name,it_range", [("nan-1g", (1, 3)),
                                           ("nan-3g", (1, 2)),
                                           ("nan-1g", (3, 4))])
def test_iteration_range(name, it_range, mode):
    for sparse in (False, True):
        got, ref, trees = _public(name, mode, sparse, it_range, n=10)
        assert len(trees) == (it_range[1] - it_range[0]) * CASES[name][2]
        sc.assert_close(got, ref, trees, cube="pred_interactions" in mode,
                        what=f"{name}{it_range}")


def test_unused_features_are_exactly_zero():
    trees, groups, g, missing, X = _case("nan-3g")
    assert set(sc.used_features(trees)) == set(FEATS)
    bst = sc.booster(trees, F, g)
    for d in (xgb.DMatrix(X), xgb.DMatrix(sc.to_csr(X))):
        phi = bst.predict(d, pred_contribs=True)
        assert phi[..., :6].any(axis=(0, 1)).all()
        assert (phi[..., 6:8] == 0.0).all()
        cube = bst.predict(xgb.DMatrix(X[:6]), pred_interactions=True)
        assert (cube[..., 6:8, :] == 0.0).all()
        assert (cube[..., :, 6:8] == 0.0).all()
        assert (cube[..., :8, 8] == 0.0).all()
        assert (cube[..., 8, :8] == 0.0).all()


# -- 3. the path table, evaluated in numpy ------------------------------------

def _table_contribs(trees, groups, g, X, missing):
    """What the path kernels compute from build_path_table, in fp64."""
    pp, pg, ef, elo, ehi, emiss, ez, pv, bias = build_path_table(trees,
                                                                 groups)
    n, f = X.shape
    out = np.zeros((n, g, f + 1))
    out[:, :len(bias), f] = bias
    for p in range(len(pg)):
        s, e = int(pp[p]), int(pp[p + 1])
        zs = [float(z) for z in ez[s:e]]
        for r in range(n):
            ones = [1.0 if element_agrees(X[r, ef[j]], elo[j], ehi[j],
                                          emiss[j], missing) else 0.0
                    for j in range(s, e)]
            for i in range(e - s):
                if ones[i] == zs[i]:
                    continue  # (one - zero) = 0; the kernels hold rz = 0
                out[r, pg[p], ef[s + i]] += (
                    pv[p] * (ones[i] - zs[i]) * _unwound_sum(zs, ones, i))
    return out


def _builder_tree():
    """f0 three times on one path; an f1 interval [1.0, 0.25) that only
    a missing value reaches (default right, then default left); f1 with
    opposite defaults where a missing value cannot follow."""
    rng = np.random.RandomState(7)
    t = RegTree(3)
    h = lambda nid: float(t.sum_hess[nid])  # noqa: E731
    l, r = sc._add(t, 0, 0, 1.0, True, rng, 9.0)
    _, lr = sc._add(t, l, 0, -0.5, False, rng, h(l))
    lrl, _ = sc._add(t, lr, 0, 0.25, True, rng, h(lr))
    sc._add(t, lrl, 1, 0.0, False, rng, h(lrl))
    rl, rr = sc._add(t, r, 1, 1.0, False, rng, h(r))
    rrl, _ = sc._add(t, rr, 1, 0.25, True, rng, h(rr))
    sc._add(t, rrl, 2, 0.0, True, rng, h(rrl))
    rll, _ = sc._add(t, rl, 1, 2.5, True, rng, h(rl))
    sc._add(t, rll, 2, 0.25, False, rng, h(rll))
    return t


@pytest.mark.parametrize("missing", [np.nan, sc.SENTINEL],
                         ids=["nan", "sentinel"])
def test_path_table_matches_definition(missing):
    trees = [_builder_tree()] + sc.random_forest(11, 3, 3, 5)
    groups = [0, 1, 0, 1]
    X = sc.rows(12, 60, 3, missing)
    sc.assert_edge_values(trees, X, missing)
    pp, _, ef, elo, ehi, emiss = build_path_table(trees[:1], [0])[:6]
    assert ((elo >= ehi) & (emiss == 1)).any()   # empty, missing reaches it
    assert ((elo >= ehi) & (emiss == 0)).any()   # empty and unreachable
    assert np.diff(pp).max() == 3
    ref = sc.shapley(trees, groups, X, missing, 2)
    sc.assert_close(_table_contribs(trees, groups, 2, X, missing), ref,
                    trees, what="table")
    # the host recursion walks the same forest
    phi = np.zeros_like(ref)
    shap._host_contribs(trees, groups, X, phi, missing, False)
    sc.assert_close(phi, ref, trees, what="host")


# -- 4. a child without cover -----------------------------------------------------

def test_zero_cover_children():
    """A branch whose cover is zero has weight 0 in the definition; no
    route may raise or return NaN, and every row is compared."""
    trees, groups = [sc.zero_cover_tree(), sc.random_forest(3, 3, 1, 3)[0]], \
        [0, 0]
    X = sc.zero_cover_rows()
    t = trees[0]
    leaves = t.predict_leaf_np(X)
    assert set(leaves) == set(np.nonzero(t.left[:t.n_nodes] == -1)[0])
    assert (t.sum_hess[leaves] == 0).any()
    ref = sc.shapley(trees, groups, X)
    cube = sc.shapley_interactions(trees, groups, X)
    sc.assert_close(_table_contribs(trees, groups, 1, X, np.nan), ref, trees,
                    what="table")
    phi = np.zeros_like(ref)
    shap._host_contribs(trees, groups, X, phi, np.nan, False)
    sc.assert_close(phi, ref, trees, what="host fp64")
    sc.assert_close(shap._host_interactions(trees, groups, X, phi, np.nan),
                    cube, trees, cube=True, what="host fp64 interactions")
    bst = sc.booster(trees, 3)
    for d in (xgb.DMatrix(X), xgb.DMatrix(sc.to_csr(X))):
        got = bst.predict(d, pred_contribs=True, strict_shape=True)
        sc.assert_close(got, sc.with_base(ref, bst), trees, what="public")
        got = bst.predict(d, pred_interactions=True, strict_shape=True)
        sc.assert_close(got, sc.with_base(cube, bst), trees, cube=True,
                        what="public interactions")
