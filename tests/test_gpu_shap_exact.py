"""The SHAP kernels against the Shapley definition (tests/shap_cases.py).
Each kernel is launched directly: ShapPathsKernel<8> and <16>
(shap_paths.hip), ShapIxKernel (shap_ix.hip) and the DFS kernel
(shap.hip); then the public device routes, with the host recursion made
to raise.  Every case draws its rows from the threshold grid and asserts
that values on a threshold, next to it, +-inf, NaN and the sentinel occur
in split features.  fp64 results are held to 1e-12 * S, float32 casts to
2^-23 * S; the DFS kernel, which keeps its frame fractions and its output
in float32, to DFS_BOUND (profiles/r07_shap_exact.md)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import shap_cases as sc
import xgboost_amd as xgb
from xgboost_amd import shap

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 4 x the largest |got - reference| / S measured on an MI355X over the
# DFS cases of this file: 6.323e-8 at k8-1g (6 trees, depth 8, S = 2.404)
DFS_BOUND = 4 * 6.323e-8


def _gpu():
    from xgboost_amd.backend import gpu
    return gpu


def _forest(name):
    """(trees, F) of a named forest."""
    if name == "zero":
        return [sc.zero_cover_tree(10), sc.random_forest(3, 10, 1, 3,
                                                         range(3))[0],
                sc.zero_cover_tree(10)], 10
    if name == "cat":
        trees = sc.random_forest(21, 10, 6, 5, range(7), cat_feats=(4,))
        rng = np.random.RandomState(21)
        first = sc.RegTree(10)
        l, r = sc._add(first, 0, 4, 0.0, True, rng, 8.0,
                       cats=np.asarray(sc.CATS))
        sc._add(first, l, 0, 0.25, False, rng, float(first.sum_hess[l]))
        sc._add(first, r, 4, 0.0, False, rng, float(first.sum_hess[r]),
                cats=np.asarray([0, 33, 45]))
        trees[0] = first
        return trees, 10
    if name == "comb16":
        rng = np.random.RandomState(40)
        return [sc.comb(rng, 18, list(range(16)))], 18
    if name == "wide128":
        return sc.random_forest(31, 128, 3, 5, [0, 5, 64, 126, 127]), 128
    k = int(name[1:])  # "k8": the longest path has 8 distinct features
    F = max(10, k + 2)
    return sc.random_forest(50 + k, F, 6, min(k, 5), range(F - 2),
                            longest=k), F


CASES = {
    # name: (forest, groups, rows, missing)
    "k1": ("k1", 3, 300, np.nan),
    "k2": ("k2", 3, 300, sc.SENTINEL),
    "k7": ("k7", 3, 300, np.nan),
    "k8": ("k8", 3, 300, sc.SENTINEL),
    "k8-1g": ("k8", 1, 300, np.nan),
    "k9": ("k9", 3, 300, np.nan),
    "k9-1g": ("k9", 1, 300, sc.SENTINEL),
    "comb16": ("comb16", 1, 8, np.nan),
    "zero": ("zero", 3, 64, np.nan),
    "cat": ("cat", 3, 300, sc.SENTINEL),
    "wide128": ("wide128", 3, 300, np.nan),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    fname, g, n, missing = CASES[name]
    trees, F = _forest(fname)
    groups = [i % g for i in range(len(trees))]
    if fname == "zero":
        X = np.zeros((n, F), np.float32)
        X[:, :3] = sc.zero_cover_rows()
        leaves = trees[0].predict_leaf_np(X)
        assert (trees[0].sum_hess[leaves] == 0).any()
    else:
        cats = (4,) if fname == "cat" else ()
        X = sc.rows(40 if fname == "comb16" else 7, n, F, missing, cats)
        sc.assert_edge_values(trees, X, missing)
    return trees, groups, g, missing, X, F


@functools.lru_cache(maxsize=None)
def _ref(name):
    trees, groups, g, missing, X, F = _case(name)
    return sc.shapley(trees, groups, X, missing, g)


@functools.lru_cache(maxsize=None)
def _ref_cube(name):
    trees, groups, g, missing, X, F = _case(name)
    return sc.shapley_interactions(trees, groups, X, missing, g)


def _longest(name):
    from xgboost_amd.shap_paths import build_path_table
    trees, groups = _case(name)[:2]
    return int(np.diff(build_path_table(trees, groups)[0]).max())


def _model(trees, groups):
    return SimpleNamespace(trees=trees, tree_info=groups)


def _paths(name, entry=None):
    """fp64 [n, g, C] device tensor from the path kernel: the one the
    dispatcher picks, or the `entry` point named."""
    from xgboost_amd import ops as hip_ops
    gpu = _gpu()
    trees, groups, g, missing, X, F = _case(name)
    dev = torch.device(DEV)
    tab = gpu._PathTable(_model(trees, groups), 0, len(trees), dev)
    assert int(tab.t["ef"].max()) < F and int(tab.t["pg"].max()) < g
    n = X.shape[0]
    Xt = torch.from_numpy(X).to(dev).t().contiguous()
    out = torch.zeros((g, F + 1, n), dtype=torch.float64, device=dev)
    for grp in range(len(tab.bias)):
        out[grp, F] = float(tab.bias[grp])
    if entry is None:
        gpu._launch_shap_paths(tab, Xt, n, F, missing, g, F + 1, out)
    else:
        getattr(hip_ops.load(), entry)(
            hip_ops.ptr(Xt), n, F, *gpu._missing_args(missing), *tab.args(),
            g, F + 1, hip_ops.ptr(out), hip_ops.stream())
    return out.permute(2, 0, 1), tab, Xt


# -- 1. gbt_shap_paths, kD = 8 ----------------------------------------------

@pytest.mark.parametrize("name,k", [("k1", 1), ("k2", 2), ("k7", 7),
                                    ("k8", 8), ("k8-1g", 8), ("zero", 3)])
def test_paths8(name, k):
    assert _longest(name) == k
    trees = _case(name)[0]
    got = _paths(name, "gbt_shap_paths")[0].cpu().numpy()
    sc.assert_close(got, _ref(name), trees, what=name)


def test_dispatch_boundary(monkeypatch):
    """8 elements go to gbt_shap_paths, 9 to gbt_shap_paths16."""
    from xgboost_amd import ops as hip_ops
    lib = hip_ops.load()
    seen = []

    def spy(entry):
        fn = getattr(lib, entry)

        def call(*args):
            seen.append(entry)
            return fn(*args)
        return call

    for entry in ("gbt_shap_paths", "gbt_shap_paths16"):
        monkeypatch.setattr(lib, entry, spy(entry))
    for name in ("k8", "k9"):
        got = _paths(name)[0].cpu().numpy()
        sc.assert_close(got, _ref(name), _case(name)[0], what=name)
    assert seen == ["gbt_shap_paths", "gbt_shap_paths16"]


# -- 2. gbt_shap_paths16 -----------------------------------------------------

@pytest.mark.parametrize("name,k", [("k1", 1), ("k2", 2), ("k7", 7),
                                    ("k8", 8), ("k9", 9), ("k9-1g", 9),
                                    ("comb16", 16), ("zero", 3)])
def test_paths16(name, k):
    assert _longest(name) == k
    trees = _case(name)[0]
    got = _paths(name, "gbt_shap_paths16")[0].cpu().numpy()
    sc.assert_close(got, _ref(name), trees, what=name)


# -- 3. gbt_shap_ix ------------------------------------------------------------

@pytest.mark.parametrize("name,k", [("k1", 1), ("k2", 2), ("k8", 8),
                                    ("k8-1g", 8), ("k9", 9), ("k9-1g", 9),
                                    ("comb16", 16), ("zero", 3)])
def test_ix(name, k):
    gpu = _gpu()
    assert _longest(name) == k
    trees, groups, g, missing, X, F = _case(name)
    base, tab, Xt = _paths(name)
    n, C = X.shape[0], F + 1
    cube = torch.zeros((g, C, C, n), dtype=torch.float64, device=DEV)
    gpu._launch_shap_ix(tab, Xt, n, F, missing, g, C, cube)
    if k == 1:  # no pair on any path: the kernel skips them all
        assert not cube.any()
    else:
        assert cube.any()
    got = gpu._complete_diagonal(cube, base).cpu().numpy()
    sc.assert_close(got, _ref_cube(name), trees, cube=True, what=name)


# -- 4. gbt_shap, the DFS kernel ------------------------------------------------

def _dfs(name):
    gpu = _gpu()
    trees, groups, g, missing, X, F = _case(name)
    dev = torch.device(DEV)
    assert F + 1 <= 129 and max(t.max_depth() for t in trees) <= 16
    fa = gpu._ForestArrays(_model(trees, groups), 0, len(trees), dev)
    expected = torch.tensor([shap._expected_value(t) for t in trees],
                            dtype=torch.float64, device=dev)
    n = X.shape[0]
    out = torch.zeros((n, g, F + 1), dtype=torch.float32, device=dev)
    gpu._launch_shap_dfs(fa, torch.from_numpy(X).to(dev), n, F, missing,
                         expected, g, F + 1, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["k2", "k8", "k8-1g", "k9", "comb16",
                                  "zero", "cat", "wide128"])
def test_dfs(name):
    trees, _, _, _, X, F = _case(name)
    if name == "comb16":
        assert trees[0].max_depth() == 16
    if name == "wide128":  # the local phi array is exactly full
        assert F + 1 == 129 and 127 in sc.used_features(trees)
    if name == "cat":
        assert any(t.split_type[:t.n_nodes].any() for t in trees)
    ref = _ref(name)
    got = _dfs(name)
    worst = max(t.max_depth() for t in trees)
    print(f"DFS_MEASURE {name} S={sc.scale(ref):.4g} depth={worst} "
          f"trees={len(trees)} "
          f"rel={np.abs(got - ref).max() / sc.scale(ref):.3e}")
    sc.assert_close(got, ref, trees, what=name, rel_bound=DFS_BOUND)


def test_dfs_refuses_130_columns():
    gpu = _gpu()
    F = 129
    trees = sc.random_forest(21, F, 2, 3, [0, 4, 128], cat_feats=(4,))
    trees[0] = sc.RegTree(F)
    sc._add(trees[0], 0, 4, 0.0, True, np.random.RandomState(0), 8.0,
            cats=np.asarray(sc.CATS))
    bst = sc.booster(trees, F, device=DEV)
    X = sc.rows(3, 5, F, cat_feats=(4,))
    phi = np.zeros((5, 1, F + 1))
    with pytest.raises(gpu.ShapDeviceLimit):
        gpu.shap_gpu(bst, xgb.DMatrix(X), 0, 2, phi)


# -- 5. the grid-stride loop ------------------------------------------------------

def test_grid_stride_second_trip():
    """16384 blocks of 256 rows and 300 more: only the second trip of
    the kernels' loop reaches the last 300 rows."""
    gpu = _gpu()
    dev = torch.device(DEV)
    n, F, C = 16384 * 256 + 300, 2, 3
    rng = np.random.RandomState(61)
    cond = np.array([0.25, 1.0], np.float32)  # one threshold per feature
    a, b = sc.RegTree(F), sc.RegTree(F)
    l, r = sc._add(a, 0, 0, cond[0], True, rng, 9.0)
    sc._add(a, l, 1, cond[1], False, rng, float(a.sum_hess[l]))
    sc._add(a, r, 1, cond[1], True, rng, float(a.sum_hess[r]))
    _, r = sc._add(b, 0, 1, cond[1], False, rng, 5.0)
    sc._add(b, r, 0, cond[0], True, rng, float(b.sum_hess[r]))
    trees, groups = [a, b], [0, 0]
    # the 6-value grid of a column: on its threshold, the float32 next to
    # it on either side, +-inf and NaN
    vals = np.stack([cond, np.nextafter(cond, np.float32(-np.inf)),
                     np.nextafter(cond, np.float32(np.inf)),
                     np.full(2, np.inf, np.float32),
                     np.full(2, -np.inf, np.float32),
                     np.full(2, np.nan, np.float32)])
    Xu = np.array([[vals[i, 0], vals[j, 1]] for i in range(6)
                   for j in range(6)], np.float32)
    sc.assert_edge_values(trees, Xu)
    ref = torch.from_numpy(sc.shapley(trees, groups, Xu)).to(dev)
    cube_ref = sc.shapley_interactions(trees, groups, Xu)
    S, S2 = sc.scale(ref.cpu().numpy()), sc.scale(cube_ref)
    cube_ref = torch.from_numpy(cube_ref).to(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    codes = torch.randint(len(Xu), (n,), device=dev, generator=gen)
    codes[-300:] = torch.arange(300, device=dev) % len(Xu)  # every row kind
    Xt = torch.from_numpy(Xu).to(dev).t()[:, codes].contiguous()
    tab = gpu._PathTable(_model(trees, groups), 0, 2, dev)
    assert tab.max_elems == 2

    def worst(got, want):  # one number back from the device, twice
        diff = (got - want[codes]).abs()
        return float(diff.max()), float(diff[-300:].max())

    out = torch.zeros((1, C, n), dtype=torch.float64, device=dev)
    out[0, F] = float(tab.bias[0])
    gpu._launch_shap_paths(tab, Xt, n, F, np.nan, 1, C, out)
    for c in range(C):
        every, tail = worst(out[0, c], ref[:, 0, c])
        assert every <= 1e-12 * S and tail <= 1e-12 * S, (c, every, tail)
    assert float(out[0, :2, -300:].abs().max()) > 0.01
    del out
    cube = torch.zeros((1, C, C, n), dtype=torch.float64, device=dev)
    gpu._launch_shap_ix(tab, Xt, n, F, np.nan, 1, C, cube)
    for a in range(C):
        for b in range(C):
            want = cube_ref[:, 0, a, b] if a != b else cube_ref[:, 0, a, b] * 0
            every, tail = worst(cube[0, a, b], want)
            assert every <= 1e-12 * S2 and tail <= 1e-12 * S2, \
                (a, b, every, tail)
    assert float(cube[0, 0, 1, -300:].abs().max()) > 0.001


# -- 6. the public device routes ----------------------------------------------------

def _predict_device(name, mode, sparse):
    trees, groups, g, missing, X, F = _case(name)
    bst = sc.booster(trees, F, g, device=DEV)
    d = (xgb.DMatrix(sc.to_csr(X)) if sparse
         else xgb.DMatrix(X, missing=missing))
    ref_fn = (sc.shapley_interactions if "pred_interactions" in mode
              else sc.shapley)
    # a CSR matrix has no numeric missing value: absent or NaN is missing
    ref = ref_fn(trees, groups, X, np.nan if sparse else missing, g)
    return bst, d, sc.with_base(ref, bst), trees


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("name", ["k8", "k8-1g", "k9", "zero"])
def test_public_contribs(monkeypatch, name, sparse):
    bst, d, ref, trees = _predict_device(name, {"pred_contribs": True},
                                         sparse)
    with sc.host_recursion_raises(monkeypatch, shap):
        got = bst.predict(d, pred_contribs=True, strict_shape=True)
    # dense numeric forests return the path kernel's float64
    assert got.dtype == (np.float32 if sparse else np.float64)
    sc.assert_close(got, ref, trees, what=name)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("name", ["k8", "k8-1g", "k9", "zero"])
def test_public_interactions(monkeypatch, name, sparse):
    bst, d, ref, trees = _predict_device(name, {"pred_interactions": True},
                                         sparse)
    with sc.host_recursion_raises(monkeypatch, shap):
        got = bst.predict(d, pred_interactions=True, strict_shape=True)
    assert got.dtype == np.float32
    sc.assert_close(got, ref, trees, cube=True, what=name)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_public_contribs_categorical(monkeypatch, sparse):
    bst, d, ref, trees = _predict_device("cat", {"pred_contribs": True},
                                         sparse)
    with sc.host_recursion_raises(monkeypatch, shap):
        got = bst.predict(d, pred_contribs=True, strict_shape=True)
    assert got.dtype == np.float32
    sc.assert_close(got, ref, trees, what="cat", rel_bound=DFS_BOUND)


def test_bug_in_dense_device_code_is_not_swallowed(monkeypatch):
    """An AttributeError from inside the device code is a bug, not a
    limit: the dense routes must not answer it with the host recursion."""
    gpu = _gpu()
    trees, groups, g, missing, X, F = _case("k8")
    bst = sc.booster(trees, F, g, device=DEV)

    def broken(self):
        raise AttributeError("a bug, not a limit")

    def limit(self):
        raise gpu.ShapDeviceLimit("a limit")

    modes = ({"pred_contribs": True}, {"pred_interactions": True})
    with monkeypatch.context() as m:
        m.setattr(gpu._PathTable, "args", broken)
        for mode in modes:
            with pytest.raises(AttributeError, match="a bug"):
                bst.predict(xgb.DMatrix(X, missing=missing), **mode)
    # a limit does go to the host, and there the guard of the dense
    # device tests fires: none of them passes on the host recursion
    monkeypatch.setattr(gpu._PathTable, "args", limit)
    for mode in modes:
        with sc.host_recursion_raises(monkeypatch, shap), \
                pytest.raises(AssertionError, match="host SHAP recursion"):
            bst.predict(xgb.DMatrix(X[:3], missing=missing), **mode)
