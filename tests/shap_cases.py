"""The Shapley definition as a brute-force fp64 reference, with seeded
forests and rows for the SHAP tests (test_shap_exact.py for the host
paths, test_gpu_shap_exact.py for the HIP kernels).

Nothing here comes from the TreeSHAP code under test: the node decision,
the cover-weighted expectation and the subset sums are written out from
the definition.  Per tree, with N the features it splits on:

  v(S)    at a node that splits on f in S follow the row, otherwise
          average the children by sum_hess[child] / sum_hess[node]
          (weight 0 where the node's cover is 0)
  phi_i   = sum over S in N\\{i} of |S|! (|N|-|S|-1)! / |N|!
            * (v(S+i) - v(S));  the bias column is v({})
  Phi_ij  = sum over S in N\\{i,j} of |S|! (|N|-|S|-2)! / (2 (|N|-1)!)
            * (v(S+ij) - v(S+i) - v(S+j) + v(S)),  i != j
  Phi_ii  = phi_i - sum_{j != i} Phi_ij

v is held for all 2^|N| subsets at once, one array per node, and
computed once per distinct pattern of node decisions."""
import contextlib
from math import factorial

import numpy as np
import scipy.sparse as sp

import xgboost_amd as xgb
from xgboost_amd.tree_model import RegTree

# every threshold comes from this grid and so do most row values
GRID = np.array([-1.5, -0.5, 0.0, 0.25, 1.0, 2.5], np.float32)
SENTINEL = -999.0                 # the non-NaN missing value
CATS = (1, 5, 33, 40)             # crosses the first 32-bit word
CAT_VALUES = np.array([0, 1, 5, 12, 33, 40, 45, 64, -1], np.float32)


# -- the definition -----------------------------------------------------------

def goes_right(tree, nid, x, missing):
    """bool [n]: the rows whose values `x` of the node's feature go to
    the right child.  Missing goes to the default child, a category in
    the set goes right, x < cond goes left."""
    x = np.asarray(x, np.float32)
    miss = np.isnan(x)
    if not np.isnan(missing):
        miss |= x == np.float32(missing)
    if tree.split_type[nid] == 1:
        cats = np.asarray(tree.cat_segments.get(nid, ()), np.int64)
        safe = np.where(np.isfinite(x), x, -1.0)
        right = np.isin(np.trunc(safe).astype(np.int64), cats[cats >= 0])
    else:
        right = ~(x < np.float32(tree.split_cond[nid]))
    return np.where(miss, not tree.default_left[nid], right)


def split_features(tree):
    n = tree.n_nodes
    return np.unique(tree.split_index[:n][tree.left[:n] != -1]).astype(int)


def subset_values(tree, right, feats):
    """v(S) for all subsets of `feats`, fp64 [2^m]: bit b of the index
    says whether feats[b] is in S.  `right` [n_nodes] bool is the row's
    decision at every internal node."""
    bit = {int(f): b for b, f in enumerate(feats)}
    masks = np.arange(1 << len(feats))
    v = [None] * tree.n_nodes
    for nid in range(tree.n_nodes - 1, -1, -1):  # children follow parents
        l, r = int(tree.left[nid]), int(tree.right[nid])
        if l == -1:
            v[nid] = np.full(len(masks), float(tree.split_cond[nid]))
            continue
        h = float(tree.sum_hess[nid])
        wl = float(tree.sum_hess[l]) / h if h > 0 else 0.0
        wr = float(tree.sum_hess[r]) / h if h > 0 else 0.0
        in_s = (masks >> bit[int(tree.split_index[nid])]) & 1
        v[nid] = np.where(in_s == 1, v[r] if right[nid] else v[l],
                          wl * v[l] + wr * v[r])
        v[l] = v[r] = None
    return v[0]


def _popcount(m):
    masks = np.arange(1 << m)
    return sum((masks >> b) & 1 for b in range(m)) if m else masks * 0


def _phi(v, m):
    """Shapley values [m] of the game v [2^m]."""
    pc = _popcount(m)
    w = np.array([factorial(s) * factorial(m - s - 1) / factorial(m)
                  for s in range(m)])
    masks = np.arange(1 << m)
    out = np.zeros(m)
    for i in range(m):
        s = masks[(masks >> i) & 1 == 0]
        out[i] = np.sum(w[pc[s]] * (v[s | (1 << i)] - v[s]))
    return out


def _pair(v, m):
    """Shapley interaction index [m, m] of the game v, diagonal 0."""
    out = np.zeros((m, m))
    if m < 2:
        return out
    pc = _popcount(m)
    w = np.array([factorial(s) * factorial(m - s - 2)
                  / (2 * factorial(m - 1)) for s in range(m - 1)])
    masks = np.arange(1 << m)
    for i in range(m):
        for j in range(i + 1, m):
            s = masks[((masks >> i) & 1 == 0) & ((masks >> j) & 1 == 0)]
            bi, bj = 1 << i, 1 << j
            out[i, j] = out[j, i] = np.sum(
                w[pc[s]] * (v[s | bi | bj] - v[s | bi] - v[s | bj] + v[s]))
    return out


def _per_tree(tree, X, missing, want_pairs):
    """(feats, phi [n, m], bias [n], pairs [n, m, m] or None) of one
    tree, computed once per distinct decision pattern."""
    feats = split_features(tree)
    m, n = len(feats), X.shape[0]
    internal = np.nonzero(tree.left[:tree.n_nodes] != -1)[0]
    right = np.zeros((n, tree.n_nodes), bool)
    for nid in internal:
        right[:, nid] = goes_right(tree, nid, X[:, tree.split_index[nid]],
                                   missing)
    pats, inv = np.unique(right, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    phi = np.zeros((len(pats), m))
    bias = np.zeros(len(pats))
    pairs = np.zeros((len(pats), m, m)) if want_pairs else None
    for p, pat in enumerate(pats):
        v = subset_values(tree, pat, feats)
        phi[p], bias[p] = _phi(v, m), v[0]
        if want_pairs:
            pairs[p] = _pair(v, m)
    return feats, phi[inv], bias[inv], (pairs[inv] if want_pairs else None)


def shapley(trees, groups, X, missing=np.nan, n_groups=None):
    """fp64 [n, groups, F + 1]: per-group Shapley values of the forest,
    the bias column the sum of the trees' v({})."""
    X = np.asarray(X, np.float32)
    n, F = X.shape
    g = (max(groups, default=-1) + 1) if n_groups is None else n_groups
    out = np.zeros((n, g, F + 1))
    for tree, k in zip(trees, groups):
        feats, phi, bias, _ = _per_tree(tree, X, missing, False)
        out[:, k, feats] += phi
        out[:, k, F] += bias
    return out


def shapley_interactions(trees, groups, X, missing=np.nan, n_groups=None):
    """fp64 [n, groups, F + 1, F + 1]; the bias row and column are zero
    but for the corner, which holds the bias."""
    X = np.asarray(X, np.float32)
    n, F = X.shape
    g = (max(groups, default=-1) + 1) if n_groups is None else n_groups
    out = np.zeros((n, g, F + 1, F + 1))
    for tree, k in zip(trees, groups):
        feats, phi, bias, pairs = _per_tree(tree, X, missing, True)
        m = len(feats)
        pairs[:, np.arange(m), np.arange(m)] = phi - pairs.sum(axis=2)
        out[:, k, feats[:, None], feats[None, :]] += pairs
        out[:, k, F, F] += bias
    return out


def distinct_rows(X):
    """(Xu, inverse): the bitwise-distinct rows and, per row, its index
    into them, so a reference is computed for Xu alone and broadcast."""
    X = np.ascontiguousarray(X, np.float32)
    _, first, inv = np.unique(X.view(np.int32), axis=0, return_index=True,
                              return_inverse=True)
    return X[first], np.asarray(inv).reshape(-1)


# -- forests -------------------------------------------------------------------

def _add(tree, nid, f, cond, default_left, rng, h, cats=None, frac=None):
    """Split nid with an uneven, non-dyadic cover and fresh leaf values."""
    frac = rng.uniform(0.15, 0.85) if frac is None else frac
    lh = np.float32(h * frac)
    rh = np.float32(h * (1.0 - frac))
    lw, rw = rng.uniform(-1.0, 1.0, 2)
    return tree.add_split(nid, int(f), float(cond), bool(default_left), 1.0,
                          0.0, lw, rw, h, float(lh), float(rh),
                          categories_go_right=cats)


def _cat_set(rng):
    """A category set with members on both sides of bit 32."""
    low = rng.choice([0, 1, 5, 12], 2, replace=False)
    high = rng.choice([33, 40, 45], rng.randint(1, 3), replace=False)
    return np.concatenate([low, high])


def random_tree(rng, F, feats, max_depth, cat_feats=(), p_split=0.75,
                p_repeat=0.35):
    """A tree over `feats` no deeper than max_depth: thresholds from
    GRID, either default direction, a feature repeated on a path with
    probability p_repeat, category sets on `cat_feats`."""
    tree = RegTree(F)
    todo = [(0, 0, (), float(np.float32(rng.uniform(2.0, 12.0))))]
    while todo:
        nid, depth, on_path, h = todo.pop()
        if depth == max_depth or (depth and rng.rand() > p_split):
            continue
        if on_path and rng.rand() < p_repeat:
            f = on_path[rng.randint(len(on_path))]
        else:
            f = feats[rng.randint(len(feats))]
        cats = _cat_set(rng) if f in cat_feats else None
        l, r = _add(tree, nid, f, GRID[rng.randint(len(GRID))],
                    rng.rand() < 0.5, rng, h, cats)
        for c in (l, r):
            todo.append((c, depth + 1, on_path + (f,),
                         float(tree.sum_hess[c])))
    return tree


def comb(rng, F, feats):
    """One feature per level, so the deepest path holds len(feats)
    distinct features; the side the comb continues on alternates."""
    tree = RegTree(F)
    nid, h = 0, float(np.float32(rng.uniform(4.0, 12.0)))
    for i, f in enumerate(feats):
        l, r = _add(tree, nid, f, GRID[rng.randint(len(GRID))], i % 3 == 0,
                    rng, h, frac=rng.uniform(0.35, 0.65))
        nid = l if i % 2 else r
        h = float(tree.sum_hess[nid])
    return tree


def random_forest(seed, F, n_trees, max_depth, feats=None, cat_feats=(),
                  longest=None):
    """Seeded forest over `feats` (default: all F).  With `longest` = k
    the first tree is a comb over the first k of them and the others use
    only those k, so the longest path has exactly k distinct features."""
    rng = np.random.RandomState(seed)
    feats = list(range(F)) if feats is None else [int(f) for f in feats]
    trees = []
    if longest is not None:
        feats = feats[:longest]
        trees.append(comb(rng, F, feats))
    while len(trees) < n_trees:
        trees.append(random_tree(rng, F, feats, max_depth, cat_feats))
    return trees


def zero_cover_tree(F=3):
    """Depth 3 over 3 features; the right child of node 1 and the left
    child of node 2 have no cover, and so has everything below them."""
    tree = RegTree(F)
    l, r = tree.add_split(0, 0, 0.0, True, 1.0, 0.0, 0.3, -0.2, 8.0, 5.0, 3.0)
    ll, lr = tree.add_split(l, 1, 0.25, False, 1.0, 0.0, 0.7, -0.9, 5.0,
                            5.0, 0.0)
    rl, rr = tree.add_split(r, 2, 1.0, True, 1.0, 0.0, 0.45, 0.15, 3.0,
                            0.0, 3.0)
    tree.add_split(ll, 2, -0.5, True, 1.0, 0.0, -0.35, 0.6, 5.0, 1.75, 3.25)
    tree.add_split(lr, 2, 0.0, False, 1.0, 0.0, 0.8, -0.55, 0.0, 0.0, 0.0)
    tree.add_split(rl, 1, 0.0, False, 1.0, 0.0, -0.65, 0.25, 0.0, 0.0, 0.0)
    tree.add_split(rr, 0, 1.0, True, 1.0, 0.0, 0.5, -0.4, 3.0, 1.25, 1.75)
    return tree


def zero_cover_rows():
    """Rows to every leaf of zero_cover_tree, missing ones included."""
    vals = [np.float32(-1.0), np.float32(0.5), np.float32(2.0),
            np.float32("nan")]
    return np.array([[a, b, c] for a in vals for b in vals for c in vals],
                    np.float32)


# -- rows ------------------------------------------------------------------------

def rows(seed, n, F, missing=np.nan, cat_feats=()):
    """[n, F] float32 drawn mostly from GRID, so many values sit exactly
    on a threshold; also the float32 neighbours of a threshold on either
    side, NaN, +-inf, a few off-grid values and, with a numeric
    `missing`, that sentinel.  Categorical columns draw category ids."""
    rng = np.random.RandomState(seed)
    below = np.nextafter(GRID, np.float32(-np.inf))
    above = np.nextafter(GRID, np.float32(np.inf))
    special = [np.float32("nan"), np.float32("inf"), np.float32("-inf")]
    if not np.isnan(missing):
        special.append(np.float32(missing))
    kind = rng.choice(5, (n, F), p=[0.35, 0.15, 0.15, 0.15, 0.2])
    pick = rng.randint(0, len(GRID), (n, F))
    X = np.where(kind == 0, GRID[pick], 0).astype(np.float32)
    X = np.where(kind == 1, below[pick], X)
    X = np.where(kind == 2, above[pick], X)
    X = np.where(kind == 3, rng.randn(n, F).astype(np.float32), X)
    sp_pick = np.asarray(special, np.float32)[rng.randint(0, len(special),
                                                          (n, F))]
    X = np.where(kind == 4, sp_pick, X).astype(np.float32)
    for c in cat_feats:
        X[:, c] = CAT_VALUES[rng.randint(0, len(CAT_VALUES), n)]
        X[rng.rand(n) < 0.1, c] = (np.nan if np.isnan(missing) else missing)
    return X


def assert_edge_values(trees, X, missing=np.nan):
    """Each kind of edge value occurs in a numeric split feature: on a
    threshold, its float32 neighbour on either side, +-inf, NaN and the
    sentinel; with categorical splits, a member past bit 32 too."""
    seen = dict.fromkeys(("on", "below", "above", "+inf", "-inf", "nan"),
                         False)
    if not np.isnan(missing):
        seen["sentinel"] = False
    for t in trees:
        for nid in np.nonzero(t.left[:t.n_nodes] != -1)[0]:
            x = X[:, t.split_index[nid]]
            if t.split_type[nid] == 1:
                seen["cat>32"] = seen.get("cat>32", False) or bool(
                    np.isin(x[x > 32], t.cat_segments[nid]).any())
                continue
            c = np.float32(t.split_cond[nid])
            seen["on"] |= bool((x == c).any())
            seen["below"] |= bool(
                (x == np.nextafter(c, np.float32(-np.inf))).any())
            seen["above"] |= bool(
                (x == np.nextafter(c, np.float32(np.inf))).any())
            seen["+inf"] |= bool(np.isposinf(x).any())
            seen["-inf"] |= bool(np.isneginf(x).any())
            seen["nan"] |= bool(np.isnan(x).any())
            if "sentinel" in seen:
                seen["sentinel"] |= bool((x == np.float32(missing)).any())
    assert all(seen.values()), seen


def to_csr(X):
    """CSR that stores every non-NaN entry of X, zeros included."""
    keep = ~np.isnan(X)
    r, c = np.nonzero(keep)
    indptr = np.zeros(X.shape[0] + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return sp.csr_matrix((X[r, c], c.astype(np.int32), indptr),
                         shape=X.shape)


# -- boosters ---------------------------------------------------------------------

def booster(trees, F, n_groups=1, device="cpu"):
    """A booster over F columns that holds `trees`, dealt round-robin
    over n_groups outputs, saved and loaded on `device`."""
    from test_shap_csr import _hand_booster, _reload
    if n_groups == 1:
        return _reload(_hand_booster(trees, F), device)
    assert len(trees) % n_groups == 0
    rng = np.random.RandomState(1)
    X = rng.randn(32, F).astype(np.float32)
    y = (np.arange(32) % n_groups).astype(np.float32)
    bst = xgb.train({"objective": "multi:softprob", "num_class": n_groups,
                     "max_depth": 1, "max_bin": 8}, xgb.DMatrix(X, label=y),
                    1, verbose_eval=False)
    bst.trees = list(trees)
    bst.tree_info = [i % n_groups for i in range(len(trees))]
    bst.iteration_indptr = list(range(0, len(trees) + 1, n_groups))
    return _reload(bst, device)


def with_base(ref, bst):
    """The reference with the booster's base margin in the bias cell."""
    out = ref.copy()
    out[(Ellipsis,) + (-1,) * (ref.ndim - 2)] += bst._base_margin_value()
    return out


# -- tolerances ---------------------------------------------------------------------

F32_EPS = 2.0 ** -23


def scale(ref):
    return float(np.abs(ref).max())


def used_features(trees):
    return np.unique(np.concatenate(
        [split_features(t) for t in trees] + [np.zeros(0, int)]))


def assert_close(got, ref, trees, cube=False, what="", rel_bound=None):
    """`got` against the fp64 reference `ref` of the forest `trees`,
    every cell.  Cells that are zero by definition (a feature no tree
    splits on; the bias row and column of a `cube` but for the corner)
    are compared with ==.  An fp64 result gets 1e-12 * S, S the largest
    |reference|.  A float32 result, computed in fp64 and cast once, gets
    2^-23 * S, and an interaction diagonal 2^-23 * S * (k + 1) with k
    the nonzero off-diagonal cells of its row.  `rel_bound` replaces
    these by rel_bound * S (the DFS kernel, whose bound is measured).
    Returns max |err| / S."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert got.dtype in (np.float32, np.float64), got.dtype
    assert not np.isnan(got).any(), f"{what}: NaN in the result"
    S = scale(ref)
    C = ref.shape[-1]
    live = np.zeros(C, bool)
    live[used_features(trees)] = True
    if cube:
        zero = ~(live[:, None] & live[None, :])
        zero[C - 1, C - 1] = False
    else:
        zero = ~live
        zero[C - 1] = False
    assert (ref[..., zero] == 0.0).all()
    assert (got[..., zero] == 0.0).all(), \
        f"{what}: a cell that is zero by definition is not 0.0"
    if rel_bound is not None:
        bound = np.full(ref.shape, rel_bound * S)
    elif got.dtype == np.float64:
        bound = np.full(ref.shape, 1e-12 * S)
    else:
        bound = np.full(ref.shape, F32_EPS * S)
        if cube:
            k = (ref != 0).sum(axis=-1) - (ref[..., np.arange(C),
                                               np.arange(C)] != 0)
            bound[..., np.arange(C), np.arange(C)] = F32_EPS * S * (k + 1)
    err = np.abs(got.astype(np.float64) - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: S={S:.4g} max|err|={err.max():.3e} "
          f"({err.max() / max(S, 1e-300):.3e} S) dtype={got.dtype}")
    assert (err <= bound).all(), (
        f"{what}: |err| {err[worst]:.3e} > {bound[worst]:.3e} at {worst}: "
        f"got {got[worst]!r}, reference {ref[worst]!r}")
    return err.max() / S


# -- the device guard ------------------------------------------------------------------

def boom(*a, **k):
    raise AssertionError("host SHAP recursion used on the device path")


@contextlib.contextmanager
def host_recursion_raises(monkeypatch, shap_module):
    """While the block runs, the host recursion of `shap_module`
    (xgboost_amd.shap, passed in so that this file imports none of it)
    raises: a silent fallback from the device fails the test."""
    with monkeypatch.context() as m:
        m.setattr(shap_module, "_tree_shap", boom)
        m.setattr(shap_module, "_saabas", boom)
        yield m
