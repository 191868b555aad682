"""Bin-based prediction on external-memory matrices (host paths) and the
host split-bin helper that the packed-node GPU predictor builds on."""
import numpy as np

import xgboost_amd as xgb
from xgboost_amd.data import quantize_dense
from xgboost_amd.extmem import DataIter, ExtMemQuantileDMatrix
from xgboost_amd.quantile import make_cuts
from xgboost_amd.tree_model import RegTree, local_split_bins


class _Iter(DataIter):
    def __init__(self, Xs, ys=None):
        super().__init__()
        self.Xs, self.ys, self.i = Xs, ys, 0

    def reset(self):
        self.i = 0

    def next(self, input_data) -> bool:
        if self.i >= len(self.Xs):
            return False
        kw = {"data": self.Xs[self.i]}
        if self.ys is not None:
            kw["label"] = self.ys[self.i]
        input_data(**kw)
        self.i += 1
        return True


def _split(a, sizes):
    return np.split(a, np.cumsum(sizes)[:-1])


def test_pred_leaf_extmem_matches_incore():
    rng = np.random.RandomState(3)
    X = rng.randn(600, 5).astype(np.float32)
    X[rng.rand(600, 5) < 0.1] = np.nan
    y = (np.nan_to_num(X[:, 0]) - np.nan_to_num(X[:, 1]) > 0).astype(
        np.float32)
    sizes = [349, 1, 250]  # unequal pages, one single-row page
    d_ext = ExtMemQuantileDMatrix(_Iter(_split(X, sizes), _split(y, sizes)),
                                  max_bin=32)
    assert [p.n_rows for p in d_ext.pages] == sizes
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 4,
                     "max_bin": 32}, d_ext, 4, verbose_eval=False)
    leaf_ext = bst.predict(d_ext, pred_leaf=True)
    leaf_in = bst.predict(xgb.DMatrix(X), pred_leaf=True)
    assert leaf_ext.shape == (600, 4)
    assert leaf_ext.dtype == leaf_in.dtype
    assert np.array_equal(leaf_ext, leaf_in)
    strict = bst.predict(d_ext, pred_leaf=True, strict_shape=True,
                         iteration_range=(1, 3))
    assert strict.shape == (600, 2, 1, 1)
    assert np.array_equal(strict.reshape(600, 2), leaf_in[:, 1:3])


def test_vector_leaf_extmem_matches_incore():
    rng = np.random.RandomState(5)
    X = rng.randn(500, 6).astype(np.float32)
    X[rng.rand(500, 6) < 0.05] = np.nan
    W = rng.randn(6, 3)
    Y = (np.nan_to_num(X) @ W + 0.1 * rng.randn(500, 3)).astype(np.float32)
    d_in = xgb.DMatrix(X, label=Y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 4,
                     "multi_strategy": "multi_output_tree", "eta": 0.3,
                     "max_bin": 32}, d_in, 4, verbose_eval=False)
    assert all(t.leaf_values is not None for t in bst.trees)
    sizes = [200, 1, 299]
    d_ext = ExtMemQuantileDMatrix(_Iter(_split(X, sizes)), max_bin=32,
                                  ref=d_in)
    p_in = bst.predict(xgb.DMatrix(X))
    p_ext = bst.predict(d_ext)
    assert p_ext.shape == (500, 3)
    assert np.array_equal(p_ext, p_in)
    # DART drop-set helper takes the same branch
    sub_ext = bst._predict_tree_subset(d_ext, [0, 2]).cpu().numpy()
    sub_in = bst._predict_tree_subset(xgb.DMatrix(X), [0, 2]).cpu().numpy()
    assert np.array_equal(sub_ext, sub_in)


def _random_tree(rng, n_features, cond_of, depth=4):
    tree = RegTree(n_features)
    frontier = [0]
    for _ in range(depth):
        nxt = []
        for nid in frontier:
            if rng.rand() < 0.2 and nid != 0:
                continue
            f = int(rng.randint(n_features))
            l, r = tree.add_split(nid, f, cond_of(f), bool(rng.rand() < 0.5),
                                  1.0, 0.0, rng.randn(), rng.randn(),
                                  1.0, 0.5, 0.5)
            nxt += [l, r]
        frontier = nxt
    return tree


def _bin_walk(tree, local, cuts):
    """The kernel's rule on local bins, in numpy."""
    n = tree.n_nodes
    sb = np.zeros(n, np.int64)
    inner = tree.left[:n] != -1
    sb[inner] = local_split_bins(tree.split_index[:n][inner],
                                 tree.split_cond[:n][inner], cuts)
    n_bins = np.diff(cuts.ptrs)
    pos = np.zeros(local.shape[0], np.int32)
    for _ in range(64):
        live = tree.left[pos] != -1
        if not live.any():
            break
        f = tree.split_index[pos]
        b = local[np.arange(local.shape[0]), f]
        missing = b >= n_bins[f]
        go_left = np.where(missing, tree.default_left[pos] != 0, b <= sb[pos])
        nxt = np.where(go_left, tree.left[pos], tree.right[pos])
        pos = np.where(live, nxt, pos).astype(np.int32)
    return pos


def test_local_split_bins_reproduces_raw_traversal():
    rng = np.random.RandomState(11)
    n, F = 400, 4
    X = rng.randn(n, F).astype(np.float32)
    X[:, 3] = rng.randint(0, 7, n)  # few distinct values: ties on cuts
    X[rng.rand(n, F) < 0.1] = np.nan
    cuts = make_cuts(X, 16)
    # rows that sit exactly on every cut, and on the column min and max
    extra = []
    for f in range(F):
        col = X[:, f]
        for v in list(cuts.feature_cuts(f)) + [np.nanmin(col),
                                               np.nanmax(col)]:
            if v <= np.nanmax(col):  # the last cut lies above the data
                row = X[rng.randint(n)].copy()
                row[f] = v
                extra.append(row)
    X = np.vstack([X, np.asarray(extra, np.float32)])
    qm = quantize_dense(X, cuts)
    local = qm.gidx.numpy().astype(np.int64)
    if qm.gidx.dtype.itemsize == 2:
        local &= 0xFFFF
    gg = qm.global_gidx().numpy()
    for seed in range(8):
        trng = np.random.RandomState(100 + seed)
        tree = _random_tree(
            trng, F, lambda f: float(trng.choice(cuts.feature_cuts(f))))
        got = _bin_walk(tree, local, cuts)
        assert np.array_equal(got, tree.predict_leaf_np(X)), seed
        assert np.array_equal(got, tree.predict_leaf_bins(gg, cuts)), seed


def test_local_split_bins_off_cut_conditions_follow_bin_oracle():
    """A model from elsewhere: split conditions between, below and above
    the cut values.  Bin traversal cannot match raw traversal there; it
    must match RegTree.predict_leaf_bins."""
    rng = np.random.RandomState(12)
    n, F = 300, 3
    X = rng.randn(n, F).astype(np.float32)
    X[rng.rand(n, F) < 0.1] = np.nan
    cuts = make_cuts(X, 16)
    qm = quantize_dense(X, cuts)
    local = qm.gidx.numpy().astype(np.int64)
    gg = qm.global_gidx().numpy()
    for seed in range(8):
        trng = np.random.RandomState(200 + seed)

        def cond_of(f):
            fc = cuts.feature_cuts(f)
            return float(trng.uniform(fc[0] - 1.0, fc[-1] + 1.0))

        tree = _random_tree(trng, F, cond_of)
        got = _bin_walk(tree, local, cuts)
        assert np.array_equal(got, tree.predict_leaf_bins(gg, cuts)), seed
    # a single split whose condition exceeds every cut: all rows left
    tree = RegTree(F)
    tree.add_split(0, 1, float(cuts.feature_cuts(1)[-1] + 5.0), False,
                   1.0, 0.0, -1.0, 1.0, 1.0, 0.5, 0.5)
    got = _bin_walk(tree, local, cuts)
    assert np.array_equal(got, tree.predict_leaf_bins(gg, cuts))
    assert set(got[~np.isnan(X[:, 1])]) == {1}


def _walk_packed(fa, X):
    """numpy model of the packed-node kernel over a _ForestQ built on
    the host: returns (leaf ids [n, T], margins added to zeros [n, K])."""
    nodes = fa.nodes.numpy().view(np.uint32).reshape(-1, 4)
    left = nodes[:, 0].view(np.int32)
    right = nodes[:, 1].view(np.int32)
    feat = (nodes[:, 2] & np.uint32((1 << 30) - 1)).astype(np.int64)
    dleft = (nodes[:, 2] >> np.uint32(31)) != 0
    is_cat = (nodes[:, 2] & np.uint32(1 << 30)) != 0
    offs = fa.tree_offsets.numpy()
    cat_off = fa.cat_offsets.numpy()
    cat_bits = fa.cat_bits.numpy().view(np.uint32)
    raw = X.dtype == np.float32
    n_bins = None if raw else fa.n_bins.numpy()
    n = X.shape[0]
    rows = np.arange(n)
    leaf = np.zeros((n, fa.n_trees), np.int32)
    out = np.zeros((n, fa.n_outputs), np.float32)
    for t in range(fa.n_trees):
        base = int(offs[t])
        pos = np.zeros(n, np.int64)
        for _ in range(64):
            g = base + pos
            live = left[g] != -1
            if not live.any():
                break
            v = X[rows, feat[g]]
            if raw:
                missing = np.isnan(v)
                cat = np.nan_to_num(v).astype(np.int64)
                num_left = v < nodes[g, 3].view(np.float32)
            else:
                v = v.astype(np.int64)
                missing = v >= n_bins[feat[g]]
                cat = v
                num_left = v <= nodes[g, 3].astype(np.int64)
            nw = cat_off[g + 1] - cat_off[g]
            ok = (cat >= 0) & ((cat >> 5) < nw)
            word = cat_bits[np.where(ok, cat_off[g] + (cat >> 5), 0)]
            in_set = ok & (((word >> (cat & 31).astype(np.uint32)) & 1) != 0)
            go_left = np.where(missing, dleft[g],
                               np.where(is_cat[g], ~in_set, num_left))
            nxt = np.where(go_left, left[g], right[g])
            pos = np.where(live, nxt, pos)
        leaf[:, t] = pos
        grp = int(fa.tree_group.numpy()[t])
        if grp >= 0:
            out[:, grp] += nodes[base + pos, 3].view(np.float32)
        else:
            vo = int(fa.vec_offset.numpy()[t])
            out += fa.leaf_vec.numpy()[vo + pos]
    return leaf, out


def test_packed_forest_records_walk_like_the_host():
    """_ForestQ packing (node records, category bitsets, split bins,
    scalar and vector leaf stores) checked on the host against the tree
    model's own traversals, for bin and raw-float inputs."""
    from xgboost_amd.backend.gpu import _ForestQ
    rng = np.random.RandomState(21)
    n = 500
    cat = rng.randint(0, 40, n).astype(np.float32)
    Xn = rng.randn(n, 3).astype(np.float32)
    X = np.concatenate([cat[:, None], Xn], axis=1)
    X[rng.rand(n, 4) < 0.08] = np.nan
    good = [1, 5, 7, 12, 19, 22, 28, 33, 36, 39]
    y = (np.isin(cat, good) * 2.0 + 0.5 * np.nan_to_num(Xn[:, 0])
         + 0.1 * rng.randn(n)).astype(np.float32)
    ft = ["c", "q", "q", "q"]
    d = xgb.DMatrix(X, label=y, feature_types=ft)
    bst = xgb.train({"max_depth": 4, "max_bin": 16, "max_cat_to_onehot": 1,
                     "eta": 0.5}, d, 4, verbose_eval=False)
    assert any(int(c.max()) >= 32 for t in bst.trees
               for c in t.cat_segments.values() if len(c))
    cuts = d.quantized(16).cuts
    qm = quantize_dense(X, cuts)
    gg = qm.global_gidx().numpy()
    want_leaf = np.stack([t.predict_leaf_bins(gg, cuts) for t in bst.trees],
                         axis=1)
    fa_bins = _ForestQ(bst, range(len(bst.trees)), "cpu", cuts)
    leaf, out = _walk_packed(fa_bins, qm.gidx.numpy())
    assert np.array_equal(leaf, want_leaf)
    fa_raw = _ForestQ(bst, range(len(bst.trees)), "cpu", None)
    leaf_r, out_r = _walk_packed(fa_raw, X)
    assert np.array_equal(
        leaf_r, np.stack([t.predict_leaf_np(X) for t in bst.trees], axis=1))
    want = np.zeros((n, 1), np.float32)
    for t in bst.trees:
        want[:, 0] += t.split_cond[:t.n_nodes][t.predict_leaf_np(X)]
    assert np.array_equal(out_r, want)
    assert np.array_equal(out, want)  # conds are cuts: bins walk is exact

    # vector leaves
    W = rng.randn(4, 3)
    Y = (np.nan_to_num(X) @ W).astype(np.float32)
    bmt = xgb.train({"max_depth": 3, "max_bin": 16, "eta": 0.5,
                     "multi_strategy": "multi_output_tree"},
                    xgb.DMatrix(X[:, 1:], label=Y), 3, verbose_eval=False)
    fa = _ForestQ(bmt, range(len(bmt.trees)), "cpu", None)
    assert (fa.tree_group.numpy() == -1).all()
    _, out_v = _walk_packed(fa, X[:, 1:])
    want = np.zeros((n, 3), np.float32)
    for t in bmt.trees:
        want += t.leaf_values[:t.n_nodes][t.predict_leaf_np(X[:, 1:])]
    assert np.array_equal(out_v, want)
