"""SHAP values for tree ensembles.

Reference behavior: src/predictor/interpretability/shap.{cc,cu}
(Quadrature-TreeSHAP) — we provide the same outputs (exact SHAP
contributions, interactions, and the Saabas approximation for
approx_contribs) via the classic path-dependent TreeSHAP recursion
(Lundberg & Lee) on CPU; a HIP kernel accelerates pred_contribs on GPU
(ops/cpp/shap.hip).

Output convention matches xgboost: contribs shape [n, f+1] with the
last column the bias (expected value incl. base_score); interactions
[n, f+1, f+1]; multiclass adds a group axis [n, k, f+1].

A sparse CSR DMatrix is explained in the compact space of the columns
the forest splits on (absent entries and stored NaNs are missing) and
expanded to full width at the end, on the CPU and on the GPU alike.

Off-diagonal interaction cells hold the Shapley interaction index
Phi_ij (half the pair's joint effect in each of [i, j] and [j, i]); the
diagonal is phi_i minus the rest of its row.  A child without cover has
weight 0.

Output dtype: every route returns float32 (computed in fp64 and cast
once; the DFS kernel accumulates in float32), except dense device
pred_contribs on a numeric forest, which returns the path kernel's
float64 as it is.  Only an ImportError (kernels not built, or a
ShapDeviceLimit) sends a device call to the host recursion; any other
exception from the device code is a bug and propagates.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .tree_model import RegTree


def _extend(path: List[List[float]], zero: float, one: float, fi: int) -> None:
    length = len(path)
    path.append([fi, zero, one, 1.0 if length == 0 else 0.0])
    for i in range(length - 1, -1, -1):
        path[i + 1][3] += one * path[i][3] * (i + 1) / (length + 1)
        path[i][3] = zero * path[i][3] * (length - i) / (length + 1)


def _unwind(path: List[List[float]], idx: int) -> None:
    length = len(path) - 1
    one = path[idx][2]
    zero = path[idx][1]
    n = path[length][3]
    for j in range(length - 1, -1, -1):
        if one != 0:
            t = path[j][3]
            path[j][3] = n * (length + 1) / ((j + 1) * one)
            n = t - path[j][3] * zero * (length - j) / (length + 1)
        else:
            path[j][3] = path[j][3] * (length + 1) / (zero * (length - j))
    # shift feature/zero/one down; pweights stay in place (the canonical
    # UNWIND keeps the recomputed pweights at indices 0..length-1)
    for j in range(idx, length):
        path[j][0] = path[j + 1][0]
        path[j][1] = path[j + 1][1]
        path[j][2] = path[j + 1][2]
    del path[length]


def _unwound_sum(path: List[List[float]], idx: int) -> float:
    length = len(path) - 1
    one = path[idx][2]
    zero = path[idx][1]
    total = 0.0
    n = path[length][3]
    for j in range(length - 1, -1, -1):
        if one != 0:
            t = n * (length + 1) / ((j + 1) * one)
            total += t
            n = path[j][3] - t * zero * (length - j) / (length + 1)
        else:
            total += path[j][3] / (zero * (length - j) / (length + 1))
    return total


def _decision(tree: RegTree, nid: int, x: np.ndarray, missing: float
              ) -> Tuple[int, int]:
    """Return (hot child, cold child) for row x at node nid."""
    f = int(tree.split_index[nid])
    v = x[f]
    is_missing = bool(np.isnan(v)) if np.isnan(missing) else \
        bool(v == missing or np.isnan(v))
    left, right = int(tree.left[nid]), int(tree.right[nid])
    if is_missing:
        hot = left if tree.default_left[nid] else right
    elif tree.split_type[nid] == 1:
        cats = tree.cat_segments.get(nid)
        in_set = cats is not None and int(v) in cats
        hot = right if in_set else left
    else:
        hot = left if v < tree.split_cond[nid] else right
    cold = right if hot == left else left
    return hot, cold


def _tree_shap(tree: RegTree, x: np.ndarray, phi: np.ndarray,
               missing: float, condition: int = 0,
               condition_feature: int = -1) -> None:
    """Path-dependent TreeSHAP (Lundberg & Lee alg. 2, with the
    conditional variant used for interaction values)."""

    def recurse(nid: int, path: List[List[float]], zero: float, one: float,
                pfeat: int, cond_frac: float) -> None:
        # an element with zero == one == 0 (a cold child without cover)
        # zeroes every weight below it: prune, nothing divides by it
        if cond_frac == 0.0 or (zero == 0.0 and one == 0.0):
            return
        path = [list(e) for e in path]
        if condition == 0 or condition_feature != pfeat:
            _extend(path, zero, one, pfeat)
        if tree.is_leaf(nid):
            leaf = float(tree.split_cond[nid])
            for i in range(1, len(path)):
                w = _unwound_sum(path, i)
                phi[int(path[i][0])] += (
                    w * (path[i][2] - path[i][1]) * leaf * cond_frac)
            return
        hot, cold = _decision(tree, nid, x, missing)
        f = int(tree.split_index[nid])
        cover = max(float(tree.sum_hess[nid]), 1e-16)
        hot_zero = float(tree.sum_hess[hot]) / cover
        cold_zero = float(tree.sum_hess[cold]) / cover
        incoming_zero, incoming_one = 1.0, 1.0
        idx = -1
        for i in range(1, len(path)):
            if int(path[i][0]) == f:
                idx = i
                break
        if idx >= 0:
            incoming_zero, incoming_one = path[idx][1], path[idx][2]
            _unwind(path, idx)
        hot_cf, cold_cf = cond_frac, cond_frac
        if condition > 0 and f == condition_feature:
            cold_cf = 0.0
        elif condition < 0 and f == condition_feature:
            hot_cf *= hot_zero
            cold_cf *= cold_zero
        recurse(hot, path, incoming_zero * hot_zero, incoming_one, f, hot_cf)
        recurse(cold, path, incoming_zero * cold_zero, 0.0, f, cold_cf)

    recurse(0, [], 1.0, 1.0, -1, 1.0)


def _expected_value(tree: RegTree) -> float:
    """Cover-weighted mean of leaf values (phi_0 of the tree)."""
    total = 0.0
    root_cover = max(float(tree.sum_hess[0]), 1e-16)
    for nid in range(tree.n_nodes):
        if tree.is_leaf(nid) and (tree.parent[nid] != -1 or nid == 0):
            total += float(tree.split_cond[nid]) * float(tree.sum_hess[nid])
    return total / root_cover


def _host_contribs(trees, groups, X: np.ndarray, phi: np.ndarray,
                   missing: float, approx: bool) -> None:
    """Add every tree's contributions to phi [n, groups, f + 1]."""
    n, f = X.shape
    for tree, k in zip(trees, groups):
        phi[:, k, f] += _expected_value(tree)
        if approx:
            _saabas(tree, X, phi[:, k, :], missing)
        else:
            for i in range(n):
                _tree_shap(tree, X[i], phi[i, k], missing)


def shap_values(booster, dmat, iteration_range=(0, 0),
                approx: bool = False) -> np.ndarray:
    lo, hi = booster._tree_range(iteration_range)
    n_groups = booster.n_outputs
    if _is_sparse(dmat):
        compact, used = _csr_contribs(booster, dmat, lo, hi, approx)
        phi = _expand_columns(compact, used, dmat.num_col(), 1)
        return phi[:, 0, :] if n_groups == 1 else phi
    X = dmat.raw_data()
    n, f = X.shape
    phi = np.zeros((n, n_groups, f + 1), dtype=np.float64)
    phi[:, :, f] = booster._base_margin_value()
    if booster.device.type == "cuda" and not approx:
        try:
            from .backend.gpu import shap_gpu
            return shap_gpu(booster, dmat, lo, hi, phi)
        except ImportError:
            pass  # kernels not built, or a ShapDeviceLimit: exact host
    _host_contribs(booster.trees[lo:hi], booster.tree_info[lo:hi], X, phi,
                   dmat.missing, approx)
    if n_groups == 1:
        return phi[:, 0, :].astype(np.float32)
    return phi.astype(np.float32)


def _saabas(tree: RegTree, X: np.ndarray, phi: np.ndarray,
            missing: float) -> None:
    """Gain-path approximation (xgboost approx_contribs)."""
    n = X.shape[0]
    mean_val = np.zeros(tree.n_nodes)
    for nid in range(tree.n_nodes - 1, -1, -1):
        if tree.is_leaf(nid):
            mean_val[nid] = float(tree.split_cond[nid])
        else:
            l, r = int(tree.left[nid]), int(tree.right[nid])
            hl, hr = float(tree.sum_hess[l]), float(tree.sum_hess[r])
            tot = max(hl + hr, 1e-16)
            mean_val[nid] = (mean_val[l] * hl + mean_val[r] * hr) / tot
    for i in range(n):
        nid = 0
        while not tree.is_leaf(nid):
            hot, _ = _decision(tree, nid, X[i], missing)
            f = int(tree.split_index[nid])
            phi[i, f] += mean_val[hot] - mean_val[nid]
            nid = hot


def shap_interactions(booster, dmat, iteration_range=(0, 0)) -> np.ndarray:
    lo, hi = booster._tree_range(iteration_range)
    if _is_sparse(dmat):
        compact, used = _csr_interactions(booster, dmat, lo, hi)
        out = _expand_columns(compact, used, dmat.num_col(), 2)
        return out[:, 0] if booster.n_outputs == 1 else out
    if booster.device.type == "cuda":
        try:
            from .backend.gpu import shap_interactions_gpu
            return shap_interactions_gpu(booster, dmat, lo, hi,
                                         iteration_range)
        except ImportError:
            pass  # categorical / deep-path forests: exact CPU fallback
    X = dmat.raw_data()
    n_groups = booster.n_outputs
    base = shap_values(booster, dmat, iteration_range).astype(np.float64)
    if n_groups == 1:
        base = base[:, None, :]
    out = _host_interactions(booster.trees[lo:hi], booster.tree_info[lo:hi],
                             X, base, dmat.missing)
    if n_groups == 1:
        return out[:, 0].astype(np.float32)
    return out.astype(np.float32)


def _host_interactions(trees, groups, X: np.ndarray, base: np.ndarray,
                       missing: float) -> np.ndarray:
    """Interaction cube [n, groups, f + 1, f + 1] in fp64; the diagonal
    is completed from the contributions `base` [n, groups, f + 1]."""
    n, f = X.shape
    out = np.zeros((n, base.shape[1], f + 1, f + 1), dtype=np.float64)
    for tree, k in zip(trees, groups):
        used = sorted(set(int(tree.split_index[nid])
                          for nid in range(tree.n_nodes)
                          if not tree.is_leaf(nid)))
        for j in used:
            phi_on = np.zeros((n, f + 1))
            phi_off = np.zeros((n, f + 1))
            for i in range(n):
                _tree_shap(tree, X[i], phi_on[i], missing,
                           condition=1, condition_feature=j)
                _tree_shap(tree, X[i], phi_off[i], missing,
                           condition=-1, condition_feature=j)
            # (on - off) / 2 is the index of the ordered pair (i, j); it
            # goes into both cells, so each gets half from either order
            diff = (phi_on - phi_off) / 4.0
            diff[:, j] = 0.0
            out[:, k, j, :] += diff
            out[:, k, :, j] += diff
    for i_ in range(f + 1):
        out[:, :, i_, i_] = base[:, :, i_] - (
            out[:, :, i_, :].sum(axis=-1) - out[:, :, i_, i_])
    return out


# -- sparse CSR input: compact used-column space --------------------------

def _is_sparse(dmat) -> bool:
    return getattr(dmat, "_sparse_data", None) is not None


def used_columns(trees, n_col: int) -> Tuple[np.ndarray, np.ndarray]:
    """(used, col_map) for a forest over an `n_col`-wide matrix: `used`
    is the sorted array of distinct split features, `col_map[c]` the
    compact id of column c, or -1.  Compact ids ascend with the feature,
    so build_path_table keeps every path's element order under the remap
    and the fp64 accumulations run in the order they run on dense input.
    A split on a feature the matrix does not have has no output column
    to explain it in and raises."""
    feats = [t.split_index[:t.n_nodes][t.left[:t.n_nodes] != -1]
             for t in trees]
    used = (np.unique(np.concatenate(feats)).astype(np.int64) if feats
            else np.zeros(0, np.int64))
    if len(used) and (used[-1] >= n_col or used[0] < 0):
        bad = int(used[-1]) if used[-1] >= n_col else int(used[0])
        raise ValueError(
            f"the model splits on feature {bad}, but the matrix has "
            f"{n_col} columns: no output column can hold its contribution")
    col_map = np.full(n_col, -1, dtype=np.int32)
    col_map[used] = np.arange(len(used), dtype=np.int32)
    return used, col_map


class _RemappedTree:
    """Read-only view of a RegTree whose split features are compact
    ids; every other attribute is the tree's own."""

    def __init__(self, tree: RegTree, col_map: np.ndarray):
        self._tree = tree
        n = tree.n_nodes
        split_index = tree.split_index[:n].copy()
        internal = tree.left[:n] != -1
        split_index[internal] = col_map[split_index[internal]]
        self.split_index = split_index

    def __getattr__(self, name):
        return getattr(self._tree, name)


def _gather_used_columns(csr, used: np.ndarray) -> np.ndarray:
    """[n, U] float32 of the used columns: NaN where the CSR stores
    nothing, the stored value (a 0.0 too) where it does."""
    X = np.full((csr.shape[0], len(used)), np.nan, dtype=np.float32)
    if len(used):
        sub = csr[:, used].tocoo()
        X[sub.row, sub.col] = sub.data
    return X


def _expand_columns(compact: np.ndarray, used: np.ndarray, n_col: int,
                    n_axes: int) -> np.ndarray:
    """Compact [n, g, U+1] (n_axes=1) or [n, g, U+1, U+1] (n_axes=2) to
    the full-width float32 output: exact 0.0 in every unused column, the
    bias in the last one."""
    if len(used) == n_col:  # every column is used: compact is full width
        return np.ascontiguousarray(compact, dtype=np.float32)
    n, g = compact.shape[:2]
    dst = np.append(used, n_col).astype(np.int64)
    out = np.zeros((n, g) + (n_col + 1,) * n_axes, dtype=np.float32)
    if n_axes == 1:
        out[:, :, dst] = compact
    else:
        out[:, :, dst[:, None], dst[None, :]] = compact
    return out


def _csr_contribs(booster, dmat, lo: int, hi: int, approx: bool):
    """Compact float32 contributions [n, groups, U+1] and `used`."""
    used, col_map = used_columns(booster.trees[lo:hi], dmat.num_col())
    if booster.device.type == "cuda" and not approx:
        from .backend import gpu
        try:
            return gpu.shap_csr_gpu(booster, dmat, lo, hi, used, col_map), used
        except gpu.ShapDeviceLimit:
            pass  # categorical past the DFS caps / deep paths: exact host
    n, u = dmat.num_row(), len(used)
    X = _gather_used_columns(dmat.sparse_data(), used)
    phi = np.zeros((n, booster.n_outputs, u + 1), dtype=np.float64)
    phi[:, :, u] = booster._base_margin_value()
    trees = [_RemappedTree(t, col_map) for t in booster.trees[lo:hi]]
    _host_contribs(trees, booster.tree_info[lo:hi], X, phi, np.nan, approx)
    return phi.astype(np.float32), used


def _csr_interactions(booster, dmat, lo: int, hi: int):
    """Compact float32 interactions [n, groups, U+1, U+1] and `used`."""
    used, col_map = used_columns(booster.trees[lo:hi], dmat.num_col())
    if booster.device.type == "cuda":
        from .backend import gpu
        try:
            return gpu.shap_interactions_csr_gpu(booster, dmat, lo, hi, used,
                                                 col_map), used
        except gpu.ShapDeviceLimit:
            pass  # categorical / deep-path forests: exact host
    base, _ = _csr_contribs(booster, dmat, lo, hi, False)
    X = _gather_used_columns(dmat.sparse_data(), used)
    trees = [_RemappedTree(t, col_map) for t in booster.trees[lo:hi]]
    out = _host_interactions(trees, booster.tree_info[lo:hi], X,
                             base.astype(np.float64), np.nan)
    return out.astype(np.float32), used
