"""Native CPU split evaluator (gbt_evaluate_cpu) against the numpy oracle
on the synthetic histograms the HIP evaluator tests use: the selected
split per node, exact in everything but the gain's last bits."""
import ctypes

import numpy as np
import pytest

import eval_cases as ec
from xgboost_amd.params import make_train_param
from xgboost_amd.splits import evaluate_splits_np


def _check(k, params=None, monotone=None, bounds=None, mask=None):
    from xgboost_amd import ops
    lib = ops.load()  # a missing library is an error, not a skip
    hist, parents = ec.hists(k)
    p = make_train_param(dict({"max_depth": 6}, **(params or {})))

    def cp(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dt)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    keep = [cp(hist, np.int64), cp(ec.PTRS, np.int32), cp(parents, np.int64),
            cp(monotone, np.int8), cp(bounds, np.float64),
            cp(mask, np.uint8)]
    h, ptrs, par, mono, bnd, msk = (c[1] for c in keep)
    best = np.full((k, 6), -77, np.int64)
    lib.gbt_evaluate_cpu(h, k, ec.NB, ec.F, ptrs, par, ec.G_SCALE,
                         ec.H_SCALE, p.reg_lambda, p.reg_alpha,
                         p.max_delta_step, p.min_child_weight, mono, bnd,
                         msk, best.ctypes.data_as(ctypes.c_void_p))
    fsets = (None if mask is None
             else [np.nonzero(r)[0] for r in mask])
    want = evaluate_splits_np(
        hist, [tuple(int(v) for v in r) for r in parents], ec.G_SCALE,
        ec.H_SCALE, list(range(k)), ec.PTRS, p, feature_sets=fsets,
        monotone=monotone, node_bounds=bounds)
    ec.check_best_against_oracle(best, want, k)
    for i, e in enumerate(want):
        if e.feature < 0:  # the whole no-split record
            assert best[i].tolist() == [0, -1, 0, 0, 0, -1]


@pytest.mark.parametrize("k", [1, 3, 130])
def test_cpu_evaluate_matches_oracle(k):
    _check(k)


def test_cpu_evaluate_regularized():
    _check(5, params=ec.REGULARIZED)


def test_cpu_evaluate_monotone_with_bounds():
    mono, bounds = ec.monotone_and_bounds(5)
    _check(5, monotone=mono, bounds=bounds)


def test_cpu_evaluate_per_node_mask():
    _check(5, mask=ec.per_node_mask(5))
