"""Histogram kernels (hist.hip) at every launch mode, bin type and
geometry edge, bit-exactly against the plain reference in hist_cases.py.

Each geometry first asserts the bin dtype, group count and launch mode
GpuOps selects for it, so a case cannot drift onto another kernel, and
only then compares numbers.  No tolerance anywhere: int64 fixed point.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hist_cases as hc

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gops(case, name=None):
    from xgboost_amd.backend.gpu import GpuOps
    gops = GpuOps(case.qm.to("cuda"))
    if name is not None:
        dtype, n_groups, mode = hc.GEOMETRIES[name][2:]
        assert gops.qm.gidx.dtype == dtype
        assert gops.n_groups == n_groups
        assert gops.use_shared == mode
    return gops


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _seg_tasks(segs):
    return [(i, s, e) for i, (s, e) in enumerate(segs)]


def _build_hist(gops, case, qg, ridx, segs):
    got = gops.build_hist(_dev(qg), _dev(ridx), segs)
    torch.cuda.synchronize()
    ref = hc.ref_hist(case, qg, ridx, _seg_tasks(segs), len(segs))
    assert got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), ref)
    return ref


def _launch(gops, qg, ridx, tasks, k, mode, with_sums=False):
    """gbt_hist called directly: (hist, node_sums) as numpy."""
    hip = gops.hip
    tasks_d = _dev(np.asarray(tasks, np.int32).reshape(-1, 4))
    qg_d, ridx_d = _dev(qg), _dev(ridx)
    out = torch.zeros((k, gops.n_bins, 2), dtype=torch.int64, device="cuda")
    sums = torch.zeros((k, 2), dtype=torch.int64, device="cuda") \
        if with_sums else None
    p8, p16 = gops._gidx_ptrs()
    gops.lib.gbt_hist(
        p8, p16, gops.qm.n_features, hip.ptr(qg_d), hip.ptr(ridx_d),
        hip.ptr(tasks_d), tasks_d.shape[0], hip.ptr(out), gops.n_bins,
        hip.ptr(gops.feat_group_start), hip.ptr(gops.bin_group_start),
        gops.n_groups, gops.max_group_bins, hip.ptr(gops.cut_ptrs),
        mode, hip.ptr(sums), hip.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), (sums.cpu().numpy() if with_sums else None)


# ---- geometry matrix ------------------------------------------------------

@pytest.mark.parametrize("name", sorted(hc.GEOMETRIES))
def test_hist_geometry(name):
    case = hc.geometry_case(name)
    gops = _gops(case, name)
    ridx = hc.subset_ridx(case.n_rows)
    ref = _build_hist(gops, case, hc.make_gpair(case.n_rows), ridx,
                      hc.three_segments(len(ridx)))
    assert not ref[1].any() and ref[0].any() and ref[2].any()


@pytest.mark.parametrize("n", hc.ROW_EDGES)
@pytest.mark.parametrize("name", ["A", "G"])
def test_hist_row_edges(name, n):
    case = hc.geometry_case(name, n=n, seed=n)
    gops = _gops(case, name)
    ridx = hc.subset_ridx(n, seed=n, frac=1.0)
    _build_hist(gops, case, hc.make_gpair(n, seed=n), ridx, [(0, n)])


@pytest.mark.parametrize("kind", hc.VALUE_EDGES)
@pytest.mark.parametrize("name", ["M", "A"])
def test_hist_value_edges(name, kind):
    case, qg = hc.value_edge(name, kind)
    gops = _gops(case, name)
    n = case.n_rows
    ridx = hc.subset_ridx(n, seed=5, frac=1.0)
    ref = _build_hist(gops, case, qg, ridx, [(0, n)])
    if kind == "cancel":
        assert not ref.any()
    if kind == "contention":
        assert np.count_nonzero(ref[0, :, 1]) == len(case.widths)


# ---- forced modes, node_sums, padded tasks --------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["A", "E"])
def test_hist_forced_mode(name, mode):
    case = hc.geometry_case(name)
    gops = _gops(case, name)  # selects 3: every lower mode is legal too
    ridx = hc.subset_ridx(case.n_rows)
    tasks = _seg_tasks(hc.three_segments(len(ridx)))
    qg = hc.make_gpair(case.n_rows)
    live = [(s, b, e, 0) for s, b, e in tasks if e > b]
    got, _ = _launch(gops, qg, ridx, live, 3, mode)
    assert np.array_equal(got, hc.ref_hist(case, qg, ridx, tasks, 3))


def _uneven_tasks(m):
    """Three slots: slot 0's rows in tasks of 1, 63, 1025 and the rest,
    slot 1 without rows, slot 2 in one task."""
    a = (3 * m) // 5
    assert a > 1089 and m > a
    return [(0, 0, 1), (0, 1, 64), (0, 64, 1089), (0, 1089, a), (2, a, m)]


_SUMS_CASES = [("H", 3), ("C", 1), ("A", 1), ("A", 3)]


@pytest.mark.parametrize("name,mode", _SUMS_CASES)
def test_hist_node_sums(name, mode):
    case = hc.geometry_case(name)
    gops = _gops(case, name)
    assert gops.use_shared >= mode
    ridx = hc.subset_ridx(case.n_rows)
    tasks = _uneven_tasks(len(ridx))
    qg = hc.make_gpair(case.n_rows)
    got, sums = _launch(gops, qg, ridx, [t + (0,) for t in tasks], 3, mode,
                        with_sums=True)
    want = hc.ref_node_sums(qg, ridx, tasks, 3)
    assert want[0].all() and want[2].all()
    assert np.array_equal(sums, want)
    assert not sums[1].any()
    assert np.array_equal(got, hc.ref_hist(case, qg, ridx, tasks, 3))


@pytest.mark.parametrize("layout", ["trailing", "interleaved"])
@pytest.mark.parametrize("name,mode", [("A", 3), ("C", 1), ("H", 3),
                                       ("A", 0)])
def test_hist_padded_tasks(name, mode, layout):
    case = hc.geometry_case(name)
    gops = _gops(case, name)
    ridx = hc.subset_ridx(case.n_rows)
    live = _uneven_tasks(len(ridx))
    pads = [(0, 0, 0, 0), (2, 5, 5, 0), (1, 5, 5, 0), (0, 0, 0, 0)]
    tasks = [t + (0,) for t in live]
    if layout == "trailing":
        tasks = tasks + pads
    else:
        mixed = [pads[0]]
        for i, t in enumerate(tasks):
            mixed += [t, pads[i % len(pads)]]
        tasks = mixed
    qg = hc.make_gpair(case.n_rows)
    got, sums = _launch(gops, qg, ridx, tasks, 3, mode, with_sums=True)
    assert np.array_equal(got, hc.ref_hist(case, qg, ridx, live, 3))
    assert np.array_equal(sums, hc.ref_node_sums(qg, ridx, live, 3))


def check_env_knobs():
    """Body of the child process in test_hist_env_knobs_child_process."""
    case = hc.geometry_case("A")
    gops = _gops(case, "A")
    ridx = hc.subset_ridx(case.n_rows)
    tasks = _uneven_tasks(len(ridx))
    qg = hc.make_gpair(case.n_rows)
    got, sums = _launch(gops, qg, ridx, [t + (0,) for t in tasks], 3,
                        gops.use_shared, with_sums=True)
    assert np.array_equal(got, hc.ref_hist(case, qg, ridx, tasks, 3))
    assert np.array_equal(sums, hc.ref_node_sums(qg, ridx, tasks, 3))
    return True


def test_hist_env_knobs_child_process():
    """GBT_HIST_BLOCK_SIZE and GBT_HIST_REG are read once per process:
    a single-wave block on the generic LDS kernel, in a fresh child."""
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "import test_gpu_hist as t; "
            "assert t.check_env_knobs(); print('knobs ok')"
            % (_ROOT, os.path.join(_ROOT, "tests")))
    env = dict(os.environ, GBT_HIST_BLOCK_SIZE="64", GBT_HIST_REG="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=_ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "knobs ok" in r.stdout, r.stdout + r.stderr


# ---- multi-target ---------------------------------------------------------

def _mt_setup(case, T, seed=20):
    gops = _gops(case)
    n = case.n_rows
    ridx = hc.subset_ridx(n)
    segs = hc.three_segments(len(ridx))
    gops.reset(n)
    gops.ridx = _dev(ridx)
    gops.segments = dict(enumerate(segs))
    qgs = [hc.make_gpair(n, seed=seed + t) for t in range(T)]
    ref = np.stack([hc.ref_hist(case, q, ridx, _seg_tasks(segs), 3)
                    for q in qgs])
    return gops, qgs, ref


def _mt_check(case, T, n_groups=None):
    from xgboost_amd.backend.gpu import (HIST_MAX_GROUP_FEATURES,
                                         LDS_MAX_GROUP_BINS)
    gops, qgs, ref = _mt_setup(case, T)
    grouping = gops._mt_grouping(T)
    assert grouping is not None
    fg, bg, ng, max_gb = grouping
    fg, bg = fg.cpu().numpy(), bg.cpu().numpy()
    assert ng == len(fg) - 1 == len(bg) - 1
    assert fg[0] == 0 and fg[-1] == len(case.widths)
    assert np.array_equal(bg, np.concatenate([[0], np.cumsum(
        case.widths)])[fg])
    assert (np.diff(fg) > 0).all()
    assert np.diff(fg).max() <= HIST_MAX_GROUP_FEATURES
    assert max_gb == np.diff(bg).max() and max_gb * T <= LDS_MAX_GROUP_BINS
    if n_groups is not None:
        assert ng == n_groups
    qg_mt = _dev(np.stack(qgs, axis=1))
    assert qg_mt.shape == (case.n_rows, T, 2)
    got = gops.build_hist_nodes_mt(qg_mt, [0, 1, 2])
    torch.cuda.synchronize()
    assert got is not None
    assert np.array_equal(got.cpu().numpy(), ref)
    return fg


@pytest.mark.parametrize("T", [1, 2, 3, 8])
def test_hist_mt_geometry_a(T):
    _mt_check(hc.geometry_case("A"), T, n_groups=1)


def test_hist_mt_several_groups():
    # T = 3: 2730 bins per group, ten 256-bin features each
    _mt_check(hc.make_case([256] * 20, 0.0, 3000, seed=31), 3, n_groups=2)


def test_hist_mt_16bit_missing():
    case = hc.geometry_case("G")
    assert case.qm.gidx.dtype == torch.int16
    _mt_check(case, 2, n_groups=2)


def test_hist_mt_feature_fills_budget():
    # T = 8: one feature of exactly 8192 / 8 bins still fits
    fg = _mt_check(hc.make_case([16, 1024, 16], 0.1, 3000, seed=32), 8)
    assert list(fg) == [0, 1, 2, 3]


def test_hist_mt_feature_over_budget_falls_back():
    case = hc.make_case([16, 1025, 16], 0.1, 3000, seed=33)
    gops, qgs, ref = _mt_setup(case, 8)
    assert gops._mt_grouping(8) is None
    assert gops.build_hist_nodes_mt(_dev(np.stack(qgs, axis=1)),
                                    [0, 1, 2]) is None
    # what the grower does instead: one single-target launch per target
    loop = torch.stack([gops.build_hist_nodes(_dev(q), [0, 1, 2])
                        for q in qgs])
    torch.cuda.synchronize()
    assert np.array_equal(loop.cpu().numpy(), ref)


def test_hist_mt_many_narrow_features():
    """1100 features x 3 bins fit one group by bins (3300 <= 4096) but
    not the 1024 features a block stages metadata for: the grouping must
    break on the feature count as well."""
    fg = _mt_check(hc.make_case([3] * 1100, 0.0, 3000, seed=34), 2)
    assert list(fg) == [0, 1024, 1100]


# ---- bin dtype guard ------------------------------------------------------

def test_gpu_ops_rejects_int32_bins():
    from xgboost_amd.backend.gpu import GpuOps
    case = hc.make_case([70000, 5], 0.1, 50, seed=3)
    assert case.qm.gidx.dtype == torch.int32
    with pytest.raises(ValueError, match="65535"):
        GpuOps(case.qm.to("cuda"))
    gops = _gops(hc.geometry_case("A", n=50))
    with pytest.raises(ValueError, match="65535"):
        gops.swap_gidx(case.qm.gidx.cuda())
