"""Feature slices of the register-metadata histogram kernel
(gbt_hist_sliced, hist.hip): every slice count builds the histogram and
the node sums of the plain reference in hist_cases.py, bit for bit, and
the drivers grow the same trees whatever slice count sizes their tasks.

Slice counts: 1 is the unsliced launch, 2 and 3 cut the load units
unevenly on most geometries, 4 is what the policy picks for the
benchmark shape, 64 is clamped to the load units of each group.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hist_cases as hc

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLICES = [1, 2, 3, 4, 64]
# A: 12 u8 features, 3 dwords; B: non-vector path; E: 32 x 256; F: missing
# sentinel; G: u16, 2 features per load; H: two LDS groups; M: uneven
# widths with width-1 features
SLICED_GEOMETRIES = ["A", "B", "E", "F", "G", "H", "M"]


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _gops(name, n=3000, seed=0, pattern="random"):
    """(case, GpuOps) of a geometry, after checking the launch mode the
    case is meant to run at."""
    from xgboost_amd.backend.gpu import GpuOps
    case = hc.geometry_case(name, n=n, seed=seed, pattern=pattern)
    gops = GpuOps(case.qm.to("cuda"))
    dtype, n_groups, mode = hc.GEOMETRIES[name][2:]
    assert gops.qm.gidx.dtype == dtype
    assert gops.n_groups == n_groups
    assert gops.use_shared == mode and mode >= 2
    return case, gops


def _launch(gops, qg, ridx, tasks, k, slices):
    """gbt_hist_sliced with node sums: (hist, sums) as numpy."""
    hip = gops.hip
    tasks_d = _dev(np.asarray(tasks, np.int32).reshape(-1, 4))
    qg_d, ridx_d = _dev(qg), _dev(ridx)
    out = torch.zeros((k, gops.n_bins, 2), dtype=torch.int64, device="cuda")
    sums = torch.zeros((k, 2), dtype=torch.int64, device="cuda")
    p8, p16 = gops._gidx_ptrs()
    gops.lib.gbt_hist_sliced(
        p8, p16, gops.qm.n_features, hip.ptr(qg_d), hip.ptr(ridx_d),
        hip.ptr(tasks_d), tasks_d.shape[0], hip.ptr(out), gops.n_bins,
        hip.ptr(gops.feat_group_start), hip.ptr(gops.bin_group_start),
        gops.n_groups, gops.max_group_bins, hip.ptr(gops.cut_ptrs),
        gops.use_shared, slices, hip.ptr(sums), hip.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), sums.cpu().numpy()


def _check(case, gops, qg, ridx, tasks, live, k, slices):
    """tasks: what is launched; live: the (slot, begin, end) the reference
    accumulates."""
    got, sums = _launch(gops, qg, ridx, tasks, k, slices)
    assert np.array_equal(got, _ref(case, qg, ridx, live, k)), slices
    assert np.array_equal(sums, hc.ref_node_sums(qg, ridx, live, k)), slices


_REFS = {}


def _ref(case, qg, ridx, live, k):
    key = (id(case), qg.tobytes()[:64], len(ridx), tuple(live), k)
    if key not in _REFS:
        ref = hc.ref_hist(case, qg, ridx, live, k)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


# ---- geometries, multi-slot tasks, node sums ------------------------------

@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("name", SLICED_GEOMETRIES)
def test_sliced_geometry_multi_slot(name, slices):
    """Three segments with their own out_slot, the middle one empty; the
    node sums are added once, not once per slice."""
    case, gops = _gops(name)
    ridx = hc.subset_ridx(case.n_rows)
    live = [(i, s, e) for i, (s, e) in
            enumerate(hc.three_segments(len(ridx)))]
    qg = hc.make_gpair(case.n_rows)
    want = hc.ref_node_sums(qg, ridx, live, 3)
    assert want[0].all() and want[2].all() and not want[1].any()
    _check(case, gops, qg, ridx, [t + (0,) for t in live if t[2] > t[1]],
           live, 3, slices)


# ---- row edges ------------------------------------------------------------

@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("n", [1, 65, 513, 2049])
@pytest.mark.parametrize("name", ["A", "G"])
def test_sliced_row_edges(name, n, slices):
    case, gops = _gops(name, n=n, seed=n)
    ridx = hc.subset_ridx(n, seed=n)
    m = len(ridx)
    _check(case, gops, hc.make_gpair(n, seed=n), ridx, [(0, 0, m, 0)],
           [(0, 0, m)], 1, slices)


# ---- padded task lists ----------------------------------------------------

def _uneven_tasks(m):
    """Three slots: slot 0 in tasks of 1, 63, 1025 rows and the rest,
    slot 1 without rows, slot 2 in one task."""
    a = (3 * m) // 5
    assert a > 1089 and m > a
    return [(0, 0, 1), (0, 1, 64), (0, 64, 1089), (0, 1089, a), (2, a, m)]


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("layout", ["trailing", "interleaved"])
@pytest.mark.parametrize("name", ["A", "H"])
def test_sliced_padded_tasks(name, layout, slices):
    """Empty tasks, as the device task generation pads its list with; 9
    and 11 tasks, so the launch grid is padded past the task list too."""
    case, gops = _gops(name)
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
    _check(case, gops, hc.make_gpair(case.n_rows), ridx, tasks, live, 3,
           slices)


# ---- value edges ----------------------------------------------------------

@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("kind", ["contention", "extremes"])
@pytest.mark.parametrize("name", ["M", "A"])
def test_sliced_value_edges(name, kind, slices):
    pattern = {"extremes": "random", "contention": "same"}[kind]
    case, gops = _gops(name, seed=7, pattern=pattern)
    n = case.n_rows
    qg = hc.make_gpair(n, seed=11, kind=kind)
    ridx = hc.subset_ridx(n, seed=5, frac=1.0)
    _check(case, gops, qg, ridx, [(0, 0, n, 0)], [(0, 0, n)], 1, slices)
    if kind == "contention":
        ref = _ref(case, qg, ridx, [(0, 0, n)], 1)
        assert np.count_nonzero(ref[0, :, 1]) == len(case.widths)


# ---- slice policy ---------------------------------------------------------

def test_slice_policy_clamps_and_defaults():
    """gbt_hist_slices(n_groups, features, bins, bytes per bin, mode):
    one slice for every kernel and shape class that was not measured, never
    more slices than the group has load units."""
    from xgboost_amd import ops
    pol = ops.load().gbt_hist_slices
    env = os.environ.get("GBT_HIST_SLICES")
    forced = int(env) if env and 1 <= int(env) <= 64 else 0
    bench = pol(1, 28, 7168, 1, 3)
    assert 1 <= bench <= 7
    if forced:
        assert bench == min(forced, 7)
        return
    assert pol(1, 28, 7168, 1, 1) == 1     # generic LDS kernel
    assert pol(1, 28, 7168, 1, 0) == 1     # global-atomic kernel
    assert pol(1, 28, 7168, 2, 3) == 1     # u16
    assert pol(2, 32, 8192, 1, 3) == 1     # several LDS groups
    assert pol(1, 12, 768, 1, 3) == 1      # small flush: not measured


# ---- task geometry in the drivers -----------------------------------------

_FIELDS = ("left", "right", "split_index", "split_cond", "default_left",
           "loss_chg", "sum_hess", "base_weight")


def train_child(out_path):
    """Body of the child processes of test_task_geometry_child_processes:
    3 rounds at depth 4 on a 5000 x 28 Higgs-like matrix."""
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(5000, 28).astype(np.float32)
    y = (X[:, 0] + X[:, 1] * X[:, 2] + 0.5 * rng.randn(5000) > 0) \
        .astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 4,
                     "max_bin": 256, "device": "cuda", "seed": 7}, d, 3,
                    verbose_eval=False)
    out = {"margin": np.asarray(bst.predict(d, output_margin=True))}
    for i, tree in enumerate(bst.trees):
        assert tree.n_nodes > 3
        for name in _FIELDS:
            out["t%d_%s" % (i, name)] = np.asarray(
                getattr(tree, name)[:tree.n_nodes])
    np.savez(out_path, **out)
    print("trained ok")


def test_task_geometry_child_processes(tmp_path):
    """GBT_HIST_SLICES is read once per process: the whole-tree chain with
    1 and with 4 slices, and the direct enqueue (GBT_WT_GRAPH=0), grow
    identical trees and margins."""
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "import test_gpu_hist_slices as t; t.train_child(sys.argv[1])"
            % (_ROOT, os.path.join(_ROOT, "tests")))
    runs = {"s1": {"GBT_HIST_SLICES": "1"}, "s4": {"GBT_HIST_SLICES": "4"},
            "s4_nograph": {"GBT_HIST_SLICES": "4", "GBT_WT_GRAPH": "0"}}
    procs = {k: subprocess.Popen(
        [sys.executable, "-c", code, str(tmp_path / (k + ".npz"))],
        env=dict(os.environ, **env), cwd=_ROOT, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True) for k, env in runs.items()}
    for k, p in procs.items():
        out, _ = p.communicate(timeout=120)
        assert p.returncode == 0 and "trained ok" in out, k + ": " + out
    want = np.load(tmp_path / "s1.npz")
    for k in ("s4", "s4_nograph"):
        got = np.load(tmp_path / (k + ".npz"))
        assert sorted(got.files) == sorted(want.files), k
        for f in want.files:
            assert got[f].dtype == want[f].dtype, (k, f)
            assert np.array_equal(got[f], want[f]), (k, f)
