"""Whole-tree grow chain: the ballot-based partition kernel against a
numpy model, the device-written root task list against ChunkTasks, and
the native chain (direct enqueue, graph capture, graph replay) against
the Python GPU driver.  Everything is int64 / fp64 exact, so every
comparison is equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from xgboost_amd.backend.cpu import GradQuantizer
from xgboost_amd.data import DMatrix
from xgboost_amd.params import make_train_param

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# partition kernel vs numpy

_N_ROWS = 40000
_N_FEAT = 5
# kernel paths by task size: <= 1024 rows (4 register tiles per wave),
# <= 4096 (16 tiles), larger (re-gather)
_FALLBACK_ROWS = 5000


def _chunks(slot, begin, end, step):
    out = []
    b = begin
    while b < end:
        e = min(b + step, end)
        out.append((slot, b, e, 0))
        b = e
    return out


def _partition_case(bin_dtype, with_col, with_cat):
    """Build one multi-node launch; returns the kernel inputs and, per
    node, the expected left / right row multisets."""
    rng = np.random.RandomState(5)
    # feature f has fbins[f] real bins; value fbins[f] marks missing
    fbins = (np.array([300, 270, 17, 64, 33], np.int32)
             if bin_dtype == np.uint16
             else np.array([255, 200, 17, 64, 33], np.int32))
    gidx = np.empty((_N_ROWS, _N_FEAT), bin_dtype)
    for f in range(_N_FEAT):
        col = rng.randint(0, fbins[f], _N_ROWS)
        col[rng.rand(_N_ROWS) < 0.15] = fbins[f]  # missing
        gidx[:, f] = col
    ridx = rng.permutation(_N_ROWS).astype(np.int32)

    # (rows, task rows, feature, split bin, default_left, categorical)
    nodes = [
        (1, 1024, 0, 120, 0, False),
        (63, 1024, 1, 90, 1, False),
        (64, 1024, 2, 8, 0, False),
        (65, 1024, 3, 30, 1, False),
        (1025, 1024, 4, 16, 0, False),
        (3000, 4096, 0, 100, 1, False),            # 16-tile path
        (_FALLBACK_ROWS, 8192, 1, 150, 0, False),  # re-gather path
        (4100, 1024, 2, 16, 1, False),   # all left: every bin and missing
        (4100, 1024, 3, -1, 0, False),   # all right
        (20000, 1024, 0, 60, 0, False),
        (2000, 1024, 4, -1, 1, with_cat),
    ]
    feat = np.array([n[2] for n in nodes], np.int32)
    sbin = np.array([n[3] for n in nodes], np.int32)
    dleft = np.array([n[4] for n in nodes], np.uint8)
    cat_off = np.zeros(len(nodes) + 1, np.int32)
    cat_words = []
    counters = np.empty((len(nodes), 2), np.int32)
    tasks = [(0, 0, 0, 0)]  # a padded empty task first
    expect = []
    begin = 7  # rows before / between / after the segments stay untouched
    for j, (rows, step, f, sb, dl, is_cat) in enumerate(nodes):
        end = begin + rows
        counters[j] = (begin, end)
        tasks += _chunks(j, begin, end, step)
        seg_rows = ridx[begin:end]
        local = gidx[seg_rows, f].astype(np.int64)
        if is_cat:
            right_set = rng.rand(fbins[f]) < 0.5
            nw = (int(fbins[f]) + 31) // 32
            w = np.zeros(nw, np.uint32)
            for c in np.nonzero(right_set)[0]:
                w[c >> 5] |= np.uint32(1 << (c & 31))
            cat_words.append(w)
            cat_off[j + 1] = cat_off[j] + nw
            present_left = ~right_set[np.minimum(local, fbins[f] - 1)]
        else:
            cat_off[j + 1] = cat_off[j]
            present_left = local <= sb
        left = np.where(local >= fbins[f], bool(dl), present_left)
        expect.append((begin, end, np.sort(seg_rows[left]),
                       np.sort(seg_rows[~left])))
        begin = end + 3
    assert begin <= _N_ROWS
    tasks.append((0, 0, 0, 0))
    cat_bits = (np.concatenate(cat_words).view(np.int32)
                if cat_words else None)
    return dict(gidx=gidx, ridx=ridx, fbins=fbins, feat=feat, sbin=sbin,
                dleft=dleft, counters=counters,
                tasks=np.array(tasks, np.int32), expect=expect,
                cat_bits=cat_bits, cat_off=cat_off if cat_words else None,
                with_col=with_col)


@pytest.mark.parametrize("bin_dtype,with_col,with_cat", [
    (np.uint8, True, True), (np.uint8, False, False),
    (np.uint16, True, False), (np.uint16, False, True)])
def test_partition_matches_numpy_model(bin_dtype, with_col, with_cat):
    from xgboost_amd import ops
    lib = ops.load()
    c = _partition_case(bin_dtype, with_col, with_cat)
    dev = torch.device("cuda")

    def up(a):
        return None if a is None else torch.from_numpy(a).to(dev)

    if bin_dtype == np.uint16:
        # torch has no uint16 on every build: ship the bytes as int16
        gidx = up(c["gidx"].view(np.int16))
    else:
        gidx = up(c["gidx"])
    col = gidx.t().contiguous() if with_col else None
    g8 = bin_dtype == np.uint8
    ridx_in = up(c["ridx"])
    ridx_out = torch.full((_N_ROWS,), -1, dtype=torch.int32, device=dev)
    tasks, feat, sbin, dleft = (up(c[k]) for k in
                                ("tasks", "feat", "sbin", "dleft"))
    cnt = up(c["counters"])
    cat_bits, cat_off = up(c["cat_bits"]), up(c["cat_off"])
    fbins = up(c["fbins"])
    lib.gbt_partition(
        ops.ptr(gidx) if g8 else None, None if g8 else ops.ptr(gidx),
        _N_FEAT,
        ops.ptr(col) if (g8 and with_col) else None,
        ops.ptr(col) if (not g8 and with_col) else None,
        _N_ROWS if with_col else 0,
        ops.ptr(ridx_in), ops.ptr(ridx_out), ops.ptr(tasks), len(c["tasks"]),
        ops.ptr(feat), ops.ptr(sbin), ops.ptr(dleft), ops.ptr(cat_bits),
        ops.ptr(cat_off), ops.ptr(fbins), ops.ptr(cnt), ops.stream())
    torch.cuda.synchronize()
    out = ridx_out.cpu().numpy()
    final = cnt.cpu().numpy()
    touched = np.zeros(_N_ROWS, bool)
    for j, (b, e, left, right) in enumerate(c["expect"]):
        split = b + len(left)
        assert final[j, 0] == split and final[j, 1] == split, (j, final[j])
        assert np.array_equal(np.sort(out[b:split]), left), j
        assert np.array_equal(np.sort(out[split:e]), right), j
        touched[b:e] = True
    assert np.all(out[~touched] == -1), "wrote outside the task segments"


@pytest.mark.parametrize("n_rows,min_rows,target", [
    (0, 2048, 256), (1, 2048, 256), (2048, 2048, 256), (2049, 2048, 256),
    (5000, 2048, 64), (10007, 16, 64), (10007, 16, 7)])
def test_root_tasks_match_chunk_tasks(n_rows, min_rows, target):
    from xgboost_amd import ops
    lib = ops.load()
    assert lib.gbt_root_tasks_check(n_rows, min_rows, target,
                                    ops.stream()) == 0


# ---------------------------------------------------------------------------
# whole chain vs the python GPU driver

_TREE_FIELDS = ("left", "right", "split_index", "split_cond", "default_left",
                "loss_chg", "sum_hess", "base_weight")


def _chain_data(n, f=10, seed=11):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, f).astype(np.float32)
    X[rng.rand(n, f) < 0.05] = np.nan
    return X


def _gpair(n, seed):
    rng = np.random.RandomState(seed)
    g = rng.randn(n).astype(np.float32)
    h = rng.rand(n).astype(np.float32) + 0.1
    return torch.tensor(np.stack([g, h], axis=1))


def _gpair_step(n, seed):
    """Gradients that are a step in feature 0 plus small noise: the root
    split gains orders of magnitude more than any later one."""
    x0 = np.nan_to_num(_chain_data(n)[:, 0])
    rng = np.random.RandomState(seed)
    g = (np.where(x0 > 0, 1.0, -1.0)
         + 0.01 * rng.randn(n)).astype(np.float32)
    h = np.ones(n, np.float32)
    return torch.tensor(np.stack([g, h], axis=1))


def check_chain(n, params, seeds=(3, 4, 5), make_gpair=_gpair, monotone=None,
                per_level=False):
    """Grow one tree per seed with the native chain on ONE GpuOps (call 1
    enqueues directly, call 2 captures the graph, call 3 replays it) and
    compare each with the python driver's tree on a fresh GpuOps.

    monotone: int8 constraint per feature for both drivers, or None.
    per_level: hand the native side a quantizer without its device
    max-abs, so gbt_grow_tree takes its per-level mode at any depth (the
    host scales remain)."""
    from xgboost_amd.backend.gpu import GpuOps
    from xgboost_amd.grower import TreeGrower
    from xgboost_amd.tree_model import RegTree
    X = _chain_data(n)
    qm = DMatrix(X).quantized(64)
    param = make_train_param(params)
    gops = GpuOps(qm.to("cuda"))
    n_split = []
    for call, seed in enumerate(seeds):
        gpair = make_gpair(n, seed).cuda()
        quant = GradQuantizer(gpair)
        if per_level:
            del quant.maxabs_dev
        qg = quant.quantize(gpair)
        rs = qg.to(torch.int64).sum(dim=0).contiguous()
        res = gops.grow_tree_native(qg, RegTree(X.shape[1]), param, quant,
                                    monotone, rs)
        assert res is not None, "native driver refused a supported config"
        t_native, pos_native = res
        pos_native = pos_native.clone()

        gops_py = GpuOps(qm.to("cuda"))
        quant_py = GradQuantizer(gpair)
        grower = TreeGrower(gops_py, param, quant_py, n, monotone=monotone)
        t_py, pos_py = grower._grow(quant_py.quantize(gpair),
                                    RegTree(X.shape[1]))
        torch.cuda.synchronize()
        k = t_py.n_nodes
        assert t_native.n_nodes == k, (call, t_native.n_nodes, k)
        for name in _TREE_FIELDS:
            a = np.asarray(getattr(t_native, name)[:k])
            b = np.asarray(getattr(t_py, name)[:k])
            assert np.array_equal(a, b), (call, name)
        assert torch.equal(pos_native.cpu(), pos_py.cpu()), call
        n_split.append(int((np.asarray(t_py.left[:k]) >= 0).sum()))
    return n_split


def test_chain_depth2():
    assert min(check_chain(10007, {"max_depth": 2})) == 3


def test_chain_depth6():
    assert min(check_chain(10007, {"max_depth": 6, "reg_lambda": 1.2,
                                   "min_child_weight": 2.0})) > 31


def test_chain_nodes_stop_early():
    # a child below 2 * min_child_weight hessian cannot split: the tree
    # stays well short of the 63 splits a full depth-6 tree has
    n_split = check_chain(10007, {"max_depth": 6,
                                  "min_child_weight": 400.0})
    assert all(3 <= s < 31 for s in n_split), n_split


_MONOTONE = np.array([1, -1] * 5, np.int8)  # every feature constrained


def test_per_level_depth2():
    # root eval sync, one partition level, the final-level leaf decide
    assert min(check_chain(10007, {"max_depth": 2}, per_level=True)) >= 3


def test_per_level_depth6():
    # device sibling choice, pair sums on device
    assert min(check_chain(10007, {"max_depth": 6, "reg_lambda": 1.2,
                                   "min_child_weight": 2.0},
                           per_level=True)) >= 3


def test_per_level_nodes_stop_early():
    # leaves at both ping-pong parities: the two-parity leaf sweep
    n_split = check_chain(10007, {"max_depth": 6,
                                  "min_child_weight": 400.0},
                          per_level=True)
    assert all(3 <= s < 31 for s in n_split), n_split


def test_per_level_monotone():
    # host sibling choice by hessian, staged sums and bounds
    assert min(check_chain(10007, {"max_depth": 6}, monotone=_MONOTONE,
                           per_level=True)) >= 3


def test_chain_monotone_exact():
    # ApplyKernel's bound propagation against the python driver's
    assert min(check_chain(10007, {"max_depth": 6},
                           monotone=_MONOTONE)) >= 3


def test_chain_depth1():
    # below the whole-tree gate: the root goes straight to leaf decide
    assert check_chain(10007, {"max_depth": 1}) == [1, 1, 1]


def test_chain_depth13_no_arena():
    # too deep for the whole-tree arena: per-level mode without one
    n_split = check_chain(10007, {"max_depth": 13,
                                  "min_child_weight": 400.0})
    assert all(s >= 3 for s in n_split), n_split


def test_chain_children_do_not_split():
    # gamma admits the root split only: every later kernel sees count 0
    X = _chain_data(10007)
    qm = DMatrix(X).quantized(64)
    from xgboost_amd.backend.gpu import GpuOps
    from xgboost_amd.grower import TreeGrower
    from xgboost_amd.tree_model import RegTree
    gains = []
    for seed in (3, 4, 5):
        gpair = _gpair_step(10007, seed).cuda()
        quant = GradQuantizer(gpair)
        t, _ = TreeGrower(GpuOps(qm.to("cuda")),
                          make_train_param({"max_depth": 2}), quant,
                          10007)._grow(quant.quantize(gpair), RegTree(10))
        g = np.asarray(t.loss_chg[:t.n_nodes], np.float64)
        gains.append((g[0], g[1:].max()))
    lo = max(g[1] for g in gains)
    hi = min(g[0] for g in gains)
    assert lo < hi, "root gain does not dominate the children's"
    gamma = 0.5 * (lo + hi)
    assert check_chain(10007, {"max_depth": 6, "gamma": gamma},
                       make_gpair=_gpair_step) == [1, 1, 1]


def test_chain_multi_task_root_child_process():
    """GBT_HIST_TASKS is read once per process: a 64-task target at
    n = 5000 gives a 3-task root list, run in a child."""
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "import test_gpu_chain as t; "
            "assert t.check_chain(5000, {'max_depth': 2}) == [3, 3, 3]; "
            "print('chain ok')" % (_ROOT, os.path.join(_ROOT, "tests")))
    env = dict(os.environ, GBT_HIST_TASKS="64")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=_ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "chain ok" in r.stdout, r.stdout + r.stderr

