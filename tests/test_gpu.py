"""GPU kernel tests: every HIP kernel is cross-checked against the
torch/numpy CPU oracle (reference analog: tests/cpp/tree/gpu_hist/*).

The int64 fixed-point design means histogram, partition counts and
split sums must match the CPU oracle EXACTLY (not approximately)."""
import numpy as np
import pytest
import torch

import xgboost_amd as xgb
from xgboost_amd.backend.cpu import CpuOps, GradQuantizer
from xgboost_amd.data import DMatrix, quantize_dense
from xgboost_amd.params import make_train_param
from xgboost_amd.quantile import make_cuts

pytestmark = pytest.mark.gpu


def _data(n=5000, f=12, seed=0, missing_frac=0.0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, f).astype(np.float32)
    if missing_frac > 0:
        X[rng.rand(n, f) < missing_frac] = np.nan
    w = rng.randn(f)
    y = (np.nansum(X * w, axis=1) > 0).astype(np.float32)
    return X, y


def _gpair(n, seed=1):
    rng = np.random.RandomState(seed)
    g = rng.randn(n).astype(np.float32)
    h = (rng.rand(n).astype(np.float32) + 0.1)
    return torch.tensor(np.stack([g, h], axis=1))


def _gpu_ops(X, max_bin=64):
    from xgboost_amd.backend.gpu import GpuOps
    d = DMatrix(X)
    qm = d.quantized(max_bin)
    return GpuOps(qm.to("cuda")), CpuOps(qm), d


def test_native_lib_loads():
    from xgboost_amd import ops
    lib = ops.load()
    assert lib is not None


def test_compress_matches_cpu():
    from xgboost_amd import ops as hip_ops
    lib = hip_ops.load()
    X, _ = _data(2000, 8, missing_frac=0.1)
    cuts = make_cuts(X, 64)
    qm_cpu = quantize_dense(X, cuts)
    dev = torch.device("cuda")
    Xd = torch.from_numpy(X).to(dev)
    out = torch.empty((2000, 8), dtype=torch.uint8, device=dev)
    cut_vals = torch.from_numpy(cuts.values).to(dev)
    cut_ptrs = torch.from_numpy(cuts.ptrs.astype(np.int32)).to(dev)
    lib.gbt_compress(hip_ops.ptr(Xd), 2000, 8, hip_ops.ptr(cut_vals),
                     hip_ops.ptr(cut_ptrs), None, 0.0, 1,
                     hip_ops.ptr(out), None, hip_ops.stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), qm_cpu.gidx.numpy())


def test_hist_matches_cpu_exactly():
    X, y = _data(20000, 12)
    gops, cops, d = _gpu_ops(X)
    gpair = _gpair(20000)
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair)
    n = X.shape[0]
    segs = [(0, n // 3), (n // 3, n)]
    h_cpu = cops.build_hist(qg, cops.make_ridx(n), segs)
    h_gpu = gops.build_hist(qg.cuda(), gops.make_ridx(n), segs)
    torch.cuda.synchronize()
    assert torch.equal(h_cpu, h_gpu.cpu())


def test_hist_shared_vs_global():
    X, y = _data(8000, 10)
    gops, cops, d = _gpu_ops(X)
    gpair = _gpair(8000)
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair).cuda()
    ridx = gops.make_ridx(8000)
    h1 = gops.build_hist(qg, ridx, [(0, 8000)])
    gops.use_shared = 0
    h2 = gops.build_hist(qg, ridx, [(0, 8000)])
    gops.use_shared = 1
    torch.cuda.synchronize()
    assert torch.equal(h1, h2)


def test_hist_with_missing():
    X, y = _data(10000, 8, missing_frac=0.15)
    gops, cops, d = _gpu_ops(X)
    gpair = _gpair(10000)
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair)
    n = X.shape[0]
    h_cpu = cops.build_hist(qg, cops.make_ridx(n), [(0, n)])
    h_gpu = gops.build_hist(qg.cuda(), gops.make_ridx(n), [(0, n)])
    torch.cuda.synchronize()
    assert torch.equal(h_cpu, h_gpu.cpu())


def test_evaluate_matches_cpu():
    X, y = _data(20000, 12)
    gops, cops, d = _gpu_ops(X, max_bin=128)
    gpair = _gpair(20000)
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair)
    n = X.shape[0]
    segs = [(0, n // 2), (n // 2, n)]
    hist = cops.build_hist(qg, cops.make_ridx(n), segs)
    sums = [(int(hist[i, :, 0].sum() // 12), 0) for i in range(2)]
    # parent sums: exact per-node totals (hist double counts per feature)
    s0 = qg[:n // 2].to(torch.int64).sum(0)
    s1 = qg[n // 2:].to(torch.int64).sum(0)
    parents = [(int(s0[0]), int(s0[1])), (int(s1[0]), int(s1[1]))]
    param = make_train_param({"max_depth": 6, "reg_lambda": 1.5,
                              "alpha": 0.3, "min_child_weight": 2.0})
    cpu_e = cops.evaluate_splits(hist, quant, parents, [0, 1], param)
    gpu_e = gops.evaluate_splits(hist.cuda(), quant, parents, [0, 1], param)
    torch.cuda.synchronize()
    for ce, ge in zip(cpu_e, gpu_e):
        assert ce.feature == ge.feature, (ce, ge)
        assert ce.split_bin == ge.split_bin
        assert ce.default_left == ge.default_left
        assert ce.left_gq == ge.left_gq
        assert ce.left_hq == ge.left_hq
        assert ce.gain == pytest.approx(ge.gain, rel=1e-12)


def test_evaluate_with_monotone_and_mask():
    X, y = _data(10000, 6)
    gops, cops, d = _gpu_ops(X, max_bin=64)
    gpair = _gpair(10000)
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair)
    n = X.shape[0]
    hist = cops.build_hist(qg, cops.make_ridx(n), [(0, n)])
    s = qg.to(torch.int64).sum(0)
    parents = [(int(s[0]), int(s[1]))]
    param = make_train_param({"max_depth": 6})
    mono = np.array([1, -1, 0, 0, 0, 0], np.int64)
    fsets = [np.array([0, 1, 2, 3])]
    bounds = np.array([[-2.0, 2.0]])
    cpu_e = cops.evaluate_splits(hist, quant, parents, [0], param,
                                 feature_sets=fsets, monotone=mono,
                                 node_bounds=bounds)
    gpu_e = gops.evaluate_splits(hist.cuda(), quant, parents, [0], param,
                                 feature_sets=fsets, monotone=mono,
                                 node_bounds=bounds)
    torch.cuda.synchronize()
    ce, ge = cpu_e[0], gpu_e[0]
    assert ce.feature == ge.feature and ce.split_bin == ge.split_bin
    assert ge.feature in (0, 1, 2, 3)
    assert ce.gain == pytest.approx(ge.gain, rel=1e-12)


def test_partition_matches_cpu():
    X, y = _data(30000, 8)
    gops, cops, d = _gpu_ops(X)
    gpair = _gpair(30000)
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair)
    n = X.shape[0]
    hist = cops.build_hist(qg, cops.make_ridx(n), [(0, n)])
    s = qg.to(torch.int64).sum(0)
    param = make_train_param({"max_depth": 6})
    splits = cops.evaluate_splits(hist, quant, [(int(s[0]), int(s[1]))],
                                  [0], param)
    ridx_c = cops.make_ridx(n)
    segs_c = cops.partition(ridx_c, [(0, n)], splits)
    ridx_g = gops.make_ridx(n)
    segs_g = gops.partition(ridx_g, [(0, n)], splits)
    torch.cuda.synchronize()
    assert segs_c == segs_g  # same left/right counts
    (ls, le), (rs, re) = segs_g[0]
    left_gpu = set(ridx_g[ls:le].cpu().numpy().tolist())
    left_cpu = set(ridx_c[ls:le].numpy().tolist())
    assert left_gpu == left_cpu  # same membership (order may differ)


def test_gpu_training_matches_cpu_trees():
    X, y = _data(20000, 10)
    params = {"objective": "binary:logistic", "max_depth": 5, "eta": 0.3,
              "max_bin": 128}
    d1 = xgb.DMatrix(X, label=y)
    bst_cpu = xgb.train(dict(params, device="cpu"), d1, 5, verbose_eval=False)
    d2 = xgb.DMatrix(X, label=y)
    bst_gpu = xgb.train(dict(params, device="cuda"), d2, 5, verbose_eval=False)
    for tc, tg in zip(bst_cpu.trees, bst_gpu.trees):
        assert tc.n_nodes == tg.n_nodes
        assert np.array_equal(tc.split_index[:tc.n_nodes],
                              tg.split_index[:tg.n_nodes])
        assert np.array_equal(tc.left[:tc.n_nodes], tg.left[:tg.n_nodes])
        # leaf values: last-ulp fp32 drift is expected (torch sigmoid on
        # CPU vs GPU differs by 1 ulp -> quantized gradients shift by 1
        # in later iterations); structure must still match exactly.
        assert np.allclose(tc.split_cond[:tc.n_nodes],
                           tg.split_cond[:tg.n_nodes], rtol=1e-4, atol=1e-6)
    p_cpu = bst_cpu.predict(d1)
    p_gpu = bst_gpu.predict(d2)
    assert np.allclose(p_cpu, p_gpu, atol=1e-4)


def test_gpu_predict_matches_cpu():
    X, y = _data(5000, 8)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 6},
                    d, 8, verbose_eval=False)
    p_cpu = bst.predict(d)
    bst.set_param("device", "cuda")
    bst.reset()
    p_gpu = bst.predict(d)
    assert np.allclose(p_cpu, p_gpu, atol=1e-6)


def test_gpu_training_with_missing():
    X, y = _data(20000, 10, missing_frac=0.2)
    d = xgb.DMatrix(X, label=y)
    res = {}
    xgb.train({"objective": "binary:logistic", "max_depth": 5,
               "device": "cuda"}, d, 10, evals=[(d, "train")],
              evals_result=res, verbose_eval=False)
    assert res["train"]["logloss"][-1] < 0.45


def test_gpu_multiclass():
    rng = np.random.RandomState(0)
    X = rng.randn(10000, 8).astype(np.float32)
    w = rng.randn(8, 3)
    y = (X @ w).argmax(axis=1).astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "multi:softprob", "num_class": 3,
                     "device": "cuda", "max_depth": 4}, d, 8,
                    verbose_eval=False)
    p = bst.predict(d)
    assert (p.argmax(axis=1) == y).mean() > 0.8


def test_gpu_e2e_quality():
    X, y = _data(100000, 28, seed=3)
    d = xgb.DMatrix(X, label=y)
    res = {}
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 8,
                     "max_bin": 256, "device": "cuda", "eta": 0.2,
                     "eval_metric": "auc"}, d, 20, evals=[(d, "train")],
                    evals_result=res, verbose_eval=False)
    assert res["train"]["auc"][-1] > 0.9


def _shap_device_only(monkeypatch):
    """The host SHAP recursion raises while the block runs, so a silent
    fallback from the device fails the test."""
    import shap_cases
    from xgboost_amd import shap
    return shap_cases.host_recursion_raises(monkeypatch, shap)


def test_gpu_shap_matches_cpu(monkeypatch):
    from xgboost_amd.shap import shap_values
    X, y = _data(500, 8)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 5},
                    d, 5, verbose_eval=False)
    cpu_contribs = bst.predict(d, pred_contribs=True)
    bst.set_param("device", "cuda")
    bst.reset()
    with _shap_device_only(monkeypatch):
        gpu_contribs = bst.predict(d, pred_contribs=True)
    assert gpu_contribs.shape == cpu_contribs.shape
    assert np.allclose(cpu_contribs, gpu_contribs, atol=1e-4), \
        np.abs(cpu_contribs - gpu_contribs).max()
    # efficiency: contribs sum to margin
    margin = bst.predict(d, output_margin=True)
    assert np.allclose(gpu_contribs.sum(axis=1), margin, atol=1e-3)


def test_gpu_shap_with_missing(monkeypatch):
    from xgboost_amd.shap import shap_values
    X, y = _data(300, 6, missing_frac=0.2)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 4,
                     "device": "cuda"}, d, 4, verbose_eval=False)
    with _shap_device_only(monkeypatch):
        contribs = bst.predict(d, pred_contribs=True)
    margin = bst.predict(d, output_margin=True)
    assert np.allclose(contribs.sum(axis=1), margin, atol=1e-3)


def test_device_data_ingestion():
    X, y = _data(20000, 10)
    Xd = torch.from_numpy(X).cuda()
    d_dev = xgb.DMatrix(Xd, label=y)
    assert d_dev.num_row() == 20000
    res = {}
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 5,
                     "device": "cuda", "eval_metric": "auc"}, d_dev, 10,
                    evals=[(d_dev, "t")], evals_result=res,
                    verbose_eval=False)
    assert res["t"]["auc"][-1] > 0.9
    # compare with host ingestion (same data): quality must match closely
    d_host = xgb.DMatrix(X, label=y)
    res2 = {}
    xgb.train({"objective": "binary:logistic", "max_depth": 5,
               "device": "cuda", "eval_metric": "auc"}, d_host, 10,
              evals=[(d_host, "t")], evals_result=res2, verbose_eval=False)
    assert abs(res["t"]["auc"][-1] - res2["t"]["auc"][-1]) < 0.02
    # inplace predict from a device tensor
    p = bst.inplace_predict(Xd)
    assert p.shape == (20000,)


def test_native_driver_matches_python_driver():
    """The C++ level-loop driver (driver.hip) must produce the same tree
    as the Python GPU driver (same kernels, same host math)."""
    from xgboost_amd.backend.gpu import GpuOps
    from xgboost_amd.grower import TreeGrower
    from xgboost_amd.tree_model import RegTree
    X, y = _data(30000, 10, seed=11)
    d = DMatrix(X)
    qm = d.quantized(128)
    gpair = _gpair(30000, seed=3).cuda()
    quant = GradQuantizer(gpair)
    qg = quant.quantize(gpair)
    param = make_train_param({"max_depth": 6, "reg_lambda": 1.2,
                              "min_child_weight": 2.0})

    gops = GpuOps(qm.to("cuda"))
    grower = TreeGrower(gops, param, quant, 30000)
    t_native = RegTree(10)
    rs = qg.to(torch.int64).sum(dim=0).contiguous()  # device-resident
    res = gops.grow_tree_native(qg, t_native, param, quant, None, rs)
    assert res is not None, "native driver refused a supported config"
    t_native, pos_native = res

    # force the python driver (fresh ops to reset state)
    gops2 = GpuOps(qm.to("cuda"))
    grower2 = TreeGrower(gops2, param, quant, 30000)
    t_py = RegTree(10)
    t_py, pos_py = grower2._grow(qg, t_py)
    # finalize leaves of native path like _grow does (native already did)
    torch.cuda.synchronize()
    assert t_native.n_nodes == t_py.n_nodes
    assert np.array_equal(t_native.left[:t_py.n_nodes],
                          t_py.left[:t_py.n_nodes])
    assert np.array_equal(t_native.split_index[:t_py.n_nodes],
                          t_py.split_index[:t_py.n_nodes])
    assert np.allclose(t_native.split_cond[:t_py.n_nodes],
                       t_py.split_cond[:t_py.n_nodes], rtol=1e-6)
    assert np.allclose(t_native.sum_hess[:t_py.n_nodes],
                       t_py.sum_hess[:t_py.n_nodes], rtol=1e-5)
    # same leaf assignment for every row
    assert torch.equal(pos_native.cpu(), pos_py.cpu())


def test_native_driver_with_monotone():
    X = np.random.RandomState(0).rand(20000, 3).astype(np.float32)
    y = (X[:, 0] + 0.1 * np.random.RandomState(1).randn(20000)).astype(
        np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 5,
                     "device": "cuda", "monotone_constraints": [1, 0, 0],
                     "eta": 0.5}, d, 10, verbose_eval=False)
    grid = np.linspace(0.01, 0.99, 50, dtype=np.float32)
    Xq = np.stack([grid, np.full_like(grid, 0.5),
                   np.full_like(grid, 0.5)], axis=1)
    p = bst.predict(xgb.DMatrix(Xq))
    assert np.all(np.diff(p) >= -1e-5)


def test_fused_gpair_path_matches_torch():
    """The fused gradient+quantize kernel must reproduce the torch
    gradient chain (same trees up to fp ulp ties, same quality)."""
    from xgboost_amd.core import Booster
    X, y = _data(30000, 10, seed=21)
    params = {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3,
              "device": "cuda", "eval_metric": "auc"}
    d1 = xgb.DMatrix(X, label=y)
    res1 = {}
    b1 = xgb.train(params, d1, 10, evals=[(d1, "t")], evals_result=res1,
                   verbose_eval=False)
    assert hasattr(b1, "_fused_cache"), "fused path was not taken"
    # disable fused path via unsupported option (subsample) for reference
    d2 = xgb.DMatrix(X, label=y)
    res2 = {}
    b2 = xgb.train(dict(params, subsample=0.9999999), d2, 10,
                   evals=[(d2, "t")], evals_result=res2, verbose_eval=False)
    assert abs(res1["t"]["auc"][-1] - res2["t"]["auc"][-1]) < 0.01
    # weights exercised through the kernel
    w = np.random.RandomState(0).rand(30000).astype(np.float32) + 0.5
    d3 = xgb.DMatrix(X, label=y, weight=w)
    res3 = {}
    xgb.train(params, d3, 5, evals=[(d3, "t")], evals_result=res3,
              verbose_eval=False)
    assert res3["t"]["auc"][-1] > 0.9


def test_mt_gpu_eval_matches_cpu():
    """Vector-leaf trees: the MT evaluation kernel must agree with the
    numpy multi-target evaluator."""
    rng = np.random.RandomState(0)
    X = rng.randn(20000, 8).astype(np.float32)
    W = rng.randn(8, 3)
    Y = (X @ W + 0.1 * rng.randn(20000, 3)).astype(np.float32)
    params = {"objective": "reg:squarederror", "max_depth": 5,
              "multi_strategy": "multi_output_tree", "eta": 0.3,
              "max_bin": 128}
    b_cpu = xgb.train(dict(params, device="cpu"),
                      xgb.DMatrix(X, label=Y), 5, verbose_eval=False)
    b_gpu = xgb.train(dict(params, device="cuda"),
                      xgb.DMatrix(X, label=Y), 5, verbose_eval=False)
    for tc, tg in zip(b_cpu.trees, b_gpu.trees):
        assert tc.n_nodes == tg.n_nodes
        assert np.array_equal(tc.split_index[:tc.n_nodes],
                              tg.split_index[:tg.n_nodes])
        assert np.allclose(tc.leaf_values[:tc.n_nodes],
                           tg.leaf_values[:tg.n_nodes], rtol=1e-4, atol=1e-5)
    p1 = b_cpu.predict(xgb.DMatrix(X))
    p2 = b_gpu.predict(xgb.DMatrix(X))
    assert np.allclose(p1, p2, atol=1e-4)


def test_extmem_streamed_pages():
    """Force the beyond-HBM streaming path (_StreamedPage) and verify
    it trains identically to the device-cached path."""
    from xgboost_amd.extmem import DataIter, ExtMemQuantileDMatrix, ExtMemOps
    from xgboost_amd.core import Booster

    class It(DataIter):
        def __init__(self):
            super().__init__()
            self.i = 0

        def reset(self):
            self.i = 0

        def next(self, input_data):
            if self.i >= 3:
                return False
            rng = np.random.RandomState(self.i)
            Xb = rng.randn(5000, 8).astype(np.float32)
            yb = (Xb[:, 0] > 0).astype(np.float32)
            input_data(data=Xb, label=yb)
            self.i += 1
            return True

    d1 = ExtMemQuantileDMatrix(It(), max_bin=64)
    b1 = Booster({"objective": "binary:logistic", "max_depth": 4,
                  "device": "cuda", "max_bin": 64}, cache=[d1])
    # force every page through the streamed path (budget 0)
    b1._ops_cache[id(d1)] = ExtMemOps(d1, torch.device("cuda"),
                                      device_cache_bytes=0)
    from xgboost_amd.extmem import _StreamedPage
    assert all(isinstance(p, _StreamedPage)
               for p in b1._ops_cache[id(d1)].page_ops)
    for i in range(5):
        b1.update(d1, i)
    d2 = ExtMemQuantileDMatrix(It(), max_bin=64)
    b2 = Booster({"objective": "binary:logistic", "max_depth": 4,
                  "device": "cuda", "max_bin": 64}, cache=[d2])
    for i in range(5):
        b2.update(d2, i)
    for t1, t2 in zip(b1.trees, b2.trees):
        assert t1.n_nodes == t2.n_nodes
        assert np.array_equal(t1.split_index[:t1.n_nodes],
                              t2.split_index[:t2.n_nodes])


def test_gpu_lossguide_matches_cpu():
    """Python GPU driver path (lossguide heap growth is not in the
    native driver) must produce the same trees as the CPU oracle."""
    X, y = _data(20000, 8, seed=21)
    dg = xgb.DMatrix(X, label=y)
    dc = xgb.DMatrix(X, label=y)
    pg = {"objective": "binary:logistic", "grow_policy": "lossguide",
          "max_leaves": 24, "max_depth": 0, "max_bin": 64, "seed": 5}
    bg = xgb.train({**pg, "device": "cuda"}, dg, 8)
    bc = xgb.train(pg, dc, 8)
    for tg, tc in zip(bg.trees, bc.trees):
        assert tg.n_nodes == tc.n_nodes
        assert np.array_equal(tg.split_index[:tg.n_nodes],
                              tc.split_index[:tc.n_nodes])
        assert np.array_equal(tg.left[:tg.n_nodes], tc.left[:tc.n_nodes])


def test_gpu_colsample_matches_cpu():
    """Column sampling forces the python driver with per-node feature
    masks staged into the eval kernel; identical seeds must give
    identical trees on CPU and GPU."""
    X, y = _data(15000, 10, seed=22)
    dg = xgb.DMatrix(X, label=y)
    dc = xgb.DMatrix(X, label=y)
    p = {"objective": "binary:logistic", "max_depth": 5, "max_bin": 64,
         "colsample_bytree": 0.7, "colsample_bynode": 0.8, "seed": 3}
    bg = xgb.train({**p, "device": "cuda"}, dg, 6)
    bc = xgb.train(p, dc, 6)
    for tg, tc in zip(bg.trees, bc.trees):
        assert tg.n_nodes == tc.n_nodes
        assert np.array_equal(tg.split_index[:tg.n_nodes],
                              tc.split_index[:tc.n_nodes])


def test_native_driver_distributed_branch_rccl_world1():
    """Initialize a 1-rank RCCL process group so the native driver takes
    its DISTRIBUTED branch (global-hessian sibling choice, host-staged
    eval sums, allreduce callback into torch.distributed) — the exact
    code the multi-GPU scaling run exercises — and check the trees
    equal the non-distributed CPU oracle."""
    import os
    import torch.distributed as dist
    from xgboost_amd import collective

    X, y = _data(20000, 8, seed=31)
    # two configs: full-expansion depth 6, and depth 8 with gamma so some
    # levels only partially expand (exercises the padded fixed-count
    # hist/pair-sum allreduces of the distributed WHOLE-TREE chain)
    param_sets = [
        {"objective": "binary:logistic", "max_depth": 6, "max_bin": 64,
         "seed": 2},
        {"objective": "binary:logistic", "max_depth": 8, "max_bin": 128,
         "gamma": 0.5, "seed": 2},
    ]
    refs = [xgb.train(pd, xgb.DMatrix(X, label=y), 6) for pd in param_sets]

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29771")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        assert collective.is_distributed()
        for pd, bc in zip(param_sets, refs):
            dg = xgb.DMatrix(X, label=y)
            bg = xgb.train({**pd, "device": "cuda"}, dg, 6)
            for tg, tc in zip(bg.trees, bc.trees):
                assert tg.n_nodes == tc.n_nodes
                assert np.array_equal(tg.split_index[:tg.n_nodes],
                                      tc.split_index[:tc.n_nodes])
                assert np.array_equal(tg.left[:tg.n_nodes],
                                      tc.left[:tc.n_nodes])
    finally:
        dist.destroy_process_group()


def test_gpu_categorical_matches_cpu():
    """Categorical splits force the python driver with bitset partition
    args (partition.hip DecideLeft cat path) and one-hot/sorted split
    evaluation; CPU and GPU must agree exactly."""
    rng = np.random.RandomState(7)
    n = 12000
    Xc = rng.randint(0, 12, size=(n, 2)).astype(np.float32)
    Xn = rng.randn(n, 3).astype(np.float32)
    X = np.concatenate([Xc, Xn], axis=1)
    logits = (np.isin(Xc[:, 0], [1, 4, 7]) * 2.0 - 1.0) + 0.5 * Xn[:, 0]
    y = (logits + 0.3 * rng.randn(n) > 0).astype(np.float32)
    ft = ["c", "c", "q", "q", "q"]
    # onehot=4 -> sorted-partition subsets; onehot=32 -> in-kernel one-hot
    for onehot in (4, 32):
        params = {"objective": "binary:logistic", "max_depth": 5,
                  "max_bin": 64, "max_cat_to_onehot": onehot, "seed": 0}
        dg = xgb.DMatrix(X, label=y, feature_types=ft)
        dc = xgb.DMatrix(X, label=y, feature_types=ft)
        bg = xgb.train({**params, "device": "cuda"}, dg, 6)
        bc = xgb.train(params, dc, 6)
        used_cat = False
        for tg, tc in zip(bg.trees, bc.trees):
            assert tg.n_nodes == tc.n_nodes, f"onehot={onehot}"
            assert np.array_equal(tg.split_index[:tg.n_nodes],
                                  tc.split_index[:tc.n_nodes])
            assert np.array_equal(tg.left[:tg.n_nodes],
                                  tc.left[:tc.n_nodes])
            used_cat = used_cat or any(
                tg.split_index[i] < 2 and tg.left[i] >= 0
                for i in range(tg.n_nodes))
        assert used_cat, "categorical feature never used - test is vacuous"
        # prediction parity on the categorical model
        pg = bg.predict(dg)
        pc = bc.predict(dc)
        np.testing.assert_allclose(pg, pc, atol=2e-6)


def test_gpu_approx_matches_cpu():
    """tree_method=approx re-sketches with hessian weights each
    iteration; cuts come from the same host sketch, so CPU and GPU
    trees must still agree exactly."""
    X, y = _data(8000, 6, seed=13)
    params = {"objective": "binary:logistic", "tree_method": "approx",
              "max_depth": 4, "max_bin": 64, "seed": 0}
    bc = xgb.train(params, xgb.DMatrix(X, label=y), 5)
    bg = xgb.train({**params, "device": "cuda"},
                   xgb.DMatrix(X, label=y), 5)
    for tc, tg in zip(bc.trees, bg.trees):
        assert tc.n_nodes == tg.n_nodes
        assert np.array_equal(tc.split_index[:tc.n_nodes],
                              tg.split_index[:tg.n_nodes])


def test_gpu_shap_multiclass_matches_cpu(monkeypatch):
    """Path-table SHAP with n_groups > 1: per-group bias and the
    transposed phi indexing must match the CPU oracle."""
    rng = np.random.RandomState(17)
    X = rng.randn(3000, 6).astype(np.float32)
    y = np.abs(X[:, :3]).argmax(axis=1).astype(np.float32)
    params = {"objective": "multi:softprob", "num_class": 3,
              "max_depth": 4, "max_bin": 64, "seed": 0}
    dc = xgb.DMatrix(X, label=y)
    bc = xgb.train(params, dc, 4)
    ref = bc.predict(dc, pred_contribs=True)
    dg = xgb.DMatrix(X, label=y)
    bg = xgb.train({**params, "device": "cuda"}, dg, 4)
    with _shap_device_only(monkeypatch):
        got = bg.predict(dg, pred_contribs=True)
    assert got.shape == ref.shape == (3000, 3, 7)
    np.testing.assert_allclose(got, ref, atol=5e-4, rtol=1e-3)


def test_native_driver_monotone_whole_tree_matches_cpu_trees():
    """Monotone configs used to force the per-level sync driver; the
    whole-tree chain now propagates fp64 weight bounds inside
    ApplyKernel (device) and the host replay — trees must still match
    the CPU oracle exactly."""
    X, y = _data(30000, 6, seed=13)
    pd = {"objective": "reg:squarederror", "max_depth": 8, "max_bin": 128,
          "monotone_constraints": [1, -1, 0, 0, 1, 0], "eta": 0.4}
    bc = xgb.train(pd, xgb.DMatrix(X, label=y), 8)
    bg = xgb.train({**pd, "device": "cuda"}, xgb.DMatrix(X, label=y), 8)
    assert len(bg.trees) == len(bc.trees)
    for tg, tc in zip(bg.trees, bc.trees):
        assert tg.n_nodes == tc.n_nodes
        assert np.array_equal(tg.split_index[:tg.n_nodes],
                              tc.split_index[:tc.n_nodes])
        assert np.array_equal(tg.left[:tg.n_nodes], tc.left[:tc.n_nodes])
        assert np.allclose(tg.split_cond[:tg.n_nodes],
                           tc.split_cond[:tc.n_nodes], rtol=1e-6)


def test_gpu_lambdarank_device_gradients():
    """rank:ndcg gradients computed on-device (vectorized segmented
    sort/cumsum lambdarank, reference lambdarank_obj.cu) and trained
    through the GPU hist path."""
    rng = np.random.RandomState(17)
    n = 5000
    X = rng.randn(n, 6).astype(np.float32)
    y = np.clip((X[:, 0] + X[:, 1] + 2).astype(int), 0, 4).astype(np.float32)
    qid = np.repeat(np.arange(50), n // 50)
    d = xgb.DMatrix(X, label=y, qid=qid)
    bst = xgb.train({"objective": "rank:ndcg", "max_depth": 4, "eta": 0.3,
                     "device": "cuda"}, d, 15, verbose_eval=False)
    res = bst.eval_set([(d, "train")], 14)
    ndcg = float(res.split(":")[-1])
    assert ndcg > 0.93, res
    # MAP objective exercises the n_rel/acc segmented statistics
    yb = (X[:, 0] > 0).astype(np.float32)
    d2 = xgb.DMatrix(X, label=yb, qid=qid)
    bst2 = xgb.train({"objective": "rank:map", "max_depth": 4, "eta": 0.3,
                      "device": "cuda"}, d2, 10, verbose_eval=False)
    res2 = bst2.eval_set([(d2, "train")], 9)
    assert float(res2.split(":")[-1]) > 0.8, res2


def test_gpu_shap_interactions_matches_cpu(monkeypatch):
    """pred_interactions on GPU (shap_ix.hip) vs the exact CPU
    conditional TreeSHAP."""
    from xgboost_amd.shap import shap_interactions
    X, y = _data(800, 6, seed=23, missing_frac=0.05)
    d = xgb.DMatrix(X, label=y)
    bst_c = xgb.train({"objective": "binary:logistic", "max_depth": 5,
                       "eta": 0.3}, d, 8, verbose_eval=False)
    ref = shap_interactions(bst_c, d)
    dg = xgb.DMatrix(X, label=y)
    bst_g = xgb.train({"objective": "binary:logistic", "max_depth": 5,
                       "eta": 0.3, "device": "cuda"}, dg, 8,
                      verbose_eval=False)
    # same data/params -> identical trees (tested elsewhere); compare
    # the GPU interactions of the GPU model vs CPU interactions of it
    bst_g.device = bst_g.device  # noqa: B018
    with _shap_device_only(monkeypatch):
        got = shap_interactions(bst_g, dg)
    cpu_of_g = None
    import torch as _t
    dev = bst_g.device
    try:
        bst_g.device = _t.device("cpu")
        cpu_of_g = shap_interactions(bst_g, dg)
    finally:
        bst_g.device = dev
    assert got.shape == cpu_of_g.shape
    assert np.allclose(got, cpu_of_g, atol=2e-4), np.abs(
        got.astype(np.float64) - cpu_of_g.astype(np.float64)).max()
    # row sums reproduce the margin (SHAP completeness)
    margin = bst_g.predict(dg, output_margin=True)
    total = got.sum(axis=(1, 2))
    assert np.allclose(total, margin, atol=1e-3)
    del ref


def test_gpu_inplace_predict_device_resident():
    """inplace_predict on a cuda tensor: zero-copy proxy straight into
    the HIP predict kernel, forest SoA cached across calls."""
    X, y = _data(20000, 8, seed=41)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "binary:logistic", "max_depth": 6,
                     "device": "cuda"}, d, 10, verbose_eval=False)
    ref = bst.predict(xgb.DMatrix(X))
    Xd = torch.from_numpy(X).cuda()
    got = bst.inplace_predict(Xd)
    assert np.allclose(got, ref, atol=1e-6)
    # repeated call reuses the cached device forest (same object)
    fc = bst.__dict__.get("_forest_dev_cache", {})
    assert len(fc) == 1
    fa0 = next(iter(fc.values()))
    got2 = bst.inplace_predict(Xd)
    assert next(iter(fc.values())) is fa0
    assert np.allclose(got2, ref, atol=1e-6)


def test_gpu_lossguide_native_replay_matches_python_gpu_driver():
    """lossguide / max_leaves on the native driver: depthwise chain +
    host policy replay must match the PYTHON GPU lossguide driver
    node-for-node.  (The GPU python driver is the right oracle: its
    heap keys are the same fp64 gains the native records carry.  A
    CPU-trained tree is NOT node-comparable for lossguide: CPU and GPU
    gains agree only to ~1e-12 relative, and the lossguide POP ORDER
    is sensitive to last-ulp differences — depthwise expansion is not.)
    """
    from xgboost_amd.grower import TreeGrower
    X, y = _data(30000, 8, seed=19)
    for params in (
        {"grow_policy": "lossguide", "max_depth": 8, "max_leaves": 31},
        {"grow_policy": "lossguide", "max_depth": 6, "max_leaves": 0},
        {"grow_policy": "depthwise", "max_depth": 7, "max_leaves": 40},
        {"grow_policy": "lossguide", "max_depth": 8, "max_leaves": 31,
         "monotone_constraints": [1, 0, 0, 0, -1, 0, 0, 0]},
    ):
        pd = {"objective": "binary:logistic", "eta": 0.3, "max_bin": 128,
              "device": "cuda", **params}
        bg = xgb.train(pd, xgb.DMatrix(X, label=y), 5)  # native + replay
        orig = TreeGrower._try_native
        TreeGrower._try_native = lambda self, qg, t: None
        try:
            bp = xgb.train(pd, xgb.DMatrix(X, label=y), 5)  # python driver
        finally:
            TreeGrower._try_native = orig
        for tg, tc in zip(bg.trees, bp.trees):
            assert tg.n_nodes == tc.n_nodes, params
            assert np.array_equal(tg.split_index[:tg.n_nodes],
                                  tc.split_index[:tc.n_nodes]), params
            assert np.array_equal(tg.left[:tg.n_nodes],
                                  tc.left[:tc.n_nodes]), params
            assert np.allclose(tg.split_cond[:tg.n_nodes],
                               tc.split_cond[:tc.n_nodes],
                               rtol=1e-6, atol=1e-7), params
        # and the CPU oracle agrees on QUALITY (training accuracy)
        bc = xgb.train({k: v for k, v in pd.items() if k != "device"},
                       xgb.DMatrix(X, label=y), 5)
        pg = bg.predict(xgb.DMatrix(X))
        pc = bc.predict(xgb.DMatrix(X))
        acc_g = (((pg > 0.5) == y).mean())
        acc_c = (((pc > 0.5) == y).mean())
        assert abs(acc_g - acc_c) < 0.02, (params, acc_g, acc_c)


def test_gpu_mt_hist_fused_matches_per_target_loop():
    """Fused multi-target histogram (gbt_hist_mt, one pass over the bin
    matrix) must equal T single-target launches exactly (int64)."""
    X, _ = _data(20000, 10)
    gops, cops, d = _gpu_ops(X, max_bin=64)
    T = 3
    qgpairs = []
    for t in range(T):
        gp = _gpair(20000, seed=40 + t)
        quant = GradQuantizer(gp)
        qgpairs.append(quant.quantize(gp).cuda())
    gops.reset(20000)
    n = 20000
    gops.segments = {0: (0, n // 2), 1: (n // 2, n)}
    qg_mt = torch.stack(qgpairs, dim=1).contiguous()
    fused = gops.build_hist_nodes_mt(qg_mt, [0, 1])
    assert fused is not None, "fused MT hist refused a supported shape"
    loop = torch.stack([gops.build_hist_nodes(qgpairs[t], [0, 1])
                        for t in range(T)])
    torch.cuda.synchronize()
    assert torch.equal(fused, loop)


def test_gpu_multi_target_training_quality():
    """multi_output_tree training on GPU (fused MT hist path)."""
    rng = np.random.RandomState(9)
    n = 20000
    X = rng.randn(n, 6).astype(np.float32)
    Y = np.stack([X[:, 0] + 0.1 * rng.randn(n),
                  X[:, 1] - X[:, 2] + 0.1 * rng.randn(n)],
                 axis=1).astype(np.float32)
    d = xgb.DMatrix(X, label=Y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 5,
                     "multi_strategy": "multi_output_tree",
                     "device": "cuda", "eta": 0.3}, d, 10,
                    verbose_eval=False)
    pred = bst.predict(xgb.DMatrix(X))
    rmse = float(np.sqrt(((pred - Y) ** 2).mean()))
    assert rmse < 0.4, rmse


def test_gpu_colsample_bytree_native_matches_python_driver():
    """colsample_bytree now runs on the native whole-tree driver with a
    broadcast feature mask; trees must match the Python GPU driver."""
    from xgboost_amd.grower import TreeGrower
    X, y = _data(30000, 12, seed=29)
    pd = {"objective": "binary:logistic", "max_depth": 7, "max_bin": 128,
          "colsample_bytree": 0.5, "seed": 11, "device": "cuda"}
    bg = xgb.train(pd, xgb.DMatrix(X, label=y), 6)
    orig = TreeGrower._try_native
    TreeGrower._try_native = lambda self, qg, t: None
    try:
        bp = xgb.train(pd, xgb.DMatrix(X, label=y), 6)
    finally:
        TreeGrower._try_native = orig
    used = set()
    for tg, tc in zip(bg.trees, bp.trees):
        assert tg.n_nodes == tc.n_nodes
        assert np.array_equal(tg.split_index[:tg.n_nodes],
                              tc.split_index[:tc.n_nodes])
        assert np.array_equal(tg.left[:tg.n_nodes], tc.left[:tc.n_nodes])
        used |= set(int(f) for i, f in enumerate(tg.split_index[:tg.n_nodes])
                    if tg.left[i] != -1)
    assert len(used) <= 12  # sanity; sampling varies per tree


def test_distributed_whole_tree_chain_vs_duplicated_data():
    """End-to-end check of the DISTRIBUTED whole-tree chain without
    multiple devices: patch the collectives to emulate world=2 with
    both ranks holding the SAME shard (allreduce-sum doubles buffers,
    max/broadcast are identity).  With reg_lambda=0, min_child_weight=0
    the doubled histograms must produce EXACTLY the tree that
    single-rank training on the row-duplicated dataset produces
    (int64 sums scale exactly by 2; gains scale uniformly; leaf values
    -2G/2H == -G/H).  This exercises the padded fixed-count hist and
    pair-sum reduces, the global-hessian sibling choice and the
    built-is-left records — the exact code the 8-GPU run drives."""
    import xgboost_amd.sketch as sketch_mod
    from xgboost_amd import collective as coll
    X, y = _data(20000, 8, seed=37)
    pd = {"objective": "binary:logistic", "max_depth": 8, "max_bin": 128,
          "reg_lambda": 0.0, "min_child_weight": 0.0, "seed": 2,
          "device": "cuda"}
    X2 = np.concatenate([X, X])
    y2 = np.concatenate([y, y])
    # both runs must bin with IDENTICAL cuts (the emulated world=2 would
    # otherwise take the summary-merge sketch while the reference run
    # takes the exact sort — different cut points, different trees)
    cuts_fixed = make_cuts(X, 128)
    saved_sketch = sketch_mod.sketch_cuts
    sketch_mod.sketch_cuts = lambda dmat, mb: cuts_fixed
    try:
        b_ref = xgb.train(pd, xgb.DMatrix(X2, label=y2), 6)
    finally:
        sketch_mod.sketch_cuts = saved_sketch

    saved = {k: getattr(coll, k) for k in
             ("is_distributed", "get_world_size", "get_rank",
              "allreduce_sum_", "allreduce_max_", "broadcast_obj",
              "allreduce_sum_scalars", "allreduce_max_scalars",
              "barrier", "allgather_obj")}
    try:
        coll.is_distributed = lambda: True
        coll.get_world_size = lambda: 2
        coll.get_rank = lambda: 0
        coll.allreduce_sum_ = lambda t: t.mul_(2)
        coll.allreduce_max_ = lambda t: t
        coll.broadcast_obj = lambda obj, src=0: obj
        coll.allreduce_sum_scalars = lambda v: [2 * x for x in v]
        coll.allreduce_max_scalars = lambda v: list(v)
        coll.barrier = lambda: None
        coll.allgather_obj = lambda obj: [obj, obj]
        sketch_mod.sketch_cuts = lambda dmat, mb: cuts_fixed
        b_dist = xgb.train(pd, xgb.DMatrix(X, label=y), 6)
    finally:
        sketch_mod.sketch_cuts = saved_sketch
        for k, v in saved.items():
            setattr(coll, k, v)
    assert len(b_dist.trees) == len(b_ref.trees)
    for td, tr in zip(b_dist.trees, b_ref.trees):
        assert td.n_nodes == tr.n_nodes
        assert np.array_equal(td.split_index[:td.n_nodes],
                              tr.split_index[:tr.n_nodes])
        assert np.array_equal(td.left[:td.n_nodes], tr.left[:tr.n_nodes])
        assert np.allclose(td.split_cond[:td.n_nodes],
                           tr.split_cond[:tr.n_nodes], rtol=1e-6, atol=1e-7)
        # doubled shard hessians == duplicated-data hessians directly
        assert np.allclose(td.sum_hess[:td.n_nodes],
                           tr.sum_hess[:tr.n_nodes], rtol=1e-5)


def test_gpu_u16_bins_training_matches_cpu():
    """max_bin > 256 stores u16 local bins — exercises the u16
    register-metadata hist kernel variant against the CPU oracle."""
    X, y = _data(30000, 6, seed=43)
    pd = {"objective": "binary:logistic", "max_depth": 6, "max_bin": 700,
          "eta": 0.3}
    bc = xgb.train(pd, xgb.DMatrix(X, label=y), 5)
    bg = xgb.train({**pd, "device": "cuda"}, xgb.DMatrix(X, label=y), 5)
    for tg, tc in zip(bg.trees, bc.trees):
        assert tg.n_nodes == tc.n_nodes
        assert np.array_equal(tg.split_index[:tg.n_nodes],
                              tc.split_index[:tc.n_nodes])
        assert np.array_equal(tg.left[:tg.n_nodes], tc.left[:tc.n_nodes])
        assert np.allclose(tg.split_cond[:tg.n_nodes],
                           tc.split_cond[:tc.n_nodes], rtol=1e-6)


def test_wt_graph_replay_matches_no_graph():
    """The hipGraph-captured whole-tree chain (driver.hip) must produce
    bit-identical models to the direct-enqueue chain (GBT_WT_GRAPH=0),
    including across rounds where the graph is REPLAYED."""
    import json
    import os
    import subprocess
    import sys
    import tempfile

    script = r"""
import json, sys
import numpy as np
import xgboost_amd as xgb
rng = np.random.RandomState(7)
X = rng.randn(60000, 12).astype(np.float32)
y = ((X[:, 0] * X[:, 1] + X[:, 2]) > 0).astype(np.float32)
d = xgb.DMatrix(X, label=y)
bst = xgb.train({"objective": "binary:logistic", "max_depth": 7,
                 "device": "cuda", "eta": 0.3}, d, 15)
out = {"dump": bst.get_dump(with_stats=True),
       "pred": bst.predict(d)[:512].tolist()}
json.dump(out, open(sys.argv[1], "w"))
"""
    outs = []
    with tempfile.TemporaryDirectory() as td:
        sp = os.path.join(td, "run.py")
        with open(sp, "w") as f:
            f.write(script)
        pkg_root = os.path.dirname(os.path.dirname(
            os.path.abspath(__import__("xgboost_amd").__file__)))
        for flag in ("1", "0"):
            env = dict(os.environ, GBT_WT_GRAPH=flag,
                       PYTHONPATH=pkg_root)
            of = os.path.join(td, f"out{flag}.json")
            subprocess.run([sys.executable, sp, of], check=True, env=env,
                           timeout=300, cwd=pkg_root)
            outs.append(json.load(open(of)))
    assert outs[0]["dump"] == outs[1]["dump"]
    assert outs[0]["pred"] == outs[1]["pred"]


def test_dart_on_device():
    """DART on cuda: dropped-tree contributions come from the subset
    forest predict (predict_subset_gpu) and weighted prediction folds
    weights into the cached forest's leaf values."""
    rng = np.random.RandomState(21)
    Xn = rng.randn(20000, 8).astype(np.float32)
    yn = (Xn[:, 0] * 1.2 - Xn[:, 1] + 0.1 * rng.randn(20000)).astype(
        np.float32)
    d = DMatrix(Xn, label=yn)
    bst = xgb.train({"max_depth": 4, "eta": 0.3, "device": "cuda",
                     "rate_drop": 0.4, "one_drop": True, "seed": 9},
                    d, 10)
    assert len(bst.weight_drop) == 10
    assert any(w != 1.0 for w in bst.weight_drop)
    cached, _ = bst._cache[id(d)]
    fresh = bst._predict_margin(d)
    assert torch.allclose(cached, fresh, atol=1e-3), \
        (cached - fresh).abs().max()
    # CPU reference: same params/seed on cpu must give the same trees
    bst_cpu = xgb.train({"max_depth": 4, "eta": 0.3, "device": "cpu",
                         "rate_drop": 0.4, "one_drop": True, "seed": 9},
                        d, 10)
    assert bst.weight_drop == pytest.approx(bst_cpu.weight_drop)
    pg = bst.predict(d)
    pc = bst_cpu.predict(d)
    assert np.allclose(pg, pc, atol=2e-3), np.abs(pg - pc).max()
