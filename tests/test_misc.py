"""Callbacks, config context, UBJSON typed arrays, monitor, cv
(reference analog: tests/python/test_callback.py, test_config.py)."""
import io

import numpy as np
import pytest

import xgboost_amd as xgb
from xgboost_amd.callback import (EarlyStopping, EvaluationMonitor,
                                  LearningRateScheduler, TrainingCheckPoint)
from conftest import make_classification, make_regression


def test_config_context():
    from xgboost_amd.config import config_context, get_config, set_config
    assert get_config()["verbosity"] == 1
    with config_context(verbosity=3):
        assert get_config()["verbosity"] == 3
    assert get_config()["verbosity"] == 1
    with pytest.raises(ValueError):
        set_config(bogus=1)


def test_learning_rate_scheduler():
    X, y = make_regression(500, 4)
    d = xgb.DMatrix(X, label=y)
    rates = [0.5, 0.4, 0.3, 0.2, 0.1]
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 2}, d, 5,
                    callbacks=[LearningRateScheduler(rates)],
                    verbose_eval=False)
    assert bst.num_boosted_rounds() == 5


def test_checkpoint_callback(tmp_path):
    X, y = make_regression(300, 4)
    d = xgb.DMatrix(X, label=y)
    xgb.train({"objective": "reg:squarederror"}, d, 6,
              callbacks=[TrainingCheckPoint(directory=str(tmp_path),
                                            name="ckpt", interval=2)],
              verbose_eval=False)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert len(files) >= 2
    bst = xgb.Booster(model_file=str(tmp_path / files[0]))
    assert bst.num_features() == 4


def test_evaluation_monitor_output(capsys):
    X, y = make_classification(400, 4)
    d = xgb.DMatrix(X, label=y)
    xgb.train({"objective": "binary:logistic"}, d, 3,
              evals=[(d, "train")], verbose_eval=True)
    out = capsys.readouterr().out
    assert "train-logloss" in out
    assert "[0]" in out


def test_early_stopping_save_best():
    X, y = make_classification(1500, 6)
    dtrain = xgb.DMatrix(X[:1000], label=y[:1000])
    dvalid = xgb.DMatrix(X[1000:], label=y[1000:])
    es = EarlyStopping(rounds=3, save_best=True)
    bst = xgb.train({"objective": "binary:logistic", "eta": 0.5,
                     "max_depth": 6}, dtrain, 100,
                    evals=[(dvalid, "valid")], callbacks=[es],
                    verbose_eval=False)
    assert bst.num_boosted_rounds() == bst.best_iteration + 1


def test_cv_runs():
    X, y = make_classification(600, 5)
    d = xgb.DMatrix(X, label=y)
    res = xgb.cv({"objective": "binary:logistic", "max_depth": 3}, d,
                 num_boost_round=5, nfold=3, seed=1)
    cols = list(res.columns) if hasattr(res, "columns") else list(res)
    assert any("test-logloss-mean" in c for c in cols)
    n = len(res)
    assert n == 5


def test_cv_early_stopping():
    X, y = make_classification(600, 5)
    d = xgb.DMatrix(X, label=y)
    res = xgb.cv({"objective": "binary:logistic", "max_depth": 6,
                  "eta": 0.8}, d, num_boost_round=50, nfold=3,
                 early_stopping_rounds=3, seed=1)
    assert len(res) < 50


def test_ubjson_typed_array_roundtrip():
    """Reference UBJSON writers emit optimized typed arrays
    ([$<type>#<count>); our reader must parse them."""
    from xgboost_amd.ubjson import dumps_ubjson, loads_ubjson
    obj = {"a": np.array([1.5, 2.5], np.float32),
           "b": np.array([1, 2, 3], np.int64),
           "c": "text", "d": [1, True, None], "e": {"n": 7}}
    blob = dumps_ubjson(obj)
    back = loads_ubjson(blob)
    assert back["a"] == [1.5, 2.5]
    assert back["b"] == [1, 2, 3]
    assert back["c"] == "text"
    assert back["d"] == [1, True, None]
    assert back["e"] == {"n": 7}


def test_monitor_accumulates():
    from xgboost_amd.monitor import Monitor
    m = Monitor("test")
    m.start("phase")
    m.stop("phase")
    assert m.counts["phase"] == 1
    assert "phase" in m.report()


def test_validate_parameters():
    X, y = make_regression(100, 3)
    d = xgb.DMatrix(X, label=y)
    with pytest.raises(ValueError):
        xgb.train({"objective": "reg:squarederror", "typo_param": 1,
                   "validate_parameters": True}, d, 1, verbose_eval=False)
    # without validation: accepted silently (reference warns)
    xgb.train({"objective": "reg:squarederror", "typo_param": 1}, d, 1,
              verbose_eval=False)


def test_seed_per_iteration():
    X, y = make_classification(800, 5)
    d = xgb.DMatrix(X, label=y)
    p = {"objective": "binary:logistic", "subsample": 0.7,
         "seed_per_iteration": True, "seed": 3}
    b1 = xgb.train(p, d, 3, verbose_eval=False)
    d2 = xgb.DMatrix(X, label=y)
    b2 = xgb.train(p, d2, 3, verbose_eval=False)
    assert np.array_equal(b1.predict(d), b2.predict(d2))


def test_category_recode_between_frames():
    """Predict-frame category dictionaries are re-coded to the training
    dictionary (reference src/encoder/ordinal.h Recode)."""
    import pandas as pd
    rng = np.random.RandomState(0)
    n = 1000
    colors = rng.choice(["red", "green", "blue"], n)
    df = pd.DataFrame({"color": pd.Categorical(colors),
                       "x": rng.randn(n).astype(np.float32)})
    y = ((colors == "red") * 2.0).astype(np.float32)
    d = xgb.DMatrix(df, label=y, enable_categorical=True)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 3}, d, 5,
                    verbose_eval=False)
    p_train = bst.predict(d)
    # same data, shuffled category order
    df2 = df.copy()
    df2["color"] = pd.Categorical(colors, categories=["blue", "red", "green"])
    d2 = xgb.DMatrix(df2, label=y, enable_categorical=True)
    assert np.allclose(bst.predict(d2), p_train, atol=1e-6)
    # unseen category behaves as missing (no crash, finite output)
    df3 = pd.DataFrame({
        "color": pd.Categorical(["purple"] * 4,
                                categories=["purple", "red"]),
        "x": np.zeros(4, np.float32)})
    d3 = xgb.DMatrix(df3, label=np.zeros(4), enable_categorical=True)
    assert np.isfinite(bst.predict(d3)).all()


def test_cv_fpreproc_and_dict_result():
    import numpy as np
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(200, 4).astype(np.float32)
    y = (X[:, 0] > 0).astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    seen = []

    def fpreproc(dtr, dte, params):
        # reference-style hook: rescale a param per fold
        seen.append(dtr.num_row())
        params["eta"] = 0.1
        return dtr, dte, params

    res = xgb.cv({"objective": "binary:logistic", "max_depth": 2},
                 d, num_boost_round=3, nfold=4, fpreproc=fpreproc,
                 as_pandas=False, seed=1)
    assert len(seen) == 4
    assert isinstance(res, dict)
    assert len(res["test-logloss-mean"]) == 3


def test_feature_weights_bias_column_sampling():
    import numpy as np
    import xgboost_amd as xgb
    rng = np.random.RandomState(3)
    X = rng.randn(500, 6).astype(np.float32)
    y = (X[:, 5] + 0.05 * rng.randn(500)).astype(np.float32)
    # weight 0 on the informative feature -> it can never be sampled
    fw = np.ones(6, dtype=np.float32)
    fw[5] = 0.0
    d = xgb.DMatrix(X, label=y, feature_weights=fw)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 3,
                     "colsample_bynode": 0.5, "seed": 7}, d, 10)
    score = bst.get_score(importance_type="weight")
    assert "f5" not in score and len(score) > 0
    # weight heavily toward f5 -> it is used
    fw2 = np.full(6, 1e-6, dtype=np.float32)
    fw2[5] = 1.0
    d2 = xgb.DMatrix(X, label=y, feature_weights=fw2)
    bst2 = xgb.train({"objective": "reg:squarederror", "max_depth": 3,
                      "colsample_bynode": 0.5, "seed": 7}, d2, 10)
    assert "f5" in bst2.get_score(importance_type="weight")
    # validation
    import pytest
    with pytest.raises(ValueError):
        xgb.DMatrix(X, label=y, feature_weights=np.ones(3))


def test_public_api_surface_matches_reference():
    """Every name in the reference package's __all__ resolves here
    (reference python-package/xgboost/__init__.py)."""
    import xgboost_amd as m
    ref_all = ["Booster", "DMatrix", "DataIter", "ExtMemQuantileDMatrix",
               "QuantileDMatrix", "RabitTracker", "XGBClassifier",
               "XGBModel", "XGBRFClassifier", "XGBRFRegressor",
               "XGBRanker", "XGBRegressor", "build_info", "collective",
               "config_context", "cv", "get_config", "interpret",
               "plot_importance", "plot_tree", "set_config", "to_graphviz",
               "train"]
    for name in ref_all:
        assert getattr(m, name, None) is not None, name


def test_interpret_shap_values_split():
    import numpy as np
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(300, 5).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1]).astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 3}, d, 8)
    values, bias = xgb.interpret.shap_values(bst, X)
    assert values.shape == (300, 5)
    margin = bst.predict(d, output_margin=True)
    np.testing.assert_allclose(values.sum(axis=1) + bias, margin, atol=1e-4)


def test_rabit_tracker_rendezvous():
    import xgboost_amd as xgb
    t = xgb.RabitTracker(n_workers=2)
    t.start()
    args = t.worker_args()
    assert args["MASTER_ADDR"] == "127.0.0.1"
    assert args["WORLD_SIZE"] == 2
    assert args["MASTER_PORT"] == args["DMLC_TRACKER_PORT"]
    # wait_for now genuinely blocks on worker completion (reference
    # XGTrackerWaitFor); with no workers it must time out, not no-op
    import pytest as _pytest
    with _pytest.raises(TimeoutError):
        t.wait_for(timeout=1)
    t.free()


def test_dmatrix_info_accessors():
    import numpy as np
    from scipy import sparse as sp
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(50, 4).astype(np.float32)
    X[2, 1] = np.nan
    y = rng.rand(50).astype(np.float32)
    w = rng.rand(50).astype(np.float32)
    d = xgb.DMatrix(X, label=y, weight=w)
    assert np.allclose(d.get_float_info("label"), y)
    assert np.allclose(d.get_float_info("weight"), w)
    d.set_float_info("base_margin", np.zeros(50, np.float32))
    assert d.get_float_info("base_margin").shape == (50,)
    assert d.num_nonmissing() == 50 * 4 - 1
    csr = d.get_data()
    assert sp.issparse(csr) and csr.shape == (50, 4)
    assert csr.nnz == 50 * 4 - 1
    # quantile cuts
    d.quantized(32)
    indptr, values = d.get_quantile_cut()
    assert indptr.shape == (5,) and values.shape[0] == int(indptr[-1])
    # group accessors
    dq = xgb.DMatrix(X, label=y, qid=np.repeat(np.arange(5), 10))
    assert np.array_equal(dq.get_group(), np.full(5, 10))
    assert dq.get_uint_info("group_ptr").shape == (6,)


def test_booster_load_config_roundtrip():
    import numpy as np
    import xgboost_amd as xgb
    rng = np.random.RandomState(1)
    X = rng.randn(100, 3).astype(np.float32)
    y = X[:, 0].astype(np.float32)
    d = xgb.DMatrix(X, label=y)
    bst = xgb.train({"objective": "reg:squarederror", "max_depth": 4,
                     "eta": 0.21}, d, 2)
    cfg = bst.save_config()
    bst2 = xgb.Booster({"objective": "reg:squarederror"}, cache=[d])
    bst2.load_config(cfg)
    import json
    c2 = json.loads(bst2.save_config())
    tp = c2["learner"]["gradient_booster"]["tree_train_param"]
    assert float(tp["eta"]) == 0.21
    assert int(tp["max_depth"]) == 4


def test_bench_contract_cpu():
    """bench.py must run standalone (no flags -> N=1 quick run) and
    print one JSON line with the driver-contract fields."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"),
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=300, cwd=repo)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    blob = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in blob, key
    assert blob["metric"] == "boosting_rounds_per_sec"
    assert blob["scaling"] == "weak"
    assert blob["data"] == "synthetic"


def test_base_score_estimation_boost_from_average():
    """reference test_intercept.py: with no base_score given, the
    intercept is fitted from the labels (one Newton step), and a
    0-round model predicts it."""
    import numpy as np
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(500, 3).astype(np.float32)
    y = (rng.rand(500) < 0.25).astype(np.float32)  # 25% positives
    d = xgb.DMatrix(X, label=y)
    # estimation happens at the first boost (reference: lazy configure
    # + FitStump); the fitted intercept lands in base_score
    bst = xgb.train({"objective": "binary:logistic", "eta": 0.0}, d, 1)
    # ONE Newton step at margin 0 (reference FitStump): sigmoid(4(m-.5))
    expect = 1.0 / (1.0 + np.exp(-4.0 * (y.mean() - 0.5)))
    np.testing.assert_allclose(bst.base_score, expect, rtol=1e-3)
    # explicit base_score wins
    bst2 = xgb.train({"objective": "binary:logistic", "base_score": 0.5,
                      "eta": 0.0}, xgb.DMatrix(X, label=y), 1)
    np.testing.assert_allclose(bst2.base_score, 0.5, atol=1e-6)
    # regression: mean label
    yr = (X[:, 0] * 2 + 5).astype(np.float32)
    bst3 = xgb.train({"objective": "reg:squarederror", "eta": 0.0},
                     xgb.DMatrix(X, label=yr), 1)
    np.testing.assert_allclose(bst3.base_score, yr.mean(), rtol=1e-3)


def test_early_stopping_last_dataset_last_metric():
    """reference semantics: without explicit names, early stopping
    watches the LAST metric on the LAST eval set."""
    import numpy as np
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(600, 4).astype(np.float32)
    y = (X[:, 0] > 0).astype(np.float32)
    Xv = rng.randn(300, 4).astype(np.float32)
    yv = (rng.rand(300) > 0.5).astype(np.float32)  # pure noise valid
    res = {}
    bst = xgb.train({"objective": "binary:logistic",
                     "eval_metric": ["logloss", "auc"], "max_depth": 3},
                    xgb.DMatrix(X, label=y), 60,
                    evals=[(xgb.DMatrix(X, label=y), "train"),
                           (xgb.DMatrix(Xv, label=yv), "valid")],
                    early_stopping_rounds=5, evals_result=res,
                    verbose_eval=False)
    # stopped early on noise validation AUC (maximize inferred)
    assert bst.best_iteration is not None
    assert len(res["valid"]["auc"]) < 60
    assert "logloss" in res["valid"] and "auc" in res["valid"]


def test_training_observer(capfd, monkeypatch):
    """TrainingObserver (reference src/common/observer.h): env-gated
    per-iteration gradient/tree/prediction dumps."""
    import numpy as np
    import xgboost_amd as xgb
    from xgboost_amd.monitor import TrainingObserver
    monkeypatch.setenv("XGB_AMD_OBSERVER", "1")
    TrainingObserver._enabled = None  # re-read env
    try:
        rng = np.random.RandomState(0)
        X = rng.randn(300, 4).astype(np.float32)
        y = (X[:, 0] > 0).astype(np.float32)
        xgb.train({"objective": "binary:logistic", "max_depth": 3},
                  xgb.DMatrix(X, label=y), 2, verbose_eval=False)
    finally:
        TrainingObserver._enabled = None
        monkeypatch.delenv("XGB_AMD_OBSERVER")
    out, _ = capfd.readouterr()
    assert "[observer]" in out
    assert "grad:" in out and "tree:" in out and "margin:" in out
    TrainingObserver._enabled = None


def test_bench_contract_cpu():
    """bench.py is the driver's contract: default flags must finish
    quickly and print one JSON line with the required fields."""
    import json
    import os
    import subprocess
    import sys
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1"],
        capture_output=True, timeout=300,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr.decode()
    line = out.stdout.decode().strip().splitlines()[-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
              "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"] == "boosting_rounds_per_sec"
    assert d["config"]["parallelism"] == "dp1"


def test_testing_module_generators():
    """xgboost_amd.testing: offline analogs of the reference's public
    testing data helpers, usable end-to-end."""
    import xgboost_amd as xgb
    from xgboost_amd import testing as tm

    X, y = tm.make_regression(400, 6, seed=1)
    bst = xgb.train({"max_depth": 3}, xgb.DMatrix(X, label=y), 5)
    assert np.corrcoef(bst.predict(xgb.DMatrix(X)), y)[0, 1] > 0.7

    Xc, yc = tm.make_classification(400, 6, n_classes=3, seed=2)
    bst = xgb.train({"objective": "multi:softmax", "num_class": 3,
                     "max_depth": 3}, xgb.DMatrix(Xc, label=yc), 5)
    assert (bst.predict(xgb.DMatrix(Xc)) == yc).mean() > 0.6

    Xb, yb, wb = tm.make_batches(100, 4, 3, seed=3)
    assert len(Xb) == 3 and Xb[0].shape == (100, 4) and wb[0].min() >= 0

    Xl, yl, qid = tm.make_ltr(600, 5, 20, max_rel=3, seed=4)
    assert qid.shape == (600,) and (np.diff(qid) >= 0).all()
    d = xgb.DMatrix(Xl, label=yl)
    d.set_info(qid=qid)
    bst = xgb.train({"objective": "rank:ndcg", "max_depth": 3,
                     "eval_metric": "ndcg"}, d, 5)

    csr, ys = tm.make_sparse_regression(300, 10, sparsity=0.8, seed=5)
    assert csr.nnz < 300 * 10 * 0.4
    bst = xgb.train({"max_depth": 3}, xgb.DMatrix(csr, label=ys), 3)

    Xcat, ycat = tm.make_categorical(300, 4, 8, cat_ratio=0.5, seed=6)
    d = xgb.DMatrix(Xcat, label=ycat, enable_categorical=True)
    bst = xgb.train({"max_depth": 3}, d, 3)
    assert np.isfinite(bst.predict(d)).all()


def test_vector_leaf_requires_hist():
    """reference gbtree.cc:187: multi_output_tree rejects non-hist
    tree methods."""
    import xgboost_amd as xgb
    rng = np.random.RandomState(0)
    X = rng.randn(80, 4).astype(np.float32)
    Y = rng.randn(80, 2).astype(np.float32)
    d = xgb.DMatrix(X, label=Y)
    with pytest.raises(ValueError, match="hist tree method"):
        xgb.train({"multi_strategy": "multi_output_tree",
                   "tree_method": "approx", "max_depth": 3}, d, 1)


def test_param_lower_bounds():
    """reference param.h field bounds: eta >= 0, max_depth >= 0."""
    import xgboost_amd as xgb
    X = np.ones((20, 2), np.float32)
    d = xgb.DMatrix(X, label=np.zeros(20, np.float32))
    with pytest.raises(ValueError, match="eta"):
        xgb.train({"eta": -0.1, "max_depth": 2}, d, 1)
    with pytest.raises(ValueError, match="max_depth"):
        xgb.train({"max_depth": -2}, d, 1)


def test_gpu_id_deprecated_spelling():
    """reference maps gpu_id=N to device=cuda:N; the name must pass
    parameter validation."""
    import xgboost_amd as xgb
    b = xgb.Booster({"gpu_id": 1, "validate_parameters": 1})
    assert str(b.device) == "cuda:1"
    b2 = xgb.Booster({"device": "cpu", "gpu_id": 0})
    assert b2.device.type == "cpu"  # explicit device wins


def test_bench_dump_outputs_and_full(tmp_path):
    """bench.py --dump-outputs writes the last step's tree and margin as
    float arrays; --full adds the training-AUC check a plain run skips."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = 5000

    def run(*extra):
        out = subprocess.run(
            [sys.executable, os.path.join(repo, "bench.py"), "--steps", "2",
             "--warmup", "1", "--rows", str(rows), *extra],
            capture_output=True, text=True, timeout=300, cwd=repo)
        assert out.returncode == 0, out.stdout + out.stderr
        return json.loads(out.stdout.strip().splitlines()[-1])

    plain = run("--dump-outputs", str(tmp_path / "a"))
    full = run("--full", "--dump-outputs", str(tmp_path / "b"))
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0
    assert plain["config"]["train_auc"] is None
    assert 0.5 < full["config"]["train_auc"] <= 1.0
    names = sorted(os.listdir(tmp_path / "a"))
    assert "margin.npy" in names and "tree_split_cond.npy" in names
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for name in names:
        a = np.load(tmp_path / "a" / name)
        b = np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), name
        # seeded inputs: two runs give the same outputs
        np.testing.assert_array_equal(a, b, err_msg=name)
        total += a.nbytes
    assert np.load(tmp_path / "a" / "margin.npy").shape == (rows,)
    assert total <= 64 * 2 ** 20
