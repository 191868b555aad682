"""Single-pass split evaluation against the single-wave reference kernel
(bit for bit, every (node, feature) slot) and against the numpy oracle
(the selected split per node), on synthetic int64 histograms."""
import numpy as np
import pytest
import torch

import eval_cases as ec
from eval_cases import F as _F, G_SCALE as _G_SCALE, H_SCALE as _H_SCALE
from eval_cases import NB as _NB, PTRS as _PTRS, QS as _QS
from eval_cases import hists as _hists
from xgboost_amd.params import make_train_param
from xgboost_amd.splits import evaluate_splits_np

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------
# evaluate: gbt_evaluate_masked vs gbt_evaluate_ref vs numpy

_SENTINEL = -77


def _launch(fn, hist, parents, k_launch, p, *, maxabs=None, scales=None,
            monotone=None, bounds=None, mask=None, mask_stride=0, cat=None,
            k_dev=None, narrow_max=0):
    """One evaluate launch with sentinel-filled outputs -> numpy
    (gain bits, bin, dir, lsum)."""
    from xgboost_amd import ops
    dev = torch.device("cuda")

    def up(a, dt):
        return (None if a is None
                else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev))

    t_hist, t_par = up(hist, np.int64), up(parents, np.int64)
    t_ptrs = up(_PTRS, np.int32)
    t_maxabs, t_mono = up(maxabs, np.float32), up(monotone, np.int8)
    t_bounds, t_mask = up(bounds, np.float64), up(mask, np.uint8)
    t_cat = up(cat, np.uint8)
    t_kdev = up(None if k_dev is None else np.array([k_dev]), np.int32)
    n = hist.shape[0]
    gain = torch.full((n, _F), _SENTINEL, dtype=torch.int64, device=dev)
    bins = torch.full((n, _F), _SENTINEL, dtype=torch.int32, device=dev)
    dirs = torch.full((n, _F), 200, dtype=torch.uint8, device=dev)
    lsum = torch.full((n, _F, 2), _SENTINEL, dtype=torch.int64, device=dev)
    gs, hs = scales if scales is not None else (_G_SCALE, _H_SCALE)
    fn(ops.ptr(t_hist), k_launch, _NB, _F, ops.ptr(t_ptrs), ops.ptr(t_par),
       ops.ptr(t_maxabs), gs, hs, p.reg_lambda, p.reg_alpha,
       p.max_delta_step, p.min_child_weight, ops.ptr(t_mono),
       ops.ptr(t_bounds), mask_stride, ops.ptr(t_mask), ops.ptr(t_cat),
       ops.ptr(gain), ops.ptr(bins), ops.ptr(dirs), ops.ptr(lsum),
       ops.ptr(t_kdev), narrow_max, ops.stream())
    best = torch.full((n, 6), _SENTINEL, dtype=torch.int64, device=dev)
    ops.load().gbt_select_best(ops.ptr(gain), ops.ptr(bins), ops.ptr(dirs),
                               ops.ptr(lsum), k_launch, _F, ops.ptr(best),
                               ops.ptr(t_kdev), ops.stream())
    torch.cuda.synchronize()
    return (gain.cpu().numpy(), bins.cpu().numpy(), dirs.cpu().numpy(),
            lsum.cpu().numpy(), best.cpu().numpy())


def _check(k, params=None, oracle=True, **kw):
    """New kernel == reference kernel in every output slot; its selected
    split per node == the numpy oracle's.  Returns the new kernel's
    outputs."""
    from xgboost_amd import ops
    lib = ops.load()
    hist, parents = _hists(k)
    p = make_train_param(dict({"max_depth": 6}, **(params or {})))
    new = _launch(lib.gbt_evaluate_masked, hist, parents, k, p, **kw)
    ref = _launch(lib.gbt_evaluate_ref, hist, parents, k, p, **kw)
    for name, a, b in zip(("gain bits", "bin", "dir", "lsum", "best"),
                          new, ref):
        assert np.array_equal(a, b), name
    if not oracle:
        return new
    mask = kw.get("mask")
    fsets = None
    if mask is not None:
        rows = mask if kw.get("mask_stride") else np.repeat(mask, k, axis=0)
        fsets = [np.nonzero(r)[0] for r in rows.reshape(k, _F)]
    cat = kw.get("cat")
    want = evaluate_splits_np(
        hist, [tuple(int(v) for v in r) for r in parents], _G_SCALE,
        _H_SCALE, list(range(k)), _PTRS, p, feature_sets=fsets,
        monotone=kw.get("monotone"),
        cat_mask=None if cat is None else cat.astype(bool),
        node_bounds=kw.get("bounds"))
    ec.check_best_against_oracle(new[4], want, k)
    return new


@pytest.mark.parametrize("k", [1, 3, 130])
def test_evaluate_matches_ref_and_oracle(k):
    gain, bins, dirs, lsum, _ = _check(k)
    hist, parents = _hists(k)
    g = gain.view(np.float64)
    # the all-empty feature of node 0: with a missing remainder the only
    # candidates put everything on one side
    assert bins[0, 6] == -1 and g[0, 6] == -np.inf
    if k >= 3:
        assert np.all(bins[k - 1] == -1)  # h = 0: nothing is valid
        # no missing remainder (odd nodes): both directions tie, dir 0 wins
        # (the one-bin feature holds the whole parent: no valid split)
        assert np.all(bins[1, 1:] >= 0) and np.all(dirs[1] == 0)
    # an empty bin ties with the bin before it, and the lower bin wins:
    # the chosen bin is never empty unless it is the feature's first
    for i in range(k):
        for f in range(_F):
            b = bins[i, f]
            if b > _PTRS[f]:
                assert hist[i, b].any(), (i, f, b)


def test_evaluate_monotone_with_bounds():
    k = 5
    mono, bounds = ec.monotone_and_bounds(k)
    _check(k, monotone=mono, bounds=bounds)


def test_evaluate_per_node_mask():
    k = 5
    mask = ec.per_node_mask(k)
    gain, bins, *_ = _check(k, mask=mask, mask_stride=_F)
    assert np.all(bins[mask == 0] == -1)
    assert np.all(gain.view(np.float64)[mask == 0] == -np.inf)


_BROADCAST_MASK = np.array([[1, 0, 1, 1, 0, 1, 0, 1, 1, 0]], np.uint8)


def test_evaluate_broadcast_mask_row():
    mask = _BROADCAST_MASK
    gain, bins, *_ = _check(5, mask=mask, mask_stride=0)
    assert np.all(bins[:, mask[0] == 0] == -1)


def test_evaluate_categorical_feature():
    cat = np.zeros(_F, np.uint8)
    cat[4] = 1  # 65 categories, one-vs-rest
    # min_child_weight stays at its default of 1, so the oracle's one-hot
    # branch rejects the same empty-side candidates as the kernels do
    _check(5, params={"max_cat_to_onehot": 128}, cat=cat)


def test_evaluate_regularized():
    _check(5, params=ec.REGULARIZED)


_MAXABS = np.array([3.7, 0.9], np.float32)


def test_evaluate_device_scales_match_host_scales():
    from xgboost_amd import ops
    lib = ops.load()
    k = 5
    hist, parents = _hists(k)
    p = make_train_param({"max_depth": 6})
    maxabs = _MAXABS
    scales = tuple(_QS / float(m) for m in maxabs)
    dev_new = _launch(lib.gbt_evaluate_masked, hist, parents, k, p,
                      maxabs=maxabs, scales=(0.0, 0.0))
    dev_ref = _launch(lib.gbt_evaluate_ref, hist, parents, k, p,
                      maxabs=maxabs, scales=(0.0, 0.0))
    host_new = _launch(lib.gbt_evaluate_masked, hist, parents, k, p,
                       scales=scales)
    for a, b, c in zip(dev_new, dev_ref, host_new):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.any(dev_new[1] >= 0)


def test_evaluate_k_dev_leaves_later_slots_untouched():
    k, live = 130, 77
    new = _check(k, oracle=False, k_dev=live)
    full = _check(k, oracle=False)
    gain, bins, dirs, lsum, best = new
    assert np.all(gain[live:] == _SENTINEL) and np.all(bins[live:] == _SENTINEL)
    assert np.all(dirs[live:] == 200) and np.all(lsum[live:] == _SENTINEL)
    assert np.all(best[live:] == _SENTINEL)
    for a, b in zip(new, full):
        assert np.array_equal(a[:live], b[:live])


# ---------------------------------------------------------------------------
# narrow path: EvaluateNarrowKernel's slots vs the block kernel's


def _narrow_cases():
    mono, bounds = ec.monotone_and_bounds(5)
    cat = np.zeros(_F, np.uint8)
    cat[1] = cat[4] = 1  # a narrow (two-bin) one and a wide one
    return {
        "plain": (5, None, {}),
        "regularized": (5, ec.REGULARIZED, {}),
        "monotone_bounds": (5, None, dict(monotone=mono, bounds=bounds)),
        "per_node_mask": (5, None, dict(mask=ec.per_node_mask(5),
                                        mask_stride=_F)),
        "broadcast_mask": (5, None, dict(mask=_BROADCAST_MASK,
                                         mask_stride=0)),
        "device_scales": (5, None, dict(maxabs=_MAXABS, scales=(0.0, 0.0))),
        "categorical": (5, {"max_cat_to_onehot": 128}, dict(cat=cat)),
        "k_dev": (130, None, dict(k_dev=77)),
    }


@pytest.mark.parametrize("narrow_max", [2, 64, 256])
@pytest.mark.parametrize("case", list(_narrow_cases()))
def test_evaluate_narrow_matches_block(case, narrow_max):
    """With narrow_max = n the scalar kernel owns every non-categorical
    feature of at most n bins (2, 4 and 8 of the ten); every output slot,
    the sentinels in untouched ones included, equals narrow_max = 0."""
    from xgboost_amd import ops
    lib = ops.load()
    k, params, kw = _narrow_cases()[case]
    hist, parents = _hists(k)
    p = make_train_param(dict({"max_depth": 6}, **(params or {})))
    block = _launch(lib.gbt_evaluate_masked, hist, parents, k, p, **kw)
    narrow = _launch(lib.gbt_evaluate_masked, hist, parents, k, p,
                     narrow_max=narrow_max, **kw)
    for name, a, b in zip(("gain bits", "bin", "dir", "lsum", "best"),
                          narrow, block):
        assert np.array_equal(a, b), name
    live = kw.get("k_dev", k)
    gain, bins, dirs, lsum, best = narrow
    assert np.all(gain[live:] == _SENTINEL) and np.all(dirs[live:] == 200)
    assert np.all(best[live:] == _SENTINEL)
    if "mask" not in kw and "monotone" not in kw:
        # the one-bin feature of an even node splits present from missing:
        # the narrow kernel found it
        assert bins[0, 0] == 0
    if "cat" in kw:
        # the flagged two-bin feature stays with the block kernel, which
        # writes the whole record
        assert np.all(bins[:, 1] != _SENTINEL) and np.all(dirs[:, 1] != 200)
        assert np.all(lsum[:, 1] != _SENTINEL)
    if "mask" in kw:
        rows = np.broadcast_to(kw["mask"], (k, _F)) == 0
        assert np.all(bins[rows] == -1) and np.all(dirs[rows] == 200)
        assert np.all(lsum[rows] == _SENTINEL)


# ---------------------------------------------------------------------------
# select: gbt_select_best vs numpy argmax

_SELECT_K = 4
_select_cache = {}


def _select_inputs(f):
    """Gains from eight finite values (ties everywhere) with about a
    quarter -inf; row 1 all -inf; row 2's maximum planted at f = 70 and
    again at the last feature; random payload."""
    if f in _select_cache:
        return _select_cache[f]
    k = _SELECT_K
    rng = np.random.RandomState(7 + f)
    values = np.array([-3.5, -1.0, 0.0, 0.125, 0.5, 1.0, 2.75, 9.0])
    gain = values[rng.randint(0, 8, (k, f))]
    gain[rng.rand(k, f) < 0.25] = -np.inf
    gain[1] = -np.inf
    if f > 70:
        gain[2, 70] = gain[2, f - 1] = 11.0
    bins = rng.randint(0, 1 << 20, (k, f)).astype(np.int32)
    dirs = rng.randint(0, 2, (k, f)).astype(np.uint8)
    lsum = rng.randint(-(1 << 50), 1 << 50, (k, f, 2)).astype(np.int64)
    want = np.zeros((k, 6), np.int64)
    for i in range(k):
        if not np.isfinite(gain[i]).any():
            want[i] = (0, -1, 0, 0, 0, -1)
            continue
        j = int(np.argmax(gain[i]))  # the first maximum
        want[i] = (gain[i, j:j + 1].view(np.int64)[0], bins[i, j],
                   dirs[i, j], lsum[i, j, 0], lsum[i, j, 1], j)
    _select_cache[f] = (gain, bins, dirs, lsum, want)
    return _select_cache[f]


def _select(f, k_dev=None):
    from xgboost_amd import ops
    dev = torch.device("cuda")
    gain, bins, dirs, lsum, want = _select_inputs(f)
    t = [torch.from_numpy(a).to(dev) for a in (gain, bins, dirs, lsum)]
    t_kdev = (None if k_dev is None else
              torch.tensor([k_dev], dtype=torch.int32, device=dev))
    best = torch.full((_SELECT_K, 6), _SENTINEL, dtype=torch.int64,
                      device=dev)
    ops.load().gbt_select_best(ops.ptr(t[0]), ops.ptr(t[1]), ops.ptr(t[2]),
                               ops.ptr(t[3]), _SELECT_K, f, ops.ptr(best),
                               ops.ptr(t_kdev), ops.stream())
    torch.cuda.synchronize()
    return best.cpu().numpy(), want


# 4096 is the last width of the one-wave launch and 4097 the first of the
# 1024-thread one; at 20001 every thread of the latter loops
@pytest.mark.parametrize("f", [1, 63, 4096, 4097, 20001])
def test_select_best_matches_numpy_argmax(f):
    got, want = _select(f)
    assert np.array_equal(got, want)
    assert want[1, 5] == -1
    if f > 70:
        assert want[2, 5] == 70  # the lower index wins across waves


@pytest.mark.parametrize("f", [63, 4097])
def test_select_best_k_dev_leaves_later_rows_untouched(f):
    got, want = _select(f, k_dev=2)
    assert np.array_equal(got[:2], want[:2])
    assert np.all(got[2:] == _SENTINEL)
