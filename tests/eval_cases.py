"""Synthetic int64 node histograms shared by the split-evaluation tests
(test_gpu_eval_leaf.py for the HIP kernels, test_eval_cpu.py for the
native CPU evaluator)."""
import numpy as np

# one wave's chunk is 64 bins and the block covers 256: widths on both
# sides of each, a one- and a two-bin feature, and one far wider than the
# block (the max_bin 1024 case)
WIDTHS = np.array([1, 2, 63, 64, 65, 128, 255, 256, 257, 1000])
PTRS = np.concatenate([[0], np.cumsum(WIDTHS)]).astype(np.int32)
F = len(WIDTHS)
NB = int(PTRS[-1])
QS = float(1 << 30)
# a bin holds up to a few thousand rows of gradients quantized to 2^30
BIN_MAX = 3000 * (1 << 30)
G_SCALE = QS / 3.7
H_SCALE = QS / 0.9

REGULARIZED = {"reg_alpha": 0.3, "max_delta_step": 0.7,
               "min_child_weight": 2.5, "reg_lambda": 1.5}

_hist_cache = {}


def hists(k):
    """-> (hist [k, n_bins, 2], parents [k, 2]) int64, built once per k.

    Every feature of a node sums to the node's parent minus a missing
    remainder, as real histograms do.  Even nodes have a remainder (h >=
    0, g of either sign) that differs per feature; odd nodes have none,
    so both missing directions tie at every bin.  Runs of empty bins give
    consecutive equal gains.  Node 0 has one all-empty feature; the last
    node (k >= 3) has h = 0 everywhere."""
    if k in _hist_cache:
        return _hist_cache[k]
    rng = np.random.RandomState(100 + k)
    hist = np.zeros((k, NB, 2), np.int64)
    hist[:, :, 0] = rng.randint(-BIN_MAX, BIN_MAX, (k, NB))
    hist[:, :, 1] = rng.randint(0, BIN_MAX, (k, NB))
    for i in range(k):
        for f in range(F):
            b0, b1 = int(PTRS[f]), int(PTRS[f + 1])
            for _ in range(3):  # runs of empty bins
                if b1 - b0 >= 8:
                    s = rng.randint(b0, b1 - 4)
                    hist[i, s:s + rng.randint(2, 40), :][: b1 - s] = 0
    hist[0, PTRS[6]:PTRS[7], :] = 0  # an all-empty feature
    parents = np.zeros((k, 2), np.int64)
    for i in range(k):
        tot = np.stack([hist[i, PTRS[f]:PTRS[f + 1]].sum(0)
                        for f in range(F)])          # [F, 2]
        parents[i, 0] = tot[:, 0].max() + rng.randint(-BIN_MAX, BIN_MAX)
        parents[i, 1] = tot[:, 1].max() + rng.randint(0, BIN_MAX)
        if i % 2 == 1:
            # no missing remainder: top one bin of every feature up to the
            # parent (h stays >= 0: the parent is above every total)
            for f in range(F):
                b = rng.randint(PTRS[f], PTRS[f + 1])
                hist[i, b] += parents[i] - tot[f]
    if k >= 3:
        hist[k - 1, :, 1] = 0
        parents[k - 1, 1] = 0
    _hist_cache[k] = (hist, parents)
    return _hist_cache[k]


def monotone_and_bounds(k):
    """The monotone signs and per-node weight bounds of the monotone case."""
    rng = np.random.RandomState(1)
    mono = np.array([1, -1, 1, -1, 0, 1, -1, 0, 1, -1], np.int8)
    lo = -np.abs(rng.randn(k)) * 2.0
    bounds = np.stack([lo, lo + np.abs(rng.randn(k)) * 3.0], axis=1)
    return mono, bounds


def per_node_mask(k):
    rng = np.random.RandomState(2)
    mask = (rng.rand(k, F) < 0.5).astype(np.uint8)
    mask[:, 3] = 1
    return mask


def check_best_against_oracle(best, want, k):
    """best: packed [k, 6] records; want: evaluate_splits_np's entries.
    Feature, bin, dir and left sums exact; gain to 1e-12 relative."""
    import pytest
    n_valid = 0
    for i, e in enumerate(want):
        if e.feature < 0:
            assert best[i, 1] == -1 and best[i, 5] == -1, i
            continue
        n_valid += 1
        assert int(best[i, 5]) == e.feature, (i, best[i], e)
        assert int(best[i, 1]) == e.split_bin, (i, best[i], e)
        assert bool(best[i, 2]) == e.default_left, (i, best[i], e)
        assert int(best[i, 3]) == e.left_gq and int(best[i, 4]) == e.left_hq
        assert best[i, 0:1].view(np.float64)[0] == pytest.approx(
            e.gain, rel=1e-12)
    assert n_valid >= (k + 1) // 2
    return n_valid
