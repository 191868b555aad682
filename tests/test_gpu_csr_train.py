"""Kernel-level tests of the quantized-CSR training kernels (csr.hip):
gbt_hist_csr against the plain np.add.at reference and gbt_partition_csr
against a per-row Python loop, both bit-exactly."""
import numpy as np
import pytest
import torch

import hist_cases as hc
from xgboost_amd.splits import SplitEntry

pytestmark = pytest.mark.gpu


def _csr_ops(case):
    from xgboost_amd.sparse import CsrGpuOps
    return CsrGpuOps(case.sqm, "cuda")


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _check_hist(case, qg, ridx, segs):
    ops = _csr_ops(case)
    ops.reset(case.n_rows)
    ops.ridx = _dev(ridx)
    ops.segments = dict(enumerate(segs))
    nids = list(range(len(segs)))
    got = ops.build_hist_nodes(_dev(qg), nids)
    torch.cuda.synchronize()
    ref = hc.ref_hist_csr(case, qg, ridx,
                          [(i, s, e) for i, (s, e) in enumerate(segs)],
                          len(segs))
    assert got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), ref)
    return ref


_WIDTHS = [8] * 50


def _live_ridx(n, must, seed):
    """Permuted 80 % subset of the rows with `must` in the first segment."""
    ridx = hc.subset_ridx(n, seed=seed)
    keep = [r for r in ridx if r not in must]
    return np.asarray(list(must) + keep[:len(ridx) - len(must)], np.int64)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 3000])
def test_hist_csr_rows(n):
    rows = hc.random_csr_rows(n, _WIDTHS, 50, seed=n)
    if n == 1:
        rows[0] = {0: 0, 49: 7}                          # first / last bin
        ridx, segs = np.zeros(1, np.int64), [(0, 0), (0, 0), (0, 1)]
    else:
        rows[0] = {}                                     # empty row
        rows[1] = {f: (f % 8) for f in range(50)}        # every feature
        ridx = _live_ridx(n, [0, 1], seed=n)
        segs = hc.three_segments(len(ridx))
    case = hc.make_csr_case(_WIDTHS, rows)
    ref = _check_hist(case, hc.make_gpair(n, seed=n), ridx, segs)
    assert not ref[1].any()


def test_hist_csr_wide():
    # 20000 features x 2 bins, about 10 nonzeros per row
    widths = [2] * 20000
    rows = hc.random_csr_rows(2000, widths, 20, seed=9)
    rows[0] = {0: 0, 19999: 1}
    case = hc.make_csr_case(widths, rows)
    assert case.n_bins == 40000
    ridx = _live_ridx(2000, [0], seed=9)
    ref = _check_hist(case, hc.make_gpair(2000, seed=9), ridx,
                      hc.three_segments(len(ridx)))
    assert ref[0, 0].any() and ref[0, 39999].any()


@pytest.mark.parametrize("kind", ["extremes", "cancel"])
def test_hist_csr_value_edges(kind):
    """Every row hits one bin: INT32 extremes under full contention, and
    +a / -a pairs that must leave exactly zero."""
    n = 3000
    rows = [{3: 5} for _ in range(n)]
    case = hc.make_csr_case(_WIDTHS, rows)
    ridx = hc.subset_ridx(n, seed=4, frac=1.0)
    ref = _check_hist(case, hc.make_gpair(n, seed=6, kind=kind), ridx,
                      [(0, n)])
    if kind == "cancel":
        assert not ref.any()
    else:
        assert np.count_nonzero(ref[0, :, 1]) == 1


# ---- partition ------------------------------------------------------------

_PW = [4, 3, 5, 4, 2, 6, 4, 3, 5, 4, 2, 4]   # 12 features, 46 bins
_PF = len(_PW)
_FIRST, _MID, _LAST, _RARE = 0, 6, _PF - 1, 1
_N = 4200


def _partition_case():
    rng = np.random.RandomState(17)
    presence = np.full(_PF, 0.6)
    presence[_RARE] = 0.1
    rows = []
    for _ in range(_N):
        rows.append({f: int(rng.randint(0, _PW[f])) for f in range(_PF)
                     if rng.rand() < presence[f]})
    # the split feature absent, its neighbours present at the bins just
    # outside its range: global lo - 1 and hi (FindFeatureBin off-by-one)
    i = 0
    for f in (_FIRST, _MID, _LAST):
        for with_rest in (False, True):
            for _ in range(40):
                r = dict(rows[i]) if with_rest else {}
                r.pop(f, None)
                if f > 0:
                    r[f - 1] = _PW[f - 1] - 1
                if f + 1 < _PF:
                    r[f + 1] = 0
                rows[i] = r
                i += 1
    for _ in range(20):
        rows[i] = {}
        rows[i + 1] = {f: int(rng.randint(0, _PW[f])) for f in range(_PF)}
        i += 2
    order = rng.permutation(_N)
    return hc.make_csr_case(_PW, [rows[j] for j in order])


@pytest.fixture(scope="module")
def pcase():
    return _partition_case()


def _goes_left(case, row, feature, sbin, dleft):
    lo = int(case.starts[feature])
    hi = lo + int(case.widths[feature])
    for b in case.bin_idx[case.row_ptr[row]:case.row_ptr[row + 1]]:
        if lo <= b < hi:
            return bool(b <= sbin)
    return bool(dleft)


def _check_partition(case, ridx, parents):
    """parents: [((begin, end), feature, global split bin, default_left)]"""
    ops = _csr_ops(case)
    ops.reset(case.n_rows)
    ops.ridx = _dev(ridx)
    ops._ridx_out = torch.empty_like(ops.ridx)
    ops.segments = {10 + i: seg for i, (seg, _, _, _) in enumerate(parents)}
    nids = [10 + i for i in range(len(parents))]
    splits = [SplitEntry(nid=nid, feature=f, split_bin=sb, default_left=dl)
              for nid, (_, f, sb, dl) in zip(nids, parents)]
    children = [(20 + 2 * i, 21 + 2 * i) for i in range(len(parents))]
    ops.partition_nodes(nids, splits, children)
    torch.cuda.synchronize()
    got = ops.ridx.cpu().numpy()
    covered = np.zeros(len(ridx), bool)
    counts = []
    for ((s, e), f, sb, dl), (l, r) in zip(parents, children):
        rows = ridx[s:e]
        left = [int(x) for x in rows if _goes_left(case, x, f, sb, dl)]
        counts.append((len(left), e - s - len(left)))
        assert ops.segments[l] == (s, s + len(left))
        assert ops.segments[r] == (s + len(left), e)
        assert sorted(got[s:s + len(left)].tolist()) == sorted(left)
        assert sorted(got[s:e].tolist()) == sorted(rows.tolist())
        covered[s:e] = True
    assert np.array_equal(got[~covered], ridx[~covered])
    return counts


_SEG_A, _SEG_B = (100, 3100), (3300, 4000)   # 3000 rows: 3 tasks; 700: 1


def _split_bin(case, feature, which):
    lo = int(case.starts[feature])
    return lo if which == "lowest" else lo + int(case.widths[feature]) - 1


@pytest.mark.parametrize("dleft", [False, True])
@pytest.mark.parametrize("which", ["lowest", "highest"])
@pytest.mark.parametrize("feature", [_FIRST, _MID, _LAST],
                         ids=["first", "middle", "last"])
def test_partition_csr(pcase, feature, which, dleft):
    ridx = hc.subset_ridx(_N, seed=21, frac=1.0)
    other = "highest" if which == "lowest" else "lowest"
    counts = _check_partition(pcase, ridx, [
        (_SEG_A, feature, _split_bin(pcase, feature, which), dleft),
        (_SEG_B, feature, _split_bin(pcase, feature, other), not dleft)])
    if which == "lowest":
        # both sides of the big parent are populated
        assert counts[0][0] > 0 and counts[0][1] > 0


@pytest.mark.parametrize("big_goes", ["left", "right"])
def test_partition_csr_one_sided(pcase, big_goes):
    """Every row of a parent on one side (the tot_l == 0 / tot_r == 0
    branches): the highest bin with default left keeps all rows left; a
    parent of rows without the feature and default right sends all
    right."""
    lo = int(pcase.starts[_RARE])
    hi = lo + int(pcase.widths[_RARE])
    has = np.array([any(lo <= b < hi for b in pcase.bin_idx[
        pcase.row_ptr[r]:pcase.row_ptr[r + 1]]) for r in range(_N)])
    rng = np.random.RandomState(23)
    absent = rng.permutation(np.flatnonzero(~has))
    assert len(absent) >= 3000
    all_left = (_MID, _split_bin(pcase, _MID, "highest"), True)
    all_right = (_RARE, _split_bin(pcase, _RARE, "highest"), False)
    # [sa, ea) holds rows without the rare feature only and goes right
    (sa, ea), (sb, eb) = (_SEG_A, _SEG_B) if big_goes == "right" \
        else (_SEG_B, _SEG_A)
    ridx = np.empty(_N, np.int64)
    ridx[sa:ea] = absent[:ea - sa]
    mask = np.ones(_N, bool)
    mask[sa:ea] = False
    ridx[mask] = rng.permutation(np.concatenate(
        [absent[ea - sa:], np.flatnonzero(has)]))
    assert sorted(ridx.tolist()) == list(range(_N))
    counts = _check_partition(pcase, ridx, [((sa, ea),) + all_right,
                                            ((sb, eb),) + all_left])
    assert counts[0] == (0, ea - sa)
    assert counts[1] == (eb - sb, 0)
