"""Generators and the plain reference shared by the histogram kernel
tests (test_hist_cpu.py, test_gpu_hist.py, test_gpu_csr_train.py).

A case is built from integers only: per-feature widths, a matrix of
local bin ids, a missing mask, int32 gradient pairs, a row-index array
and (slot, begin, end) tasks.  The reference accumulates them with
np.add.at into int64 and shares no code with the kernels, the C path or
the torch oracle: cuts and the quantized matrix are assembled directly
from the width list, so the geometry does not depend on the sketch.
"""
import dataclasses

import numpy as np
import torch

from xgboost_amd.data import QuantizedMatrix, _pick_bin_dtype
from xgboost_amd.quantile import HistogramCuts

I32_MIN = -2 ** 31
I32_MAX = 2 ** 31 - 1

U8, I16 = torch.uint8, torch.int16

# name -> (widths, missing fraction, bin dtype, n_groups, use_shared).
# The last three are what GpuOps must select for the geometry; the tests
# assert them before any numeric check so a change to the mode selection
# cannot silently move a case onto another kernel.
#
# I: the register kernel needs every group to have <= 32 features and a
# group holds <= 8192 bins, so a group break at an unaligned feature
# index needs features wider than 256 bins, i.e. 16-bit storage with two
# features per 32-bit load: the break has to fall on an ODD index.
# 29 * 282 = 8178 bins, the next 64 do not fit: groups [0, 29, 40].
GEOMETRIES = {
    "A": ([64] * 12, 0.0, U8, 1, 3),
    "B": ([64] * 10, 0.0, U8, 1, 2),
    "C": ([16] * 33, 0.10, U8, 1, 1),
    "D": ([4] * 1100, 0.10, U8, 1, 1),
    "E": ([256] * 32, 0.0, U8, 1, 3),
    "F": ([255] * 32, 0.15, U8, 1, 3),
    "G": ([256] * 32, 0.15, I16, 1, 3),
    "H": ([256] * 40, 0.0, U8, 2, 3),
    "I": ([282] * 29 + [64] * 11, 0.0, I16, 2, 2),
    "J": ([1000] * 6, 0.10, I16, 1, 3),
    "K": ([1000] * 5, 0.0, I16, 1, 2),
    "L": ([40000, 10, 300], 0.10, I16, 2, 0),
    "M": ([1, 64, 1, 7, 256, 1, 33, 2], 0.20, I16, 1, 3),
}

ROW_EDGES = [1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049]
VALUE_EDGES = ["extremes", "cancel", "contention"]


@dataclasses.dataclass
class Case:
    widths: np.ndarray    # int64 [f]
    starts: np.ndarray    # int64 [f] first global bin of each feature
    local: np.ndarray     # int64 [n, f] local bin ids
    miss: np.ndarray      # bool  [n, f]
    qm: QuantizedMatrix   # what the code under test reads

    @property
    def n_rows(self):
        return self.local.shape[0]

    @property
    def n_bins(self):
        return int(self.widths.sum())


def make_qm(widths, local, miss, has_missing):
    widths = np.asarray(widths, np.int64)
    ptrs = np.zeros(len(widths) + 1, np.int64)
    np.cumsum(widths, out=ptrs[1:])
    cuts = HistogramCuts(
        values=np.arange(1, ptrs[-1] + 1, dtype=np.float32),
        ptrs=ptrs, min_vals=np.zeros(len(widths), np.float32))
    max_local = int(widths.max()) - (0 if has_missing else 1)
    dtype = _pick_bin_dtype(max_local)
    stored = np.where(miss, widths[None, :], local)
    assert stored.max(initial=0) <= max_local
    if dtype == torch.uint8:
        arr = stored.astype(np.uint8)
    elif dtype == torch.int16:
        arr = stored.astype(np.uint16).view(np.int16)
    else:
        arr = stored.astype(np.int32)
    return QuantizedMatrix(torch.from_numpy(np.ascontiguousarray(arr)),
                           cuts, has_missing)


def make_case(widths, missing, n, seed=0, pattern="random"):
    """pattern: "random"; "pairs" (rows 2i and 2i+1 carry the same
    bins); "same" (every row carries row 0's bins, nothing missing)."""
    rng = np.random.RandomState(seed)
    widths = np.asarray(widths, np.int64)
    f = len(widths)
    local = (rng.randint(0, 2 ** 31 - 1, size=(n, f)).astype(np.int64)
             % widths[None, :])
    miss = (rng.rand(n, f) < missing) if missing > 0 \
        else np.zeros((n, f), bool)
    # every feature's first and last bin is hit by a live row
    local[0] = widths - 1
    miss[0] = False
    if n > 1:
        local[1] = 0
        miss[1] = False
    if pattern == "pairs":
        local[1::2] = local[0:2 * (n // 2):2]
        miss[1::2] = miss[0:2 * (n // 2):2]
    elif pattern == "same":
        local[:] = local[0]
        miss[:] = False
    starts = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(np.int64)
    return Case(widths, starts, local, miss,
                make_qm(widths, local, miss, missing > 0))


def geometry_case(name, n=3000, seed=0, pattern="random"):
    widths, missing = GEOMETRIES[name][:2]
    return make_case(widths, missing, n, seed=seed + ord(name),
                     pattern=pattern)


def make_gpair(n, seed=1, kind="random"):
    """int32 [n, 2] gradient pairs over the whole int32 range."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        g = rng.randint(I32_MIN, I32_MAX + 1, size=n, dtype=np.int64)
        h = rng.randint(0, I32_MAX + 1, size=n, dtype=np.int64)
    elif kind in ("extremes", "contention"):
        vals = np.array([I32_MIN, I32_MAX, -1, 0, 1], np.int64)
        g = vals[rng.randint(0, 5, size=n)]
        g[:min(n, 5)] = vals[:min(n, 5)]
        h = np.full(n, I32_MAX, np.int64)
    elif kind == "cancel":
        # rows 2i / 2i+1 share their bins (pattern="pairs") and carry
        # +a / -a in both channels; an odd last row carries zero
        a = rng.randint(1, I32_MAX + 1, size=(n, 2), dtype=np.int64)
        a[1::2] = -a[0:2 * (n // 2):2]
        if n % 2:
            a[-1] = 0
        return a.astype(np.int32)
    else:
        raise ValueError(kind)
    return np.stack([g, h], axis=1).astype(np.int32)


def value_edge(name, kind, n=3000):
    """(case, gpair) for one value edge on one geometry."""
    pattern = {"extremes": "random", "cancel": "pairs",
               "contention": "same"}[kind]
    case = geometry_case(name, n=n, seed=7, pattern=pattern)
    return case, make_gpair(n, seed=11, kind=kind)


def subset_ridx(n, seed=2, frac=0.8):
    """Random permutation of a random subset of the rows."""
    rng = np.random.RandomState(seed)
    m = max(1, int(n * frac))
    return rng.permutation(n)[:m].astype(np.int64)


def three_segments(m):
    """Two live segments with an empty one between them; the tail of
    ridx lies outside every segment."""
    a = (2 * m) // 5
    b = (9 * m) // 10
    return [(0, a), (a, a), (a, b)]


def ref_hist(case, qg, ridx, tasks, k):
    """int64 [k, n_bins, 2] from (slot, begin, end) tasks."""
    out = np.zeros((k, case.n_bins, 2), np.int64)
    qg = np.asarray(qg).astype(np.int64)
    ridx = np.asarray(ridx)
    for slot, b, e in tasks:
        if e <= b:
            continue
        rows = ridx[b:e]
        ok = ~case.miss[rows]
        gbin = (case.local[rows] + case.starts[None, :])[ok]
        for c in range(2):
            v = np.broadcast_to(qg[rows, c][:, None], ok.shape)[ok]
            np.add.at(out[slot, :, c], gbin, v)
    return out


def ref_node_sums(qg, ridx, tasks, k):
    out = np.zeros((k, 2), np.int64)
    qg = np.asarray(qg).astype(np.int64)
    for slot, b, e in tasks:
        if e > b:
            out[slot] += qg[np.asarray(ridx)[b:e]].sum(axis=0)
    return out


# ---- quantized CSR -------------------------------------------------------

@dataclasses.dataclass
class CsrCase:
    widths: np.ndarray
    starts: np.ndarray
    row_ptr: np.ndarray   # int64 [n+1]
    bin_idx: np.ndarray   # int32 [nnz] global bins, sorted within a row
    sqm: object

    @property
    def n_rows(self):
        return len(self.row_ptr) - 1

    @property
    def n_bins(self):
        return int(self.widths.sum())


def make_csr_case(widths, rows):
    """rows: list of {feature: local bin}."""
    from xgboost_amd.sparse import SparseQuantizedMatrix
    widths = np.asarray(widths, np.int64)
    ptrs = np.zeros(len(widths) + 1, np.int64)
    np.cumsum(widths, out=ptrs[1:])
    row_ptr = np.zeros(len(rows) + 1, np.int64)
    bins = []
    for i, r in enumerate(rows):
        for f in sorted(r):
            assert 0 <= r[f] < widths[f]
            bins.append(int(ptrs[f]) + int(r[f]))
        row_ptr[i + 1] = len(bins)
    bin_idx = np.asarray(bins, np.int32).reshape(-1)
    cuts = HistogramCuts(
        values=np.arange(1, ptrs[-1] + 1, dtype=np.float32),
        ptrs=ptrs, min_vals=np.zeros(len(widths), np.float32))
    sqm = SparseQuantizedMatrix(torch.from_numpy(row_ptr),
                                torch.from_numpy(bin_idx), cuts,
                                len(widths))
    return CsrCase(widths, ptrs[:-1].copy(), row_ptr, bin_idx, sqm)


def random_csr_rows(n, widths, max_nnz, seed=0):
    """0..max_nnz present features per row, uniform bins."""
    rng = np.random.RandomState(seed)
    f = len(widths)
    rows = []
    for _ in range(n):
        k = int(rng.randint(0, max_nnz + 1))
        feats = rng.choice(f, size=k, replace=False)
        rows.append({int(j): int(rng.randint(0, widths[j])) for j in feats})
    return rows


def ref_hist_csr(case, qg, ridx, tasks, k):
    out = np.zeros((k, case.n_bins, 2), np.int64)
    qg = np.asarray(qg).astype(np.int64)
    for slot, b, e in tasks:
        for r in np.asarray(ridx)[b:e]:
            bins = case.bin_idx[case.row_ptr[r]:case.row_ptr[r + 1]]
            for c in range(2):
                np.add.at(out[slot, :, c], bins, qg[r, c])
    return out
