"""Both CPU histogram implementations (the native C kernel and the torch
oracle) against the plain reference in hist_cases.py, bit-exactly, over
the geometry matrix the GPU kernels are tested on.  The older GPU tests
compare against CpuOps, so this is what pins their yardstick."""
import numpy as np
import pytest
import torch

import hist_cases as hc
from xgboost_amd.backend.cpu import CpuOps
from xgboost_amd.backend.gpu import _check_bin_dtype, _chunk_tasks

IMPLS = ["native", "torch"]


def _cpu_ops(qm, impl):
    ops = CpuOps(qm, use_native=(impl == "native"))
    # neither request may quietly run the other implementation
    assert (ops.lib is not None) == (impl == "native")
    return ops


def _check(case, qg, ridx, segs, impl):
    ops = _cpu_ops(case.qm, impl)
    got = ops.build_hist(torch.from_numpy(qg), torch.from_numpy(ridx), segs)
    ref = hc.ref_hist(case, qg, ridx,
                      [(i, s, e) for i, (s, e) in enumerate(segs)],
                      len(segs))
    assert got.dtype == torch.int64
    assert np.array_equal(got.numpy(), ref)
    return ref


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", sorted(hc.GEOMETRIES))
def test_cpu_hist_geometry(name, impl):
    case = hc.geometry_case(name)
    assert case.qm.gidx.dtype == hc.GEOMETRIES[name][2]
    ridx = hc.subset_ridx(case.n_rows)
    ref = _check(case, hc.make_gpair(case.n_rows), ridx,
                 hc.three_segments(len(ridx)), impl)
    assert not ref[1].any()
    if name == "L":
        # the case exists for local ids that do not fit a signed 16-bit
        assert (case.local[ridx[:(2 * len(ridx)) // 5], 0] >= 32768).any()


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", hc.ROW_EDGES)
@pytest.mark.parametrize("name", ["A", "G"])
def test_cpu_hist_row_edges(name, n, impl):
    case = hc.geometry_case(name, n=n, seed=n)
    ridx = hc.subset_ridx(n, seed=n, frac=1.0)
    _check(case, hc.make_gpair(n, seed=n), ridx, [(0, n)], impl)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("kind", hc.VALUE_EDGES)
@pytest.mark.parametrize("name", ["M", "A"])
def test_cpu_hist_value_edges(name, kind, impl):
    case, qg = hc.value_edge(name, kind)
    n = case.n_rows
    ridx = hc.subset_ridx(n, seed=5, frac=1.0)
    ref = _check(case, qg, ridx, [(0, n)], impl)
    if kind == "cancel":
        assert not ref.any()
    if kind == "contention":
        # one bin per feature holds every row
        assert np.count_nonzero(ref[0, :, 1]) == len(case.widths)


def test_global_gidx_reads_16bit_storage_unsigned():
    """Local ids >= 32768 live in int16 storage as negative numbers."""
    case = hc.geometry_case("L", n=200)
    assert case.qm.gidx.dtype == torch.int16
    assert (case.qm.gidx[:, 0] < 0).any()
    want = np.where(case.miss, -1, case.local + case.starts[None, :])
    assert np.array_equal(case.qm.global_gidx().numpy(), want)


@pytest.mark.parametrize("impl", IMPLS)
def test_cpu_hist_int32_bins(impl):
    """Above 65535 local ids the matrix is int32, which the C kernel
    cannot read: CpuOps must stay exact by not handing it over."""
    case = hc.make_case([70000, 5], 0.1, 500, seed=3)
    assert case.qm.gidx.dtype == torch.int32
    ops = CpuOps(case.qm, use_native=(impl == "native"))
    assert ops.lib is None
    ridx = hc.subset_ridx(500)
    segs = hc.three_segments(len(ridx))
    qg = hc.make_gpair(500)
    got = ops.build_hist(torch.from_numpy(qg), torch.from_numpy(ridx), segs)
    ref = hc.ref_hist(case, qg, ridx,
                      [(i, s, e) for i, (s, e) in enumerate(segs)], 3)
    assert np.array_equal(got.numpy(), ref)


def test_gpu_bin_dtype_guard():
    """The HIP launchers take a u8 and a u16 pointer: the guard GpuOps
    runs on every bin matrix rejects anything else."""
    _check_bin_dtype(torch.zeros((2, 2), dtype=torch.uint8))
    _check_bin_dtype(torch.zeros((2, 2), dtype=torch.int16))
    for dt in (torch.int32, torch.int64, torch.int8):
        with pytest.raises(ValueError, match="65535"):
            _check_bin_dtype(torch.zeros((2, 2), dtype=dt))


# ---- _chunk_tasks ---------------------------------------------------------

_SEGMENT_SETS = [
    [(0, 1)],
    [(0, 1023)], [(0, 1024)], [(0, 1025)], [(0, 2049)],
    [(0, 1200), (1200, 1200), (1200, 2400)],
    [(5, 5)],
    [(0, 0), (0, 0)],
    [(10, 4000), (4000, 4001), (4001, 9000)],
    [(0, 700000), (700000, 700001)],
]


@pytest.mark.parametrize("kw", [{}, {"target_tasks": 512},
                                {"target_tasks": 4, "min_rows": 1}])
@pytest.mark.parametrize("segs", _SEGMENT_SETS)
def test_chunk_tasks_tile_segments(segs, kw):
    slots = [7 + 3 * i for i in range(len(segs))]
    for use_slots in (False, True):
        tasks = _chunk_tasks(segs, slots=slots if use_slots else None, **kw)
        assert tasks.dtype == np.int32 and tasks.shape[1] == 4
        assert not tasks[:, 3].any()
        if all(s == e for s, e in segs):
            # the single placeholder for "no rows"
            assert tasks.tolist() == [[0, 0, 0, 0]]
            continue
        assert (tasks[:, 1] < tasks[:, 2]).all(), "empty task"
        pos = 0
        for i, (s, e) in enumerate(segs):
            slot = slots[i] if use_slots else i
            cur = s
            while cur < e:
                t_slot, b, t_e, _ = tasks[pos]
                assert (t_slot, b) == (slot, cur)
                assert t_e <= e
                cur = t_e
                pos += 1
        assert pos == len(tasks)
        sizes = tasks[:, 2] - tasks[:, 1]
        total = sum(e - s for s, e in segs)
        want = max(kw.get("min_rows", 1024),
                   -(-total // kw.get("target_tasks", 2048)))
        assert sizes.max() <= want
