"""Cases, reference and comparison shared by the LambdaMART kernel tests
(test_gpu_lambdarank.py, test_gpu_lambdarank_slab.py).  The reference is
the torch path on CPU tensors, which tests/test_ranking.py pins to the
per-pair oracle.

Tolerance: both sides accumulate in fp64 and cast once to fp32 (2^-24
relative each); fp64 reordering noise at these sizes is below 1e-9 of the
largest entry.  Anything larger is a wrong pair, not rounding."""
import functools

import numpy as np
import torch

from xgboost_amd.backend.gpu import lambdarank_gpair_gpu
from xgboost_amd.data import MetaInfo
from xgboost_amd.objectives import create_objective


def _close(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape
    bound = 2.0 ** -22 * ref.abs() + 1e-9 * ref.abs().max()
    err = (got - ref).abs()
    assert bool((err <= bound).all()), (
        f"max err {float(err.max()):.3e} at {int(err.argmax())}, "
        f"bound there {float(bound.view(-1)[err.argmax()]):.3e}")


class RankCases:
    """`_info`, `_case` and `_kernel` of one test file: its group layout,
    its configuration table, the group that binary labels leave without a
    hit, and whether the kernel call must reach the slab tier."""

    def __init__(self, layout, configs, no_hit, slab):
        self.layout, self.configs = layout, configs
        self.no_hit, self.slab = no_hit, slab
        self._case = functools.lru_cache(maxsize=None)(self._build)

    def _info(self, layout, binary, weights=None, seed=0, no_hit=True):
        rng = np.random.RandomState(seed)
        info = MetaInfo()
        info.num_row = int(sum(layout))
        info.group_ptr = np.concatenate(
            [[0], np.cumsum(layout)]).astype(np.int64)
        y = rng.randint(0, 2 if binary else 5, info.num_row)
        if binary and no_hit and self.no_hit < len(layout):
            y[info.group_ptr[self.no_hit]:info.group_ptr[self.no_hit + 1]] = 0
        info.labels = y.astype(np.float32)
        if weights is not None:
            info.weights = np.asarray(weights, np.float32)
        return info

    def _build(self, obj_name, cfg, ties=False):
        """(info, scores, objective params, CPU reference g and h)."""
        w = (np.random.RandomState(5).uniform(0.5, 2.0, len(self.layout))
             if cfg == "group_weights" else None)
        info = self._info(self.layout, obj_name == "rank:map", w)
        # one decimal: about 70 distinct scores, so ties cross every slab edge
        p = np.random.RandomState(1).randn(info.num_row).round(1)
        p = np.full_like(p, 0.5) if ties else p
        p = torch.tensor(p, dtype=torch.float32).view(-1, 1)
        g, h = create_objective(obj_name, self.configs[cfg]).get_gradient(
            p, info, 0)
        return info, p, self.configs[cfg], g, h

    def _kernel(self, obj_name, params, info, p):
        obj = create_objective(obj_name, params)
        scores = p.cuda().view(-1)
        state = obj._hip_state(scores, info)
        assert state is not None
        if self.slab:
            assert state.slab is not None
        return lambdarank_gpair_gpu(scores, state, obj._hip_metric, obj._k(),
                                    obj.score_norm, obj.normalize,
                                    obj.exp_gain)
