"""The CPU stand-in for ``SharedEngine.sample_area_each`` (include/smoe_hip.h: smoe_shared_sample_area_each), built on the
numpy restatement of smoe_shared_sample_area (tests/shared_sample_area_engine.py): the specification is "the result for a point
is that of smoe_shared_sample_area called with that one point, its footprint and its taps", so the stand-in calls
``shared_sample_area_reference`` once per distinct (footprint, taps) pair on the points that carry it, and applies the void rule
(``blocks.area_void_each``): 0 / 0 / count 0, the batch still the centre's.  TEST INFRASTRUCTURE, never imported by the product."""
import numpy as np
import torch

from oracle import smoe_oracle as o
from shared_sample_area_engine import OracleSharedSampleAreaEngine, shared_sample_area_reference
from shared_sample_engine import point_mapping
from steered_mixture_of_experts_amd import blocks as blk


def shared_sample_area_each_reference(p, mask, image_shape, batch_shape, points, footprints, taps, ocfg, dtype=np.float32):
    """``mean`` (N, C), ``count`` (N,), ``batch`` (N,) of the centres ``points`` [N, d] with ``footprints`` [N, d, d] and
    ``taps`` uint8 [N, d]"""
    d = len(image_shape)
    pts = np.asarray(points, np.float32).reshape(-1, d)
    foot = np.asarray(footprints, np.float32).reshape(-1, d, d)
    tp = np.asarray(taps, np.uint8).reshape(-1, d)
    N, Cn = pts.shape[0], ocfg.channels
    mean, count = np.zeros((N, Cn), dtype), np.zeros((N,), np.int64)
    with np.errstate(invalid="ignore"):
        _, batch, _ = point_mapping(pts, image_shape, batch_shape)
    void = blk.area_void_each(foot, tp)
    key = np.concatenate([foot.reshape(N, d * d).view(np.uint32), tp.astype(np.uint32)], axis=1)
    live = np.flatnonzero(~void)
    if live.size:
        _, inv = np.unique(key[live], axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        for g in range(int(inv.max()) + 1):
            idx = live[inv == g]
            r = shared_sample_area_reference(p, mask, image_shape, batch_shape, pts[idx], foot[idx[0]], [int(v) for v in tp[idx[0]]],
                                             ocfg, dtype)
            mean[idx], count[idx] = r["mean"], r["count"]
    return {"mean": mean, "count": count, "batch": batch, "void": void}


class OracleSharedSampleAreaEachEngine(OracleSharedSampleAreaEngine):
    def sample_area_each(self, params, lists, points, footprints, taps, out=None, dtype=torch.float32, want_mean=False,
                         want_count=False, want_batch=False):
        cfg = self.cfg
        d = len(cfg.image_shape)
        N = points.shape[0]
        assert points.dim() == 2 and points.shape[1] == d and points.dtype == torch.float32
        assert tuple(footprints.shape) == (N, d, d) and footprints.dtype == torch.float32 and footprints.is_contiguous()
        assert tuple(taps.shape) == (N, d) and taps.dtype == torch.uint8 and taps.is_contiguous()
        r = shared_sample_area_each_reference(self._p(params), self._all_lists(lists), list(cfg.image_shape), list(cfg.batch_shape),
                                              points.numpy(), footprints.numpy(), taps.numpy(), self.ocfg)
        q = o.fake_quant01(r["mean"], cfg.precision, np.float32).astype(np.float32)
        if dtype == torch.uint8:
            q = np.rint(q * (2 ** cfg.precision - 1)).astype(np.uint8)
        img = torch.from_numpy(np.ascontiguousarray(q))
        if out is not None:
            out.copy_(img)
            img = out
        res = (img,) + ((torch.from_numpy(np.ascontiguousarray(r["mean"], dtype=np.float32)),) if want_mean else ()) \
            + ((torch.from_numpy(r["count"].astype(np.uint8)),) if want_count else ()) \
            + ((torch.from_numpy(r["batch"].astype(np.int32)),) if want_batch else ())
        return res if len(res) > 1 else img
