"""Numpy restatement of the area-averaged decoder of whole-image models (include/smoe_hip.h: smoe_shared_sample_area),
float32 and float64, and the CPU stand-in for ``SharedEngine.sample_area`` built on it.  TEST INFRASTRUCTURE, never imported
by the product.

The restatement composes four existing statements: ``blocks.area_taps`` (the float32 tap positions),
``shared_sample_engine.point_mapping`` on the taps (every tap's OWN batch and image-unit coordinate),
``shared_points_grad_reference`` of tests/shared_sample_grad_engine.py for the taps' values before the lattice in the precision
asked for, and ``sample_area_engine.masked_mean`` -- over the taps in row-major order an inside tap adds its value to the sum
and one to the count, one division at the end, 0 where no tap is inside.  The centre's batch is ``point_mapping`` on the
centres.

A point is LOOSE if any of its inside taps is loose in ``shared_points_grad_reference``; the tests take the union over the two
precisions."""
import numpy as np
import torch

from oracle import smoe_oracle as o
from sample_area_engine import masked_mean
from shared_sample_engine import point_mapping
from shared_sample_grad_engine import OracleSharedSampleGradEngine, shared_points_grad_reference
from steered_mixture_of_experts_amd import blocks as blk


def shared_sample_area_reference(p, mask, image_shape, batch_shape, points, footprint, taps, ocfg, dtype=np.float32):
    """The cell centres ``points`` [N, d] with the common ``footprint`` and ``taps`` on the model ``p`` (leading axis 1) with
    the lists ``mask`` (NB, K) of ALL batches.  Returns ``mean`` (N, C) before the lattice, ``count`` (N,), ``batch`` (N,) the
    batch that owns the centre (-1: outside), ``loose`` and ``floor`` (N,), and the taps themselves: ``taps`` (N, T, d)
    float32, ``v`` (N, T, C), ``inside`` (N, T), ``tap_batch`` (N, T)."""
    T = dtype
    d = len(image_shape)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, d)
    N = pts.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        tp = blk.area_taps(pts, footprint, taps)
    nt = tp.shape[1]
    inside, bid, u = point_mapping(tp.reshape(-1, d), image_shape, batch_shape)
    r = shared_points_grad_reference(p, mask, u, bid, image_shape, ocfg, T)
    Cn = r["v"].shape[1]
    v, inside = r["v"].reshape(N, nt, Cn), inside.reshape(N, nt)
    mean, cnt = masked_mean(v, inside, T)
    _, cbid, _ = point_mapping(pts, image_shape, batch_shape)
    return {"mean": mean, "count": cnt, "batch": cbid, "loose": (r["loose"].reshape(N, nt) & inside).any(axis=1),
            "floor": (r["floor"].reshape(N, nt) & inside).any(axis=1), "taps": tp, "v": v, "inside": inside,
            "tap_batch": bid.reshape(N, nt)}


class OracleSharedSampleAreaEngine(OracleSharedSampleGradEngine):
    def sample_area(self, params, lists, points, footprint, taps, out=None, dtype=torch.float32, want_mean=False,
                    want_count=False, want_batch=False):
        cfg = self.cfg
        assert points.dim() == 2 and points.shape[1] == len(cfg.image_shape) and points.dtype == torch.float32
        r = shared_sample_area_reference(self._p(params), self._all_lists(lists), list(cfg.image_shape), list(cfg.batch_shape),
                                         points.numpy(), footprint, taps, self.ocfg)
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
