"""Numpy restatement of the area-averaged point decoder (include/smoe_hip.h: smoe_sample_area), float32 and float64, and the
CPU stand-in for ``BlockEngine.sample_area`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

The restatement is three lines: ``blocks.area_taps`` (the float32 tap positions), ``sample_grad_reference`` of
tests/sample_grad_engine.py on the taps (their values before the lattice, in the precision asked for), and the masked mean in
the stated order -- over the taps in row-major order an inside tap adds its value to the sum and one to the count, one division
at the end, 0 where no tap is inside.

A point is LOOSE if any of its inside taps is loose in ``sample_grad_reference`` (a gate within 1e-6 of tau, a y within 1e-6 of
0 or 1, a window ratio within 1e-6 of 0 or 1); the tests take the union over the two precisions.  ``floor`` taps (S < 1e-10)
are reported, not exempted, as for the point derivative."""
import dataclasses

import numpy as np
import torch

from oracle import smoe_oracle as o
from render_engine import NAMES, mask_of
from sample_grad_engine import OracleSampleGradEngine, sample_grad_reference
from steered_mixture_of_experts_amd import blocks as blk


def masked_mean(v, inside, T):
    """``v`` (N, taps, C) and ``inside`` (N, taps): the sum over the inside taps in their order, the count, the mean"""
    N, nt, Cn = v.shape
    acc = np.zeros((N, Cn), T)
    cnt = np.zeros((N,), np.int64)
    for t in range(nt):
        acc = np.where(inside[:, t, None], (acc + v[:, t].astype(T)).astype(T), acc)
        cnt += inside[:, t]
    mean = np.where(cnt[:, None] > 0, (acc / np.maximum(cnt, 1).astype(T)[:, None]).astype(T), T(0))
    return mean.astype(T), cnt


def sample_area_reference(p, active, n, grid, length, points, footprint, taps, blend, ocfg, dtype=np.float32):
    """The cell centres ``points`` [N, d] with the common ``footprint`` and ``taps`` on the model of all ``prod(grid)`` blocks.
    Returns ``mean`` (N, C) before the lattice, ``count`` (N,), ``block`` (N,) the centre's own block (-1: outside), ``loose``
    and ``floor`` (N,), and the taps themselves: ``taps`` (N, T, d) float32, ``v`` (N, T, C), ``inside`` (N, T)."""
    T = dtype
    d = len(n)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, d)
    N = pts.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        tp = blk.area_taps(pts, footprint, taps)
    nt = tp.shape[1]
    r = sample_grad_reference(p, active, n, grid, length, tp.reshape(-1, d), blend, ocfg, T)
    Cn = r["v"].shape[1]
    v, inside = r["v"].reshape(N, nt, Cn), r["inside"].reshape(N, nt)
    mean, cnt = masked_mean(v, inside, T)
    cin, cg, _ = blk.point_blocks(pts, n, grid, length)
    block = np.where(cin, np.ravel_multi_index(tuple(cg[:, l] for l in range(d)), grid), -1)
    return {"mean": mean, "count": cnt, "block": block, "loose": (r["loose"].reshape(N, nt) & inside).any(axis=1),
            "floor": (r["floor"].reshape(N, nt) & inside).any(axis=1), "taps": tp, "v": v, "inside": inside}


class OracleSampleAreaEngine(OracleSampleGradEngine):
    def sample_area(self, params, active, grid, length, points, footprint, taps, blend=None, out=None, dtype=torch.float32,
                    want_mean=False, want_count=False, want_block=False, center_grid=None):
        p = {k: params[k].numpy() for k in NAMES}
        B = int(np.prod(grid))
        assert p["pis"].shape[0] == B, "sample_area takes the parameters of all blocks"
        assert points.dim() == 2 and points.shape[1] == self.cfg.dim and points.dtype == torch.float32
        ocfg = self.ocfg if center_grid is None else dataclasses.replace(self.ocfg, mus_grid=center_grid.numpy())
        r = sample_area_reference(p, mask_of(active, B, self.cfg.kernels), list(self.cfg.block_shape), list(grid), list(length),
                                  points.numpy(), footprint, taps, blend, ocfg)
        q = o.fake_quant01(r["mean"], self.cfg.precision, np.float32).astype(np.float32)
        if dtype == torch.uint8:
            q = np.rint(q * (2 ** self.cfg.precision - 1)).astype(np.uint8)
        img = torch.from_numpy(np.ascontiguousarray(q))
        if out is not None:
            out.copy_(img)
            img = out
        res = (img,) + ((torch.from_numpy(np.ascontiguousarray(r["mean"], dtype=np.float32)),) if want_mean else ()) \
            + ((torch.from_numpy(r["count"].astype(np.uint8)),) if want_count else ()) \
            + ((torch.from_numpy(r["block"].astype(np.int32)),) if want_block else ())
        return res if len(res) > 1 else img
