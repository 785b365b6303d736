"""Numpy restatement of the area-averaged point decoder with per-point footprints (include/smoe_hip.h: smoe_sample_area_each)
and the CPU stand-in for ``BlockEngine.sample_area_each`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

The restatement is that of tests/sample_area_engine.py with the per-point statement of the positions: ``blocks.area_taps_each``
(float32 positions of the 64 slots of every point and their validity), ``sample_grad_reference`` on the valid slots (the
existing float32 value restatement), and ``masked_mean`` in the stated order -- over the slots in row-major order an inside tap
adds its value to the sum and one to the count, one division at the end, 0 where no tap is inside (a void point has no valid
slot)."""
import dataclasses

import numpy as np
import torch

from oracle import smoe_oracle as o
from render_engine import NAMES, mask_of
from sample_area_engine import OracleSampleAreaEngine, masked_mean
from sample_grad_engine import sample_grad_reference
from steered_mixture_of_experts_amd import blocks as blk


def sample_area_each_reference(p, active, n, grid, length, points, footprints, taps, blend, ocfg, dtype=np.float32):
    """The cell centres ``points`` [N, d] with ``footprints`` [N, d, d] and ``taps`` [N, d] on the model of all ``prod(grid)``
    blocks.  Returns ``mean`` (N, C) before the lattice, ``count`` (N,), ``block`` (N,) the centre's own block (-1: outside),
    ``void`` (N,) and the slots: ``taps`` (N, 64, d) float32, ``inside`` (N, 64)."""
    T = dtype
    d = len(n)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, d)
    N = pts.shape[0]
    tp, valid = blk.area_taps_each(pts, footprints, taps)
    Cn = p["nu_e"].shape[-1]
    v = np.zeros((N, blk.AREA_TAPS, Cn), T)
    inside = np.zeros((N, blk.AREA_TAPS), bool)
    if valid.any():
        r = sample_grad_reference(p, active, n, grid, length, tp[valid], blend, ocfg, T)
        v[valid] = r["v"]
        inside[valid] = r["inside"]
    mean, cnt = masked_mean(v, inside, T)
    cin, cg, _ = blk.point_blocks(pts, n, grid, length)
    block = np.where(cin, np.ravel_multi_index(tuple(cg[:, l] for l in range(d)), grid), -1)
    return {"mean": mean, "count": cnt, "block": block, "void": blk.area_void_each(footprints, taps), "taps": tp, "inside": inside}


class OracleSampleAreaEachEngine(OracleSampleAreaEngine):
    def sample_area_each(self, params, active, grid, length, points, footprints, taps, blend=None, out=None, dtype=torch.float32,
                         want_mean=False, want_count=False, want_block=False, center_grid=None):
        p = {k: params[k].numpy() for k in NAMES}
        B = int(np.prod(grid))
        d = self.cfg.dim
        assert p["pis"].shape[0] == B, "sample_area_each takes the parameters of all blocks"
        assert points.dim() == 2 and points.shape[1] == d and points.dtype == torch.float32
        N = points.shape[0]
        assert tuple(footprints.shape) == (N, d, d) and footprints.dtype == torch.float32
        assert tuple(taps.shape) == (N, d) and taps.dtype == torch.uint8
        ocfg = self.ocfg if center_grid is None else dataclasses.replace(self.ocfg, mus_grid=center_grid.numpy())
        r = sample_area_each_reference(p, mask_of(active, B, self.cfg.kernels), list(self.cfg.block_shape), list(grid), list(length),
                                       points.numpy(), footprints.numpy(), taps.numpy(), blend, ocfg)
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
