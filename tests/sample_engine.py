"""Numpy restatement of the point decoder (include/smoe_hip.h: smoe_sample) on top of ``oracle.smoe_oracle.forward``, and the
CPU stand-in for ``BlockEngine.sample`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

Every point has its own block and its own coordinate (``blocks.point_blocks``): the restatement groups the points by own
block and evaluates the own block and, with blend, every neighbour with weight on some point of the group on the group's point
LIST (no meshgrid).  The blend is the one of tests/blend_render_engine.py's header."""
import dataclasses
import itertools

import numpy as np
import torch

from blend_render_engine import axis_weights
from oracle import smoe_oracle as o
from render_engine import NAMES, first_max_ids, mask_of
from steered_mixture_of_experts_amd import blocks as blk
from view_render_engine import OracleViewEngine


def sample_reference(p, active, n, grid, length, points, blend, ocfg, dtype=np.float32):
    """The points ``[N, d]`` on the model of all ``prod(grid)`` blocks.  Returns what ``view_reference`` returns, per point:
    ``v`` (N, C) before the lattice, ``recon`` (N, C) on it, ``wt0`` (N, K) the own block's masked gate, ``block`` (N,) the
    image-wide index of the own block (-1: outside; everything else is 0 / False there), ``banded`` some neighbour weight > 0,
    ``near_tau`` some kernel of a contributing block has its gate within 1e-6 of the threshold, ``nblocks`` blocks left in the
    sum."""
    T = dtype
    d = len(n)
    B = int(np.prod(grid))
    K, Cn = ocfg.kernels, ocfg.channels
    assert p["pis"].shape[0] == B and active.shape[0] == B
    pts = np.asarray(points, dtype=np.float32).reshape(-1, d)
    N = pts.shape[0]
    inside, gidx, u = blk.point_blocks(pts, n, grid, length)
    bl = [0.0] * d if blend is None else [float(x) for x in np.atleast_1d(blend)]
    bl = bl * d if len(bl) == 1 else bl
    assert len(bl) == d
    sw = [axis_weights(n[l], u[:, l], bl[l], T) for l in range(d)]
    pitch = [np.float32(n[l] / (n[l] - 1)) if n[l] > 1 else np.float32(0) for l in range(d)]
    cfg = dataclasses.replace(ocfg, ssim_opt=False)
    tau = 0.5 / (2 ** ocfg.precision)
    out = {"v": np.zeros((N, Cn), T), "wt0": np.zeros((N, K), T), "block": np.full((N,), -1, np.int64),
           "banded": np.zeros((N,), bool), "near_tau": np.zeros((N,), bool), "nblocks": np.zeros((N,), np.int32)}
    ids = np.where(inside, np.ravel_multi_index(tuple(gidx[:, l] for l in range(d)), grid), -1)

    def evaluate(b, xy):
        one = {k: p[k][b:b + 1] for k in NAMES}
        f = o.forward(one, np.zeros((1, xy.shape[0], Cn), np.float32), np.ascontiguousarray(xy, dtype=np.float32),
                      active[b:b + 1], cfg, None, T)
        return f["y"][0], f["wt"][0], (np.abs(f["w"][0] - T(tau)) < 1e-6).any(axis=0)

    for b in np.unique(ids[inside]):
        idx = np.flatnonzero(ids == b)
        g = np.unravel_index(int(b), grid)
        M = idx.size
        wn, sd = [], []
        for l in range(d):
            s = np.where(sw[l][idx] > 0, 1, -1)
            exists = (g[l] + s >= 0) & (g[l] + s < grid[l])
            wn.append(np.where(exists, np.abs(sw[l][idx]), T(0)).astype(T))
            sd.append(s)
        num, den = np.zeros((M, Cn), T), np.zeros((M,), T)
        near, cnt = np.zeros((M,), bool), np.zeros((M,), np.int32)
        for corner in itertools.product((0, 1), repeat=d):
            W = np.ones((M,), dtype=T)
            for l in range(d):
                W = W * (wn[l] if corner[l] else (T(1) - wn[l]))
            axes_in = [l for l in range(d) if corner[l]]
            for signs in itertools.product((-1, 1), repeat=len(axes_in)):
                delta = [0] * d
                sel = W > 0
                for l, sg in zip(axes_in, signs):
                    delta[l] = sg
                    sel = sel & (sd[l] == sg)
                own = not any(delta)
                sub = np.arange(M) if own else np.flatnonzero(sel)       # the own block is evaluated on every point: wt0
                if sub.size == 0:
                    continue
                nb = int(np.ravel_multi_index([g[l] + delta[l] for l in range(d)], grid))
                xy = np.stack([(u[idx[sub], l] - np.float32(delta[l]) * pitch[l]).astype(np.float32) for l in range(d)], axis=-1)
                y, wt, nt = evaluate(nb, xy)
                use = (wt.max(axis=0) > 0) & sel[sub]
                Wv = W[sub]
                num[sub] += np.where(use[:, None], Wv[:, None] * np.clip(y, T(0), T(1)), T(0))
                den[sub] += np.where(use, Wv, T(0))
                near[sub] |= nt & sel[sub]
                cnt[sub] += use
                if own:
                    out["wt0"][idx] = wt.T
        out["v"][idx] = np.where(den[:, None] > 0, num / np.where(den > 0, den, T(1))[:, None], T(0)).astype(T)
        out["block"][idx] = b
        out["banded"][idx] = sum((w > 0) for w in wn) > 0
        out["near_tau"][idx] = near
        out["nblocks"][idx] = cnt
    out["recon"] = o.fake_quant01(out["v"], ocfg.precision, T)
    return out


class OracleSampleEngine(OracleViewEngine):
    def sample(self, params, active, grid, length, points, blend=None, out=None, dtype=torch.float32, want_argmax=False,
               want_block=False, center_grid=None):
        p = {k: params[k].numpy() for k in NAMES}
        B = int(np.prod(grid))
        assert p["pis"].shape[0] == B, "sample takes the parameters of all blocks"
        assert points.dim() == 2 and points.shape[1] == self.cfg.dim and points.dtype == torch.float32
        r = sample_reference(p, mask_of(active, B, self.cfg.kernels), list(self.cfg.block_shape), list(grid), list(length),
                             points.numpy(), blend, self.ocfg)
        q = r["recon"].astype(np.float32)
        if dtype == torch.uint8:
            q = np.rint(q * (2 ** self.cfg.precision - 1)).astype(np.uint8)
        img = torch.from_numpy(np.ascontiguousarray(q))
        if out is not None:
            out.copy_(img)
            img = out
        N = q.shape[0]
        am = first_max_ids(np.moveaxis(r["wt0"].reshape(1, N, self.cfg.kernels), 2, 1), 255, np.uint8).reshape(N)
        res = (img,) + ((torch.from_numpy(am),) if want_argmax else ()) + ((torch.from_numpy(r["block"].astype(np.int32)),) if want_block else ())
        return res if len(res) > 1 else img
