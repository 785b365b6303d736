"""Numpy restatement of the viewport decoder (include/smoe_hip.h: smoe_render_view) on top of ``oracle.smoe_oracle.forward``,
and the CPU stand-in for ``BlockEngine.render_view`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

Every sample has its own block (from the start tables) and its own coordinate (from the coordinate tables): the restatement
walks the blocks of the box that have a non-empty run on every axis and evaluates each on the meshgrid of its runs.  The
blend is restated here for such ragged runs (definition: tests/blend_render_engine.py's header): per block, every
neighbour with weight somewhere on the run is evaluated at its own coordinates of the run's samples."""
import dataclasses
import itertools

import numpy as np
import torch

from blend_render_engine import OracleBlendEngine, axis_weights
from oracle import smoe_oracle as o
from render_engine import NAMES, first_max_ids, mask_of


def view_reference(p, active, n, grid, first, starts, coords, blend, ocfg, dtype=np.float32):
    """The view of ``starts`` / ``coords`` (one table each per axis) on the model of all ``prod(grid)`` blocks.  Returns a
    dict of arrays over the view ``[*E, ...]``: ``v`` (C) before the lattice, ``recon`` (C) on it, ``wt0`` (K) the own block's
    masked gate, ``block`` the image-wide index of the own block, ``banded`` some neighbour weight > 0, ``near_tau`` some
    kernel of a contributing block has its gate within 1e-6 of the threshold, ``nblocks`` blocks left in the sum."""
    T = dtype
    d = len(n)
    B = int(np.prod(grid))
    K, Cn = ocfg.kernels, ocfg.channels
    assert p["pis"].shape[0] == B and active.shape[0] == B
    E = [len(c) for c in coords]
    assert all(int(s[0]) == 0 and int(s[-1]) == e for s, e in zip(starts, E))
    bl = [0.0] * d if blend is None else [float(x) for x in np.atleast_1d(blend)]
    bl = bl * d if len(bl) == 1 else bl
    assert len(bl) == d
    u32 = [np.asarray(c, dtype=np.float32) for c in coords]
    sw = [axis_weights(n[l], u32[l], bl[l], T) for l in range(d)]
    pitch = [np.float32(n[l] / (n[l] - 1)) if n[l] > 1 else np.float32(0) for l in range(d)]
    cfg = dataclasses.replace(ocfg, ssim_opt=False)
    tau = 0.5 / (2 ** ocfg.precision)
    out = {"v": np.zeros(tuple(E) + (Cn,), T), "wt0": np.zeros(tuple(E) + (K,), T), "block": np.full(tuple(E), -1, np.int64),
           "banded": np.zeros(tuple(E), bool), "near_tau": np.zeros(tuple(E), bool), "nblocks": np.zeros(tuple(E), np.int32)}

    def evaluate(b, axes):
        xy = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
        one = {k: p[k][b:b + 1] for k in NAMES}
        f = o.forward(one, np.zeros((1, xy.shape[0], Cn), np.float32), xy, active[b:b + 1], cfg, None, T)
        return f["y"][0], f["wt"][0], (np.abs(f["w"][0] - T(tau)) < 1e-6).any(axis=0)

    for js in itertools.product(*[range(len(s) - 1) for s in starts]):
        sl = tuple(slice(int(starts[l][j]), int(starts[l][j + 1])) for l, j in enumerate(js))
        m = [s.stop - s.start for s in sl]
        if min(m) == 0:
            continue
        g = [int(first[l]) + j for l, j in enumerate(js)]
        b = int(np.ravel_multi_index(g, grid))
        wn, sd = [], []
        for l in range(d):
            shape = [1] * d
            shape[l] = m[l]
            s = np.where(sw[l][sl[l]] > 0, 1, -1)
            exists = (g[l] + s >= 0) & (g[l] + s < grid[l])
            wn.append(np.where(exists, np.abs(sw[l][sl[l]]), T(0)).astype(T).reshape(shape))
            sd.append(s.reshape(shape))
        M = int(np.prod(m))
        num, den = np.zeros((M, Cn), T), np.zeros((M,), T)
        near, cnt = np.zeros((M,), bool), np.zeros((M,), np.int32)
        for corner in itertools.product((0, 1), repeat=d):
            W = np.ones(m, dtype=T)
            for l in range(d):
                W = W * (wn[l] if corner[l] else (T(1) - wn[l]))
            axes_in = [l for l in range(d) if corner[l]]
            for signs in itertools.product((-1, 1), repeat=len(axes_in)):
                delta = [0] * d
                sel = W > 0
                for l, sg in zip(axes_in, signs):
                    delta[l] = sg
                    sel = sel & np.broadcast_to(sd[l] == sg, m)
                if not sel.any():
                    continue
                nb = int(np.ravel_multi_index([g[l] + delta[l] for l in range(d)], grid))
                y, wt, nt = evaluate(nb, [(u32[l][sl[l]] - np.float32(delta[l]) * pitch[l]).astype(np.float32) for l in range(d)])
                idx = np.flatnonzero(sel.reshape(-1))
                use = wt.max(axis=0)[idx] > 0
                Wv = W.reshape(-1)[idx]
                num[idx] += np.where(use[:, None], Wv[:, None] * np.clip(y[idx], T(0), T(1)), T(0))
                den[idx] += np.where(use, Wv, T(0))
                near[idx] |= nt[idx]
                cnt[idx] += use
                if not any(delta):
                    out["wt0"][sl] = wt.T.reshape(tuple(m) + (K,))
        out["v"][sl] = np.where(den[:, None] > 0, num / np.where(den > 0, den, T(1))[:, None], T(0)).astype(T).reshape(tuple(m) + (Cn,))
        out["block"][sl] = b
        out["banded"][sl] = np.broadcast_to(sum((w > 0) for w in wn) > 0, m)
        out["near_tau"][sl] = near.reshape(m)
        out["nblocks"][sl] = cnt.reshape(m)
    assert (out["block"] >= 0).all()                         # every position of the view has a block
    out["recon"] = o.fake_quant01(out["v"], ocfg.precision, T)
    return out


class OracleViewEngine(OracleBlendEngine):
    def render_view(self, params, active, grid, view_first, starts, axes, blend=None, out=None, dtype=torch.float32,
                    want_argmax=False, center_grid=None):
        p = {k: params[k].numpy() for k in NAMES}
        B = int(np.prod(grid))
        assert p["pis"].shape[0] == B, "render_view takes the parameters of all blocks"
        r = view_reference(p, mask_of(active, B, self.cfg.kernels), list(self.cfg.block_shape), list(grid), list(view_first),
                           [np.asarray(s) for s in starts], [a.numpy() for a in axes], blend, self.ocfg)
        q = r["recon"].astype(np.float32)
        if dtype == torch.uint8:
            q = np.rint(q * (2 ** self.cfg.precision - 1)).astype(np.uint8)
        img = torch.from_numpy(np.ascontiguousarray(q))
        if out is not None:
            out.copy_(img)
            img = out
        E = r["block"].shape
        am = first_max_ids(np.moveaxis(r["wt0"].reshape(1, -1, self.cfg.kernels), 2, 1), 255, np.uint8).reshape(E)
        return (img, torch.from_numpy(am)) if want_argmax else img
