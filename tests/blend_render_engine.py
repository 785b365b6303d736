"""Numpy restatement of the seam-free decoder (include/smoe_hip.h: smoe_render_blend) on top of ``oracle.smoe_oracle.forward``,
and the CPU stand-in for ``BlockEngine.render_blend`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

Definition, per axis ``l`` with ``n`` fitted pixels per block, ``u`` the block-unit coordinate of a local sample and
``b = blend / (n - 1)``: the block at ``g + 1`` gets ``w_hi = clamp(0.5 (1 + (u - s1) / b), 0, 1)``, the block at ``g - 1``
``w_lo = clamp(0.5 (1 + (s0 - u) / b), 0, 1)`` (``s0 = -0.5 / (n - 1)``, ``s1 = 1 + 0.5 / (n - 1)``), a block outside the image
0, the own block ``1 - w_lo - w_hi``.  ``W`` of a block = product over the axes.  A block with ``W > 0`` is evaluated at its own
coordinate of the sample (fp32 ``u - P`` seen from ``g + 1``, ``u + P`` from ``g - 1``, ``P = n / (n - 1)``); blocks without a
kernel of influence are dropped; ``v = sum W clip(y, 0, 1) / sum W`` (0 if none is left), quantised once."""
import dataclasses
import itertools

import numpy as np
import torch

from oracle import smoe_oracle as o
from render_engine import NAMES, OracleRenderEngine, decoded, mask_of


def axis_weights(n, tab, beta, T=np.float32):
    """Signed neighbour weight per local sample of one axis: > 0 towards block g + 1, < 0 towards g - 1, 0 none."""
    u = np.asarray(tab, dtype=np.float32).astype(T)
    if n < 2 or float(beta) <= 0:
        return np.zeros(u.shape, dtype=T)
    s0, s1, b = T(-0.5 / (n - 1)), T(1 + 0.5 / (n - 1)), T(float(np.float32(beta)) / (n - 1))
    hi = np.clip(T(0.5) * (T(1) + (u - s1) / b), T(0), T(1))
    lo = np.clip(T(0.5) * (T(1) + (s0 - u) / b), T(0), T(1))
    return np.where(hi > 0, hi, -lo).astype(T)


def blend_reference(p, active, tabs, n, grid, blend, ocfg, dtype=np.float32):
    """All ``prod(grid)`` blocks on the meshgrid of ``tabs``.  Returns a dict: ``v`` (B, M, C) before the lattice, ``recon``
    (B, M, C) on it, ``wt0`` (B, K, M) the own block's masked gate, ``banded`` (B, M) some neighbour weight > 0,
    ``near_tau`` (B, M) some kernel of a contributing block has its gate within 1e-6 of the threshold, ``nblocks`` (B, M) the
    number of blocks left in the sum."""
    T = dtype
    d = len(n)
    B = int(np.prod(grid))
    assert p["pis"].shape[0] == B and active.shape[0] == B
    m = [len(t) for t in tabs]
    M = int(np.prod(m))
    bl = [float(v) for v in np.atleast_1d(blend)]
    bl = bl * d if len(bl) == 1 else bl
    assert len(bl) == d
    sw = [axis_weights(n[l], tabs[l], bl[l], T) for l in range(d)]
    u32 = [np.asarray(t, dtype=np.float32) for t in tabs]
    pitch = [np.float32(n[l] / (n[l] - 1)) if n[l] > 1 else np.float32(0) for l in range(d)]
    cfg = dataclasses.replace(ocfg, ssim_opt=False)
    zeros = np.zeros((B, M, ocfg.channels), dtype=np.float32)
    tau = 0.5 / (2 ** ocfg.precision)
    # view delta: every block evaluated at the coordinates under which the samples of block (g - delta) see it
    views = {}
    needed = [sorted({0} | {int(s) for s in np.sign(sw[l])}) for l in range(d)]
    for delta in itertools.product(*needed):
        ax = [(u32[l] - np.float32(delta[l]) * pitch[l]).astype(np.float32) for l in range(d)]
        coords = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, d)
        f = o.forward(p, zeros, coords, active, cfg, None, T)
        views[delta] = (f["y"], f["wt"].max(axis=1) > 0, (np.abs(f["w"] - T(tau)) < 1e-6).any(axis=1), f["wt"])
    num = np.zeros((B, M, ocfg.channels), dtype=T)
    den = np.zeros((B, M), dtype=T)
    near = np.zeros((B, M), dtype=bool)
    cnt = np.zeros((B, M), dtype=np.int32)
    banded = np.zeros((B, M), dtype=bool)
    sample = np.arange(M).reshape(m)
    for blk in range(B):
        g = np.unravel_index(blk, grid)
        wn, sd = [], []
        for l in range(d):
            shape = [1] * d
            shape[l] = m[l]
            s = np.where(sw[l] > 0, 1, -1)
            exists = (g[l] + s >= 0) & (g[l] + s < grid[l])
            wn.append(np.where(exists, np.abs(sw[l]), T(0)).astype(T).reshape(shape))
            sd.append(s.reshape(shape))
        banded[blk] = np.broadcast_to(sum((w > 0) for w in wn) > 0, m).reshape(-1)
        for corner in itertools.product((0, 1), repeat=d):
            W = np.ones(m, dtype=T)
            for l in range(d):
                W = W * (wn[l] if corner[l] else (T(1) - wn[l]))
            if not (W > 0).any():
                continue
            axes_in = [l for l in range(d) if corner[l]]
            for signs in itertools.product((-1, 1), repeat=len(axes_in)):
                delta = [0] * d
                sel = W > 0
                for l, sg in zip(axes_in, signs):
                    delta[l] = sg
                    sel = sel & np.broadcast_to(sd[l] == sg, m)
                delta = tuple(delta)
                if not sel.any():
                    continue
                nbr = tuple(g[l] + delta[l] for l in range(d))
                nb = int(np.ravel_multi_index(nbr, grid))
                y, has, nt, _ = views[delta]
                idx = sample[sel]
                use = has[nb, idx]
                Wv = W[sel]
                num[blk, idx] += np.where(use[:, None], Wv[:, None] * np.clip(y[nb, idx], T(0), T(1)), T(0))
                den[blk, idx] += np.where(use, Wv, T(0))
                near[blk, idx] |= nt[nb, idx]
                cnt[blk, idx] += use
    v = np.where(den[..., None] > 0, num / np.where(den > 0, den, T(1))[..., None], T(0)).astype(T)
    return {"v": v, "recon": o.fake_quant01(v, ocfg.precision, T), "wt0": views[(0,) * d][3], "banded": banded,
            "near_tau": near, "nblocks": cnt}


class OracleBlendEngine(OracleRenderEngine):
    def render_blend(self, params, active, axes, grid, extent, blend, first_block=0, num_blocks=None, out=None,
                     dtype=torch.float32, want_argmax=False, center_grid=None):
        p = {k: params[k].numpy() for k in NAMES}
        B = p["pis"].shape[0]
        assert B == int(np.prod(grid)), "render_blend takes the parameters of all blocks"
        count = B - first_block if num_blocks is None else int(num_blocks)
        f = None
        if count > 0:
            r = blend_reference(p, mask_of(active, B, self.cfg.kernels), [a.numpy() for a in axes], list(self.cfg.block_shape),
                                list(grid), blend, self.ocfg)
            f = (r["recon"][first_block:first_block + count], r["wt0"][first_block:first_block + count])
        return decoded(f, [int(a.numel()) for a in axes], grid, extent, first_block, self.cfg, out, dtype, 255, np.uint8, want_argmax)
