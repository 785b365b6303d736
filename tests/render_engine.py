"""CPU stand-in for ``BlockEngine.render``: tests/fake_engine.py's engine plus ``render`` evaluated with the numpy
restatement (oracle.smoe_oracle.forward) on the resampled coordinates.  TEST INFRASTRUCTURE, never imported by the product."""
import dataclasses

import numpy as np
import torch

from fake_engine import NAMES, OracleEngine
from oracle import smoe_oracle as o


def oracle_blocks(p, active, axes, ocfg, dtype=np.float32):
    """Evaluate B blocks on the meshgrid of the per-axis tables: dict of oracle.forward with ``coords`` (M, d)."""
    coords = np.stack(np.meshgrid(*[np.asarray(a, dtype=np.float32) for a in axes], indexing="ij"), axis=-1)
    coords = coords.reshape(-1, len(axes))
    B = p["pis"].shape[0]
    cfg = dataclasses.replace(ocfg, ssim_opt=False)            # the decoder has no loss
    zeros = np.zeros((B, coords.shape[0], ocfg.channels), dtype=np.float32)
    return o.forward(p, zeros, coords, active, cfg, None, dtype), coords


def place_blocks(vals, m, grid, extent, first_block, out):
    """vals (B, prod(m), X) -> out[*extent, X] at the blocks' places (row-major grid, last axis innermost)."""
    d = len(m)
    for b in range(vals.shape[0]):
        g = np.unravel_index(first_block + b, grid)
        blk = vals[b].reshape(tuple(m) + vals.shape[2:])
        src, dst = [], []
        for l in range(d):
            lo = g[l] * m[l]
            n = max(0, min(m[l], extent[l] - lo))
            src.append(slice(0, n))
            dst.append(slice(lo, lo + n))
        out[tuple(dst)] = blk[tuple(src)]
    return out


class OracleRenderEngine(OracleEngine):
    def render(self, params, active, axes, grid, extent, first_block=0, out=None, dtype=torch.float32, want_argmax=False):
        K, Cc = self.cfg.kernels, self.cfg.channels
        p = {k: params[k].numpy() for k in NAMES}
        B = p["pis"].shape[0]
        if active is None:
            mask = np.ones((B, K), dtype=bool)
        else:
            act = active.numpy().view(np.uint32)
            mask = ((act[:, None] >> np.arange(K, dtype=np.uint32)[None, :]) & 1).astype(bool)
        m = [int(a.numel()) for a in axes]
        extent = [int(e) for e in extent]
        img = np.zeros(tuple(extent) + (Cc,), dtype=np.float32) if out is None else out.numpy()
        am = np.full(tuple(extent), 255, dtype=np.uint8)
        if B > 0:
            f, _ = oracle_blocks(p, mask, [a.numpy() for a in axes], self.ocfg)
            q = f["recon"].astype(np.float32)
            if dtype == torch.uint8:
                q = np.rint(q * (2 ** self.cfg.precision - 1)).astype(np.uint8)
                if out is None:
                    img = img.astype(np.uint8)
            place_blocks(q, m, grid, extent, first_block, img)
            wt = f["wt"]                                                       # (B, K, M)
            arg = np.where(wt.max(axis=1) > 0, np.argmax(wt, axis=1), 255).astype(np.uint8)
            place_blocks(arg[..., None], m, grid, extent, first_block, am[..., None])
        elif dtype == torch.uint8 and out is None:
            img = img.astype(np.uint8)
        res = torch.from_numpy(img) if out is None else out
        return (res, torch.from_numpy(am)) if want_argmax else res
