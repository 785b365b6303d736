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


def mask_of(words, n, K):
    """(n, K) bool from the bit words of ``n`` kernel lists ((n,) or (n, KW) int32 tensor; None: every kernel listed)."""
    if words is None:
        return np.ones((n, K), dtype=bool)
    w = words.numpy().view(np.uint32).reshape(n, -1)
    k = np.arange(K)
    return ((w[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)


def first_max_ids(wt, none, dtype):
    """(n, K, M) masked gates -> (n, M) first maximum, ``none`` where no kernel has influence"""
    return np.where(wt.max(axis=1) > 0, np.argmax(wt, axis=1), none).astype(dtype)


def decoded(f, m, grid, extent, first, cfg, out, dtype, none, id_dtype, want_argmax):
    """What a stand-in's ``render`` returns for the restatement's result ``f`` = (recon (n, M, C), wt (n, K, M)) of the blocks
    from ``first`` on (None: nothing was rendered): the image -- ``out``, or a new one of zeros -- in ``dtype`` and the
    kernel-id map, ``none`` where no kernel has influence or nothing was rendered."""
    extent = [int(e) for e in extent]
    img = out.numpy() if out is not None else np.zeros(tuple(extent) + (cfg.channels,), np.uint8 if dtype == torch.uint8 else np.float32)
    am = np.full(tuple(extent), none, dtype=id_dtype)
    if f is not None:
        q = f[0].astype(np.float32)
        if dtype == torch.uint8:
            q = np.rint(q * (2 ** cfg.precision - 1)).astype(np.uint8)
        place_blocks(q, m, grid, extent, first, img)
        place_blocks(first_max_ids(f[1], none, id_dtype)[..., None], m, grid, extent, first, am[..., None])
    res = torch.from_numpy(img) if out is None else out
    return (res, torch.from_numpy(am)) if want_argmax else res


class OracleRenderEngine(OracleEngine):
    def render(self, params, active, axes, grid, extent, first_block=0, out=None, dtype=torch.float32, want_argmax=False):
        p = {k: params[k].numpy() for k in NAMES}
        B = p["pis"].shape[0]
        f = None
        if B > 0:
            r, _ = oracle_blocks(p, mask_of(active, B, self.cfg.kernels), [a.numpy() for a in axes], self.ocfg)
            f = (r["recon"], r["wt"])
        return decoded(f, [int(a.numel()) for a in axes], grid, extent, first_block, self.cfg, out, dtype, 255, np.uint8, want_argmax)
