"""CPU stand-in for ``SharedEngine.render``: tests/fake_engine.py's shared engine plus ``render`` evaluated with the numpy
restatement (oracle.smoe_oracle.forward with one global parameter set, per-batch coordinates and per-batch lists -- the
call ``shared_pass`` makes) on the resampled coordinates.  TEST INFRASTRUCTURE, never imported by the product."""
import dataclasses

import numpy as np
import torch

from fake_engine import OracleSharedEngine
from oracle import smoe_oracle as o
from render_engine import decoded, first_max_ids


def batch_sample_coords(tabs, m, grid, first, nb):
    """(nb, prod(m), d) coordinates of the samples of the batches [first, first + nb): batch (g_0, ..) owns the entries
    [g_l * m_l, (g_l + 1) * m_l) of the image-wide per-axis tables."""
    out = []
    for b in range(first, first + nb):
        g = np.unravel_index(b, grid)
        sub = [np.asarray(t)[gl * ml:(gl + 1) * ml] for t, gl, ml in zip(tabs, g, m)]
        out.append(np.stack(np.meshgrid(*sub, indexing="ij"), axis=-1).reshape(-1, len(m)))
    return np.stack(out) if out else np.zeros((0, int(np.prod(m)), len(m)), np.float32)


def oracle_shared_batches(p, mask, tabs, m, grid, first, ocfg, dtype=np.float32):
    """oracle.forward of the batches [first, first + mask.shape[0]) on their samples.  p: leading axis 1; mask (nb, K)."""
    nb = mask.shape[0]
    coords = batch_sample_coords([np.asarray(t, dtype=np.float32) for t in tabs], m, grid, first, nb)
    cfg = dataclasses.replace(ocfg, ssim_opt=False)            # the decoder has no loss
    zeros = np.zeros((nb, coords.shape[1], ocfg.channels), dtype=np.float32)
    return o.forward(o._bcast(p, nb), zeros, coords, mask, cfg, None, dtype)


def ids_of(wt):
    """(nb, K, M) masked gates -> (nb, M) first maximum, -1 where no kernel has influence"""
    return first_max_ids(wt, -1, np.int32)


class OracleSharedRenderEngine(OracleSharedEngine):
    def render(self, params, lists, axes, samples, first_batch=0, out=None, dtype=torch.float32, want_argmax=False,
               num_batches=None):
        cfg = self.cfg
        m = [int(v) for v in samples]
        grid = [int(s) // int(b) for s, b in zip(cfg.image_shape, cfg.batch_shape)]
        extent = [g * v for g, v in zip(grid, m)]
        assert [int(a.numel()) for a in axes] == extent
        if lists is None:
            nb = self.num_batches - first_batch if num_batches is None else int(num_batches)
            mask = np.ones((nb, cfg.kernels), dtype=bool)
        else:
            nb = int(lists.shape[0])
            mask = self._mask(lists)
        f = None
        if nb > 0:
            r = oracle_shared_batches(self._p(params), mask, [a.numpy() for a in axes], m, grid, first_batch, self.ocfg)
            f = (r["recon"], r["wt"])
        return decoded(f, m, grid, extent, first_batch, cfg, out, dtype, -1, np.int32, want_argmax)
