"""Numpy restatement of the shared-mode point and viewport decoders (include/smoe_hip.h: smoe_shared_sample,
smoe_shared_render_view) on top of ``oracle.smoe_oracle.forward``, and the CPU stand-in for ``SharedEngine.sample`` /
``SharedEngine.render_view`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

Every point has its own batch and its own image-unit coordinate (``point_mapping`` below: two ``blocks.point_blocks`` calls);
the restatement groups the points by batch and evaluates every group on its point LIST with that batch's kernel list -- the
call ``oracle_shared_batches`` makes for a batch's meshgrid."""
import dataclasses

import numpy as np
import torch

from oracle import smoe_oracle as o
from render_engine import first_max_ids
from shared_render_engine import OracleSharedRenderEngine
from steered_mixture_of_experts_amd import blocks as blk


def point_mapping(points, image_shape, batch_shape):
    """The host statement of smoe_shared_sample's mapping: (inside [N] bool, batch [N] int64 global batch id (-1: outside),
    u [N, d] float32 image-unit coordinates (0 where outside))."""
    d = len(image_shape)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, d)
    grid = [int(s) // int(b) for s, b in zip(image_shape, batch_shape)]
    inside, g, _ = blk.point_blocks(pts, batch_shape, grid, image_shape)
    _, _, u = blk.point_blocks(pts, image_shape, [1] * d, image_shape)
    bid = np.where(inside, np.ravel_multi_index(tuple(g[:, l] for l in range(d)), grid), -1)
    return inside, bid, u


def shared_points_reference(p, mask, u, bid, ocfg, dtype=np.float32):
    """The points with image-unit coordinates ``u`` (N, d) and global batch ids ``bid`` (N,; -1: outside) on the model ``p``
    (leading axis 1) with the lists ``mask`` (NB, K) of ALL batches.  Per point: ``y`` (N, C) before clip and lattice,
    ``recon`` (N, C) on it, ``w`` / ``wt`` (N, K) the gates / masked gates; all 0 where outside."""
    T = dtype
    N, K, Cn = u.shape[0], ocfg.kernels, ocfg.channels
    cfg = dataclasses.replace(ocfg, ssim_opt=False)            # the decoder has no loss
    out = {"y": np.zeros((N, Cn), T), "recon": np.zeros((N, Cn), T), "w": np.zeros((N, K), T), "wt": np.zeros((N, K), T)}
    for b in np.unique(bid[bid >= 0]):
        idx = np.flatnonzero(bid == b)
        xy = np.ascontiguousarray(u[idx], dtype=np.float32)[None]
        f = o.forward(p, np.zeros((1, idx.size, Cn), np.float32), xy, mask[int(b):int(b) + 1], cfg, None, T)
        out["y"][idx], out["recon"][idx] = f["y"][0], f["recon"][0]
        out["w"][idx], out["wt"][idx] = f["w"][0].T, f["wt"][0].T
    return out


def point_ids(wt):
    """(N, K) masked gates -> (N,) first maximum, -1 where no kernel has influence"""
    return first_max_ids(np.moveaxis(wt[None], 2, 1), -1, np.int32)[0]


class OracleSharedSampleEngine(OracleSharedRenderEngine):
    def _all_lists(self, lists):
        if lists is None:
            return np.ones((self.num_batches, self.cfg.kernels), dtype=bool)
        assert tuple(lists.shape) == (self.num_batches, self.list_words), "the lists of ALL batches"
        return self._mask(lists)

    def _dense(self, r, inside, shape, out, dtype, want_argmax):
        q = np.where(inside[:, None], r["recon"], 0).astype(np.float32)
        if dtype == torch.uint8:
            q = np.rint(q * (2 ** self.cfg.precision - 1)).astype(np.uint8)
        img = torch.from_numpy(np.ascontiguousarray(q.reshape(tuple(shape) + (self.cfg.channels,))))
        if out is not None:
            out.copy_(img)
            img = out
        am = np.where(inside, point_ids(r["wt"]), -1).astype(np.int32).reshape(tuple(shape))
        return (img, torch.from_numpy(am)) if want_argmax else img

    def sample(self, params, lists, points, out=None, dtype=torch.float32, want_argmax=False):
        cfg = self.cfg
        assert points.dim() == 2 and points.shape[1] == len(cfg.image_shape) and points.dtype == torch.float32
        inside, bid, u = point_mapping(points.numpy(), cfg.image_shape, cfg.batch_shape)
        r = shared_points_reference(self._p(params), self._all_lists(lists), u, bid, self.ocfg)
        return self._dense(r, inside, (points.shape[0],), out, dtype, want_argmax)

    def render_view(self, params, lists, axes, batches, out=None, dtype=torch.float32, want_argmax=False):
        cfg = self.cfg
        grid = [int(s) // int(b) for s, b in zip(cfg.image_shape, cfg.batch_shape)]
        extent = [int(a.numel()) for a in axes]
        assert [int(b.numel()) for b in batches] == extent and all(b.dtype == torch.int32 for b in batches)
        u = np.stack(np.meshgrid(*[a.numpy() for a in axes], indexing="ij"), axis=-1).reshape(-1, len(axes))
        gb = np.meshgrid(*[np.clip(b.numpy().astype(np.int64), 0, g - 1) for b, g in zip(batches, grid)], indexing="ij")
        bid = np.ravel_multi_index(tuple(g.reshape(-1) for g in gb), grid)
        r = shared_points_reference(self._p(params), self._all_lists(lists), u.astype(np.float32), bid, self.ocfg)
        return self._dense(r, np.ones((u.shape[0],), bool), extent, out, dtype, want_argmax)
