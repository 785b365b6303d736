"""Numpy restatement of the shared-mode point derivative (include/smoe_hip.h: smoe_shared_sample_grad,
smoe_shared_render_view_grad), float32 and float64, and the CPU stand-in for ``SharedEngine.sample_grad`` /
``SharedEngine.render_view_grad`` built on it.  TEST INFRASTRUCTURE, never imported by the product.

Built from ``sample_grad_engine.block_at``: the ONE global kernel set is the model state (``model_state`` with every kernel
listed: fake quantisation, steering matrices, coef with the prior > 0 rule) and ``coef`` is masked per point by the list of the
batch that owns it -- a kernel that is not listed is absent from S, sbar and y alike.  ``shared_sample_engine.point_mapping``
gives the owning batch and the image-unit coordinate.

A point is LOOSE (EDGE = 1e-6, in the arithmetic of the call) if a gate lies within EDGE of tau, or -- where at least one
kernel has influence -- a channel's y lies within EDGE of 0 or 1.  A point with no kernel of influence is NOT loose for its y:
its v and jac are exactly 0 in both precisions (the batch with the empty list alone is 1/24 to 1/6 of the test images).
S < 1e-10 is reported apart as ``floor`` and held to the tight bound, as for the block models."""
import numpy as np
import torch

from oracle import smoe_oracle as o
from sample_grad_engine import EDGE, block_at, model_state
from shared_sample_engine import OracleSharedSampleEngine, point_mapping

CHUNK = 4096                                       # points per block_at call: (CHUNK, K, d, d) temporaries


def _gates(st, u, T):
    """the gates w (M, K) of the points ``u`` on the per-point state ``st`` (leading axis M)"""
    r = u[:, None, :] - st["mu"]
    maha = o._maha(r[:, :, None, :], st["A"], st["ic"])[0][:, :, 0]
    g = st["coef"] * np.exp(T(-0.5) * maha)
    return g / np.maximum(g.sum(axis=1), T(10e-12))[:, None]


def shared_points_grad_reference(p, mask, u, bid, image_shape, ocfg, dtype=np.float32):
    """The points with image-unit coordinates ``u`` (N, d) and global batch ids ``bid`` (N,; -1: outside) on the model ``p``
    (leading axis 1) with the lists ``mask`` (NB, K) of ALL batches.  Returns ``v`` (N, C) the value before the lattice,
    ``jac`` (N, d, C) per source pixel, ``batch`` (N,), ``loose`` and ``floor`` (N,) -- and ``y`` (N, C) before the clip,
    ``wt`` (N, K) the masked gates; v, jac, y, wt are 0 where outside."""
    T = dtype
    u = np.asarray(u)
    N, d = u.shape
    K, Cn = ocfg.kernels, ocfg.channels
    g0 = model_state(p, np.ones((1, K), bool), ocfg, T)            # the one global kernel set, every kernel listed
    du_dx = np.array([T(1) / T(s - 1) if s > 1 else T(0) for s in image_shape], T)
    out = {"v": np.zeros((N, Cn), T), "jac": np.zeros((N, d, Cn), T), "batch": np.asarray(bid).astype(np.int64),
           "loose": np.zeros((N,), bool), "floor": np.zeros((N,), bool), "y": np.zeros((N, Cn), T), "wt": np.zeros((N, K), T)}
    inside = np.flatnonzero(np.asarray(bid) >= 0)
    for s in range(0, inside.size, CHUNK):
        idx = inside[s:s + CHUNK]
        M = idx.size
        st = {k: np.broadcast_to(g0[k], (M,) + g0[k].shape[1:]) for k in ("A", "mu", "nu", "gam")}
        st["coef"] = np.where(mask[bid[idx]], g0["coef"], T(0))    # (M, K): the list of the point's batch
        st.update(ic=g0["ic"], tau=g0["tau"], vmax=g0["vmax"])
        ui = u[idx].astype(T)
        v, dv, wt, edge, floor = block_at(st, np.arange(M), ui, T)
        e = st["nu"] + np.einsum("mklc,ml->mkc", st["gam"], ui)
        out["y"][idx] = np.einsum("mk,mkc->mc", wt, e)
        none = ~(wt > 0).any(axis=1)                               # no kernel of influence: y = 0 exactly, only a gate near
        if none.any():                                             # tau makes such a point loose
            sub = {k: (st[k][none] if k in ("A", "mu", "nu", "gam", "coef") else st[k]) for k in st}
            edge = edge.copy()
            edge[none] = (np.abs(_gates(sub, ui[none], T) - st["tau"]) < EDGE).any(axis=1)
            assert (v[none] == 0).all() and (dv[none] == 0).all()
        out["v"][idx], out["jac"][idx], out["wt"][idx] = v, dv * du_dx[None, :, None], wt
        out["loose"][idx], out["floor"][idx] = edge, floor
    return out


class OracleSharedSampleGradEngine(OracleSharedSampleEngine):
    def _grad(self, params, lists, u, bid, shape, out, want_values, want_batch):
        cfg = self.cfg
        r = shared_points_grad_reference(self._p(params), self._all_lists(lists), u, bid, cfg.image_shape, self.ocfg)
        d = len(cfg.image_shape)
        jac = torch.from_numpy(np.ascontiguousarray(r["jac"], dtype=np.float32).reshape(tuple(shape) + (d, cfg.channels)))
        if out is not None:
            out.copy_(jac)
            jac = out
        val = torch.from_numpy(np.ascontiguousarray(r["v"], dtype=np.float32).reshape(tuple(shape) + (cfg.channels,)))
        bk = torch.from_numpy(r["batch"].astype(np.int32).reshape(tuple(shape)))
        res = (jac,) + ((val,) if want_values else ()) + ((bk,) if want_batch else ())
        return res if len(res) > 1 else jac

    def sample_grad(self, params, lists, points, out=None, want_values=False, want_batch=False):
        cfg = self.cfg
        assert points.dim() == 2 and points.shape[1] == len(cfg.image_shape) and points.dtype == torch.float32
        _, bid, u = point_mapping(points.numpy(), cfg.image_shape, cfg.batch_shape)
        return self._grad(params, lists, u, bid, (points.shape[0],), out, want_values, want_batch)

    def render_view_grad(self, params, lists, axes, batches, out=None, want_values=False, want_batch=False):
        cfg = self.cfg
        grid = [int(s) // int(b) for s, b in zip(cfg.image_shape, cfg.batch_shape)]
        extent = [int(a.numel()) for a in axes]
        assert [int(b.numel()) for b in batches] == extent and all(b.dtype == torch.int32 for b in batches)
        u = np.stack(np.meshgrid(*[a.numpy() for a in axes], indexing="ij"), axis=-1).reshape(-1, len(axes)).astype(np.float32)
        gb = np.meshgrid(*[np.clip(b.numpy().astype(np.int64), 0, g - 1) for b, g in zip(batches, grid)], indexing="ij")
        bid = np.ravel_multi_index(tuple(g.reshape(-1) for g in gb), grid)
        return self._grad(params, lists, u, bid, extent, out, want_values, want_batch)
