"""What the CPU and GPU tests of the area-averaged decoder of whole-image models with per-point footprints share: the 13 cases
of tests/shared_sample_grad_cases.py (the five images of tests/test_gpu_shared_render.py and the second one under each of its
eight options), each with its rotated centres and with a TILT -- a projective view of the image, built as
tests/sample_area_each_cases.tilt_matrix builds it (rotation 12 degrees, z = 0.5, horizon at 0.9 E_0) with L = the image shape
-- whose magnification runs from below one source pixel per sample to thousands near its horizon.  The conditions the tests
rely on are asserted on the host.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from shared_sample_engine import point_mapping
from shared_sample_grad_cases import CASES, CASE_IDS  # noqa: F401  (re-exported)
from steered_mixture_of_experts_amd import blocks as blk
from test_gpu_sample import _rotated
from test_gpu_shared_render import _grid, _setup

SSE_POINTS = 64                                     # points per workgroup of the library under test
SSE_TILE = {2: 256, 3: 512}                         # items (taps) per round, by the number of axes (one / two items per lane)
TILT_E = [(56, 84), (56, 84), (44, 56), (24, 32, 5), (40, 48)]     # the tilt's output size per image


def tilt_size(i):
    return TILT_E[i] if i < 5 else TILT_E[1]


@functools.lru_cache(maxsize=None)
def model(i):
    """the model, the lists and the rotated centres of case ``i`` (shared_sample_grad_cases.case without its restatements)"""
    image, E, name, kw = CASES[i]
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, mus_grid = _setup(shape, bshape, C_, kpd, name, **kw)
    pts = _rotated(bshape, _grid(shape, bshape), E, 22.5, 1.7)
    pts.setflags(write=False)
    return dict(shape=shape, bshape=bshape, C=C_, K=K, NB=NB, p=p, cfg=cfg, lists=lists, mus_grid=mus_grid, kw=kw, pts=pts)


def tilt_matrix(i):
    """``H`` [d + 1, d + 1] of case ``i`` and the output size ``E`` (sample_area_each_cases.tilt_matrix with L = the image shape)"""
    shape = CASES[i][0][0]
    d = len(shape)
    L, E = np.array(shape, np.float64), np.array(tilt_size(i), np.float64)
    z, k, a = 0.5, 0.9, np.deg2rad(12.0)
    R = np.eye(d)
    R[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    A = R @ np.diag(z * L / E)
    if d == 3:
        A[2, 2] = L[2] / E[2]
    w = np.zeros(d)
    w[0] = -1.0 / (k * E[0])
    H = np.zeros((d + 1, d + 1))
    H[:d, :d] = A + np.outer(L / 2, w)
    H[:d, d] = -A @ (E / 2) + L / 2
    H[d, :d] = w
    H[d, d] = 1.0
    return H, tuple(int(e) for e in tilt_size(i))


@functools.lru_cache(maxsize=None)
def tilt_inputs(i):
    """The tilt of case ``i`` as lists: ``pts`` [N, d], ``foot`` [N, d, d], ``taps`` uint8 [N, d] (``footprint_taps_each``),
    ``valid`` [N] (False: behind the horizon), the slots ``tp`` [N, 64, d] / ``slot`` [N, 64] of ``area_taps_each``, the taps'
    ``inside`` [N, 64] and batches ``tap_batch`` [N, 64] (-1: outside, or no tap), ``count`` [N] and the centres' ``batch``
    [N].  The conditions on the inputs are asserted here, on the host; read-only."""
    image = CASES[i][0]
    shape, bshape = image[0], image[1]
    d = len(shape)
    H, E = tilt_matrix(i)
    pts, foot, valid = blk.projective_points(H, E)
    pts, foot, valid = pts.reshape(-1, d), foot.reshape(-1, d, d), valid.reshape(-1)
    taps = blk.footprint_taps_each(foot)
    tp, slot = blk.area_taps_each(pts, foot, taps)
    N = len(pts)
    with np.errstate(invalid="ignore"):
        inside, tb, _ = point_mapping(tp.reshape(-1, d), shape, bshape)
        cin, cb, _ = point_mapping(pts, shape, bshape)
    inside = inside.reshape(N, blk.AREA_TAPS) & slot
    tb = np.where(inside, tb.reshape(N, blk.AREA_TAPS), -1)
    count = inside.sum(axis=1)
    ntap = np.where(blk.area_void_each(foot, taps), 0, np.prod(taps.astype(np.int64), axis=1))
    meets = np.array([len(np.unique(b[b >= 0])) for b in tb])
    pad = np.concatenate([ntap, np.zeros(-N % SSE_POINTS, np.int64)]).reshape(-1, SSE_POINTS).sum(axis=1)
    assert len(np.unique(taps[valid], axis=0)) >= 10                         # many tap tuples within the list
    assert (ntap == 64).any()                                                # the longest run of items
    assert (~valid).any() and np.isnan(pts[~valid]).all() and (foot[~valid] == 0).all() and (count[~valid] == 0).all()
    assert (~cin & (count > 0)).any()                                        # a centre outside the image with taps inside
    assert d == 3 or (ntap[valid] == 1).sum() >= 100                         # one-tap points
    assert np.abs(foot).max() > 900.0                                        # footprints far wider than a batch
    assert (meets >= 2).any()                                                # a point whose taps lie in several batches
    assert (pad > SSE_TILE[d]).any()                                           # a workgroup with more items than one round
    out = {"pts": pts, "foot": foot, "taps": taps, "valid": valid, "tp": tp, "slot": slot, "inside": inside, "tap_batch": tb,
           "count": count, "batch": cb, "ntap": ntap}
    for a in out.values():
        a.setflags(write=False)
    out.update(H=H, E=E)
    return out
