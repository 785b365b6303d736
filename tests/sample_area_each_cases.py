"""What the CPU and GPU tests of the area-averaged point decoder with per-point footprints share: the TILT of each of the eight
cases of tests/sample_grad_cases.py -- a projective view of the case's model whose magnification runs from below one source
pixel per sample to thousands near its horizon -- with the conditions the tests rely on asserted on the host, and the three
configurations of the mixed test.  TEST INFRASTRUCTURE.

The tilt of a case.  For the image extent ``L``, the output size ``E = CASES[i][4]``, ``z = 0.5``, a rotation ``R`` by 12 degrees
on the first two axes and ``k = 0.9``: ``A = R diag(z L_l / E_l)`` (on three axes ``A[2][2] = L_2 / E_2``), ``w = (-1 / (k E_0),
0, ..)``, ``w0 = 1``, and ``H[:d, :d] = A + (L / 2) w^T``, ``H[:d, d] = -A (E / 2) + L / 2``, ``H[d] = (w, w0)``: the centre of
the output shows the centre of the image, and the rows from ``0.9 E_0`` on lie behind the horizon."""
import functools

import numpy as np

from sample_area_cases import rotated_footprint
from sample_grad_cases import CASES, case_inputs
from steered_mixture_of_experts_amd import blocks as blk


def tilt_matrix(i):
    """``H`` [d + 1, d + 1] of case ``i`` and the output size ``E``"""
    c = case_inputs(i, False)
    d = len(c["shape"])
    L, E = np.array(c["length"], np.float64), np.array(CASES[i][4], np.float64)
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
    return H, tuple(int(e) for e in CASES[i][4])


@functools.lru_cache(maxsize=None)
def tilt_inputs(i):
    """The tilt of case ``i`` as lists: ``pts`` [N, d], ``foot`` [N, d, d], ``taps`` uint8 [N, d] (``footprint_taps_each``),
    ``valid`` [N] (False: behind the horizon), the slots ``tp`` [N, 64, d] / ``slot`` [N, 64] of ``area_taps_each`` and the
    restatement's ``inside`` [N, 64] and ``count`` [N].  The conditions on the inputs are asserted here, on the host."""
    c = case_inputs(i, False)
    d = len(c["shape"])
    H, E = tilt_matrix(i)
    pts, foot, valid = blk.projective_points(H, E)
    pts, foot, valid = pts.reshape(-1, d), foot.reshape(-1, d, d), valid.reshape(-1)
    taps = blk.footprint_taps_each(foot)
    tp, slot = blk.area_taps_each(pts, foot, taps)
    with np.errstate(invalid="ignore"):
        inside = blk.point_blocks(tp, c["shape"], c["grid"], c["length"])[0] & slot
        cin = blk.point_blocks(pts, c["shape"], c["grid"], c["length"])[0]
    count = inside.sum(axis=1)
    ntap = np.prod(taps.astype(np.int64), axis=1)
    assert 957 <= len(pts) <= 10000
    assert len(np.unique(taps[valid], axis=0)) >= 10                         # many tap tuples within the list
    assert (ntap == 64).any()                                                # the longest trip
    assert (~valid).any() and np.isnan(pts[~valid]).all() and (foot[~valid] == 0).all() and (count[~valid] == 0).all()
    assert (~cin & (count > 0)).any()                                        # a centre outside the image with taps inside
    assert d == 3 or (ntap[valid] == 1).sum() >= 100                         # one-tap points
    assert np.abs(foot).max() > 1000.0                                       # footprints far wider than any box of records
    return {"pts": pts, "foot": foot, "taps": taps, "valid": valid, "tp": tp, "slot": slot, "inside": inside, "count": count,
            "H": H, "E": E}


def mixed_configs(i):
    """the three (footprint, taps) of the mixed test: the case's rotated footprint, a 2-pixel box, half the footprint with one tap"""
    d = len(CASES[i][0])
    F, taps = rotated_footprint(i)
    return [(F, tuple(taps)), (np.diag([2.0] * d).astype(np.float32), (2,) * d), ((np.float32(0.5) * F).astype(np.float32), (1,) * d)]


def each_of(N, F, taps):
    """a footprint and taps broadcast to ``N`` points: float32 [N, d, d], uint8 [N, d]"""
    F = np.asarray(F, np.float32)
    return np.ascontiguousarray(np.broadcast_to(F, (N,) + F.shape)), np.ascontiguousarray(np.broadcast_to(np.asarray(taps, np.uint8), (N, len(taps))))
