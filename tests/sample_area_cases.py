"""What the CPU and GPU tests of the area-averaged point decoder share: the rotated footprints on the eight cases of
tests/sample_grad_cases.py, and the restatement (tests/sample_area_engine.py) of each, computed once in float32 and float64.
TEST INFRASTRUCTURE."""
import functools

import numpy as np

from sample_area_engine import sample_area_reference
from sample_grad_cases import CASES, case_inputs

LOOSE_CAP = 0.03        # of the covered points; the restatement alone gives at most 2.25e-2 ((7, 5) blocks, blend (2, 1))


def rotated_footprint(i):
    """the footprint and taps of case ``i``"""
    return footprint_of(CASES[i][0], CASES[i][5], CASES[i][6])


def footprint_of(shape, deg, zoom):
    """3 times the linear part of the warp (``deg`` degrees, ``zoom``) on the first two axes, F[2][2] = 1.5; taps (3, 2) /
    (2, 2, 2)"""
    d = len(shape)
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    F = np.zeros((d, d))
    F[:2, :2] = 3.0 * np.array([[c, -s], [s, c]])
    if d == 3:
        F[2, 2] = 1.5
    return F.astype(np.float32), ((2, 2, 2) if d == 3 else (3, 2))


@functools.lru_cache(maxsize=None)
def area_reference(i, blended):
    """(float32, float64) restatement of the case's point set under its rotated footprint; read-only"""
    c = case_inputs(i, blended)
    F, taps = rotated_footprint(i)
    return tuple(sample_area_reference(c["p"], c["active"], c["shape"], c["grid"], c["length"], c["pts"], F, taps, c["beta"],
                                       c["cfg"], T) for T in (np.float32, np.float64))


def loose_of(ref, ref64):
    """a point is loose if any of its taps is loose in either precision"""
    return ref["loose"] | ref64["loose"]
