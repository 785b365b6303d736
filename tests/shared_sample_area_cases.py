"""What the CPU and GPU tests of the area-averaged decoder of whole-image models share: the 13 parity cases of
tests/shared_sample_grad_cases.py with the same rotated centres, under a rotated footprint of
tests/sample_area_cases.rotated_footprint's form, and the restatement (tests/shared_sample_area_engine.py) of each, computed
once in float32 and float64.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from shared_sample_area_engine import shared_sample_area_reference
from shared_sample_grad_cases import CASES, CASE_IDS, case  # noqa: F401  (re-exported)

LOOSE_CAP = 0.03        # tests/test_sample_area_cpu.py's cap; the restatement alone gives 0 to 7.4e-3 on these inputs
DEG, ZOOM = 22.5, 1.7   # the warp of the centres (shared_sample_grad_cases.case)


def rotated_footprint(i):
    """3 times the linear part of the centres' warp on the first two axes, F[2][2] = 1.5; taps (3, 2) / (2, 2, 2)"""
    d = len(CASES[i][0][0])
    c, s = np.cos(np.deg2rad(DEG)) / ZOOM, np.sin(np.deg2rad(DEG)) / ZOOM
    F = np.zeros((d, d))
    F[:2, :2] = 3.0 * np.array([[c, -s], [s, c]])
    if d == 3:
        F[2, 2] = 1.5
    return F.astype(np.float32), ((2, 2, 2) if d == 3 else (3, 2))


@functools.lru_cache(maxsize=None)
def area_reference(i):
    """(float32, float64) restatement of case ``i``'s centres under its rotated footprint; read-only"""
    c = case(i)
    F, taps = rotated_footprint(i)
    refs = tuple(shared_sample_area_reference(c["p"], c["lists"], c["shape"], c["bshape"], c["pts"], F, taps, c["cfg"], T)
                 for T in (np.float32, np.float64))
    for r in refs:
        for a in r.values():
            a.setflags(write=False)
    return refs


def loose_of(ref, ref64):
    """a point is loose if any of its inside taps is loose in either precision; asserts the cap on the restatement alone"""
    loose = ref["loose"] | ref64["loose"]
    assert loose.mean() < LOOSE_CAP, loose.mean()
    return loose
