"""The parity cases of the shared-mode point derivative, shared by tests/test_shared_sample_grad_cpu.py and
tests/test_gpu_shared_sample_grad.py: the rotated point sets ``_rotated(bshape, grid, E, 22.5, 1.7)`` on the five images of
tests/test_gpu_shared_render.py and on the second one under each of its eight options, with the float32 and float64
restatement of every case computed once.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from shared_sample_engine import point_mapping
from shared_sample_grad_engine import shared_points_grad_reference
from test_gpu_sample import _rotated
from test_gpu_shared_render import IMAGES, OPTIONS, _grid, _name, _setup

EXTENTS = [(112, 168), (112, 168), (88, 112), (40, 56, 7), (40, 48)]
CASES = [(IMAGES[i], EXTENTS[i], "plain", {}) for i in range(5)] + [(IMAGES[1], EXTENTS[1], n, kw) for n, kw in OPTIONS]
CASE_IDS = [_name(c[0]) + "-" + c[2] for c in CASES]
LOOSE_CAP = 0.01


@functools.lru_cache(maxsize=None)
def case(i):
    """inputs and the restatement of case ``i`` in both precisions; read-only"""
    image, E, name, kw = CASES[i]
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, mus_grid = _setup(shape, bshape, C_, kpd, name, **kw)
    pts = _rotated(bshape, _grid(shape, bshape), E, 22.5, 1.7)
    inside, bid, u = point_mapping(pts, shape, bshape)
    ref32 = shared_points_grad_reference(p, lists, u, bid, shape, cfg, np.float32)
    ref64 = shared_points_grad_reference(p, lists, u, bid, shape, cfg, np.float64)
    for r in (ref32, ref64):
        for a in r.values():
            a.setflags(write=False)
    return dict(shape=shape, bshape=bshape, C=C_, K=K, NB=NB, p=p, cfg=cfg, lists=lists, mus_grid=mus_grid, kw=kw, pts=pts,
                inside=inside, bid=bid, u=u, ref32=ref32, ref64=ref64)


def loose_of(c):
    """the loose set of a case, by the float64 restatement; asserts the cap on the restatement alone"""
    loose = c["ref64"]["loose"]
    assert loose.mean() < LOOSE_CAP, loose.mean()
    return loose
