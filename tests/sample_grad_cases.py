"""The cases the CPU and GPU tests of the point derivative share: the five rotated point sets of tests/test_gpu_sample.py on the
models of tests/test_gpu_render_view.py (``_model``), plus train_inverse_cov, mode2 and mode2_centre_grid on (16, 16) C 3; each
plain and blended.  The restatement (tests/sample_grad_engine.py) of a case is computed once, float32 and float64, and shared.
TEST INFRASTRUCTURE."""
import dataclasses
import functools

import numpy as np

from sample_grad_engine import sample_grad_reference
from test_gpu_render_view import _model
from test_gpu_sample import ROTATED, _rotated

# block shape, C, kernels per dim, option, output E, degrees, zoom, points outside
CASES = [(r[0], r[1], r[2], None) + r[3:] for r in ROTATED] \
    + [((16, 16), 3, (2, 2), name, (61, 83), 17.0, 1.7, 0) for name in ("train_inverse_cov", "mode2", "mode2_centre_grid")]
CASE_IDS = ["x".join(map(str, c[0])) + f"-c{c[1]}-k" + "x".join(map(str, c[2])) + (f"-{c[3]}" if c[3] else "") for c in CASES]


def blend_of(shape):
    """the blend of a blended case: 2 pixels ((2, 2, 1) on three axes); (2, 1) on the (7, 5) blocks, where 2 of 5 pixels leaves
    too many points on a window's end (loose share 3e-2 against 2.5e-3)"""
    if tuple(shape) == (7, 5):
        return (2, 1)
    return (2, 2, 1) if len(shape) == 3 else 2


@functools.lru_cache(maxsize=None)
def case_inputs(i, blended):
    shape, C_, kpd, opt, E, deg, zoom, n_out = CASES[i]
    cfg, p, K, active, grid, kw, centre = _model(shape, C_, kpd, opt)
    if centre is not None:
        cfg = dataclasses.replace(cfg, mus_grid=centre)
    return {"shape": list(shape), "C": C_, "kpd": kpd, "opt": opt, "cfg": cfg, "p": p, "K": K, "active": active, "grid": list(grid),
            "length": [g * n for g, n in zip(grid, shape)], "pts": _rotated(shape, grid, E, deg, zoom),
            "beta": blend_of(shape) if blended else None, "n_out": n_out}


@functools.lru_cache(maxsize=None)
def case_reference(i, blended):
    """(float32, float64) restatement of the case; read-only"""
    c = case_inputs(i, blended)
    return tuple(sample_grad_reference(c["p"], c["active"], c["shape"], c["grid"], c["length"], c["pts"], c["beta"], c["cfg"], T)
                 for T in (np.float32, np.float64))
