"""One decoder case per (dim, channels, kernels) triple of csrc/smoe_variants.def that is not FULL, shared by
tests/test_triple_cases_cpu.py and tests/test_gpu_decoder_triples.py: the model of tests/test_gpu_render_view.py (``_model``) on
12 blocks of (16, 16) / (8, 8, 4) with a kernel grid whose product is the triple's K, the rotated point set of
tests/test_gpu_sample.py (``_rotated``), each in two configurations -- (train_inverse_cov off, plain) and (train_inverse_cov
on, blend 2 / (2, 2, 1)).  The restatements of a case (tests/sample_engine.py, sample_grad_engine.py, sample_area_engine.py)
are computed once, float32 and float64, and shared.  The triples are read from smoe_variants.def itself, so the list cannot
drift from the build.  TEST INFRASTRUCTURE."""
import functools
import os
import re

import numpy as np

from sample_area_cases import footprint_of
from sample_area_engine import sample_area_reference
from sample_engine import sample_reference
from sample_grad_engine import sample_grad_reference
from test_gpu_render_view import _model
from test_gpu_sample import _rotated

VARIANTS_DEF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "steered_mixture_of_experts_amd", "csrc",
                            "smoe_variants.def")


def parse_triples(path=VARIANTS_DEF):
    """[(dim, channels, kernels, full)] in the order of the file; a line that names the macro but does not parse is an error"""
    out = []
    with open(path) as f:
        for line in f:
            code = line.split("//")[0].strip()
            if not code:
                continue
            m = re.fullmatch(r"SMOE_TRIPLE\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*([01])\s*\)", code)
            assert m, f"{path}: cannot read {line!r}"
            out.append(tuple(int(v) for v in m.groups()))
    assert len(set(t[:3] for t in out)) == len(out), "a triple is listed twice"
    return out


BLOCK_SHAPE = {2: (16, 16), 3: (8, 8, 4)}
# the rotated point set per dimension: output size E, degrees, zoom (tests/test_gpu_sample.py: ROTATED), and how many of its
# points fall outside the 12 blocks (dim 2: 48 x 64 pixels; dim 3: 16 x 24 x 8 pixels under a 40 x 50 x 5 output)
ROTATION = {2: ((61, 83), 17.0, 1.7, 0), 3: ((40, 50, 5), 17.0, 1.3, 6770)}
CONFIGS = [("plain", None, False), ("ic-blend", "train_inverse_cov", True)]          # name, option of _model, blended
# Four K = 3 configurations miss the conditions on the inputs with ``_model``'s draw: the kernels stand in one line ([3, 1],
# [1, 3, 1], [3, 1, 1]) and the steering is sharp (|A| up to 10, squared to 106 under train_inverse_cov), so far from the line
# -- and a block away, where the cross-fade evaluates the neighbour -- the sum of the gates falls under the 1e-11 floor of the
# normaliser; there g / 1e-11 passes the threshold or y passes 0 and the restatement calls the point loose.  Every loose point
# of these cases is such a point.  ic-blend: share of the point derivative 1.6e-2 on (2, 1, 3) and 1.2e-2 on (3, 3, 3), cap 0.01;
# of the area decoder 4.4e-2 on (3, 1, 3) and 7.9e-2 on (3, 3, 3), cap 0.03.  (2, 1, 3) plain: the float32 and float64
# restatements of render_blend on the resampled grid differ by 0.32 outside the loose set (a block left with one listed kernel
# drops out of the cross-fade where its gate is under the floor), and the point derivative's share is 9.9e-3.  The steering
# (A_diagonal and A_corr) of these four is scaled by the factor given, which leaves no point on the floor; every other
# configuration keeps the draw.
TAMED = {((2, 1, 3), "plain"): 0.5, ((2, 1, 3), "ic-blend"): 0.2, ((3, 1, 3), "ic-blend"): 0.2, ((3, 3, 3), "ic-blend"): 0.2}

# triple -> (kernels per dim, {configuration: loose share of the covered points of the area restatement, measured on the
# restatement alone; cap sample_area_cases.LOOSE_CAP = 0.03}).  The point decoders' loose shares are <= 2.2e-3 everywhere (cap 0.01).
TRIPLE_CASES = {
    (2, 1, 1): ((1, 1), {"plain": 0.0, "ic-blend": 0.0}),
    (2, 1, 2): ((1, 2), {"plain": 5.9e-04, "ic-blend": 5.9e-04}),
    (2, 1, 3): ((3, 1), {"plain": 0.0, "ic-blend": 0.0}),
    (2, 1, 6): ((2, 3), {"plain": 5.9e-04, "ic-blend": 1.2e-03}),
    (2, 1, 9): ((3, 3), {"plain": 9.9e-04, "ic-blend": 1.2e-03}),
    (2, 1, 12): ((3, 4), {"plain": 3.6e-03, "ic-blend": 2.2e-03}),
    (2, 1, 16): ((4, 4), {"plain": 7.9e-04, "ic-blend": 4.1e-03}),
    (2, 3, 1): ((1, 1), {"plain": 0.0, "ic-blend": 0.0}),
    (2, 3, 2): ((1, 2), {"plain": 0.0, "ic-blend": 0.0}),
    (2, 3, 3): ((3, 1), {"plain": 0.0, "ic-blend": 4.3e-03}),
    (2, 3, 6): ((2, 3), {"plain": 2.4e-03, "ic-blend": 1.8e-03}),
    (2, 3, 9): ((3, 3), {"plain": 1.2e-03, "ic-blend": 5.5e-03}),
    (3, 1, 1): ((1, 1, 1), {"plain": 0.0, "ic-blend": 0.0}),
    (3, 1, 2): ((2, 1, 1), {"plain": 8.0e-04, "ic-blend": 2.4e-03}),
    (3, 1, 3): ((1, 3, 1), {"plain": 1.7e-02, "ic-blend": 1.3e-03}),
    (3, 1, 4): ((2, 2, 1), {"plain": 1.1e-03, "ic-blend": 1.9e-03}),
    (3, 1, 6): ((3, 2, 1), {"plain": 2.1e-03, "ic-blend": 5.1e-03}),
    (3, 1, 8): ((2, 2, 2), {"plain": 2.9e-03, "ic-blend": 3.2e-03}),
    (3, 3, 1): ((1, 1, 1), {"plain": 0.0, "ic-blend": 0.0}),
    (3, 3, 2): ((1, 2, 1), {"plain": 5.3e-04, "ic-blend": 1.6e-03}),
    (3, 3, 3): ((3, 1, 1), {"plain": 8.0e-04, "ic-blend": 1.1e-03}),
    (3, 3, 6): ((1, 3, 2), {"plain": 1.6e-03, "ic-blend": 3.2e-03}),
    (3, 3, 8): ((2, 2, 2), {"plain": 2.1e-03, "ic-blend": 4.5e-03}),
}
TRIPLES = list(TRIPLE_CASES)
TRIPLE_IDS = ["d%dc%dk%d" % t for t in TRIPLES]
assert all(int(np.prod(kpd)) == t[2] and len(kpd) == t[0] for t, (kpd, _) in TRIPLE_CASES.items())


def blend_of(shape):
    return (2, 2, 1) if len(shape) == 3 else 2


def model_of(triple, opt):
    """``_model`` of the triple's kernel grid, unchanged: with its dead kernels (prior 0 in block 3, negative in block 4) and
    its kernel lists drawn at 0.85.  Shared and read-only."""
    kpd = TRIPLE_CASES[triple][0]
    shape = BLOCK_SHAPE[triple[0]]
    cfg, p, K, active, grid, kw, _ = _model(shape, triple[1], kpd, opt)
    assert K == triple[2] and int(np.prod(grid)) == 12
    return cfg, p, K, active, grid, kw


@functools.lru_cache(maxsize=None)
def case_inputs(triple, config):
    """The inputs of the restatement cases.  K >= 4: ``_model``'s draw as it is.  K <= 3: every block keeps a live kernel --
    the priors are made positive, and a block whose list came out empty gets its kernel with the largest prior back.  A block
    without a live kernel decodes to y = 0 exactly, which the restatements count as loose (``block_at``: a y within 1e-6 of 0),
    and with few kernels whole blocks die (K = 1: blocks 3 and 4 and 15 % of the rest, loose share of the area decoder 0.27 ...
    0.50 against a cap of 0.03); dead blocks are checked bit for bit in tests/test_gpu_decoder_triples.py instead.  The
    configurations of TAMED have their steering scaled as well."""
    name, opt, blended = next(c for c in CONFIGS if c[0] == config)
    cfg, p, K, active, grid, kw = model_of(triple, opt)
    shape = BLOCK_SHAPE[triple[0]]
    if K <= 3:
        p = {k: v.copy() for k, v in p.items()}
        active = active.copy()
        p["pis"] = np.where(p["pis"] > 0, p["pis"], np.float32(0.25)).astype(np.float32)
        empty = ~active.any(axis=1)
        active[empty, p["pis"][empty].argmax(axis=1)] = True
        assert (active & (p["pis"] > 0)).any(axis=1).all()
    if (triple, config) in TAMED:
        p["A_diagonal"] = (p["A_diagonal"] * np.float32(TAMED[(triple, config)])).astype(np.float32)
        p["A_corr"] = (p["A_corr"] * np.float32(TAMED[(triple, config)])).astype(np.float32)
    E, deg, zoom, n_out = ROTATION[triple[0]]
    F, taps = footprint_of(shape, deg, zoom)
    return {"shape": list(shape), "C": triple[1], "kpd": TRIPLE_CASES[triple][0], "opt": opt, "kw": kw, "cfg": cfg, "p": p, "K": K,
            "active": active, "grid": list(grid), "length": [g * n for g, n in zip(grid, shape)],
            "pts": _rotated(shape, grid, E, deg, zoom), "beta": blend_of(shape) if blended else None, "n_out": n_out,
            "F": F, "taps": taps}


def _both(fn, c, *extra):
    return tuple(fn(c["p"], c["active"], c["shape"], c["grid"], c["length"], c["pts"], *extra, c["beta"], c["cfg"], T)
                 for T in (np.float32, np.float64))


@functools.lru_cache(maxsize=None)
def sample_case_reference(triple, config):
    """(float32, float64) restatement of smoe_sample on the case; read-only"""
    return _both(sample_reference, case_inputs(triple, config))


@functools.lru_cache(maxsize=None)
def grad_case_reference(triple, config):
    """(float32, float64) restatement of smoe_sample_grad on the case; read-only"""
    return _both(sample_grad_reference, case_inputs(triple, config))


@functools.lru_cache(maxsize=None)
def area_case_reference(triple, config):
    """(float32, float64) restatement of smoe_sample_area on the case under its rotated footprint; read-only"""
    c = case_inputs(triple, config)
    return _both(sample_area_reference, c, c["F"], c["taps"])


def parity_shape(s):
    """the triple of an entry (block shape, channels, kernels per dim, use_yuv) of tests/test_gpu_parity.py"""
    return (len(s[0]), s[1], int(np.prod(s[2])))
