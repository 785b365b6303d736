"""CPU tests of the point derivative's host layer: the numpy restatement (tests/sample_grad_engine.py) against central
differences and against torch autograd, ``Smoe.sample_grad`` / ``Smoe.render_warp_grad`` driven through the oracle-backed
stand-in engine, and what the C entry point checks without a handle.

Central differences: h = 1e-5 source pixels in float64 block units, own block held fixed, on the float64 restatement.  The
truncation error of a central difference is h^2 f''' / 6 (1e-10 relative to a unit third derivative) and its rounding error
eps64 |V| / h ~ 2e-11, so 1e-7 of max |J| sits decades above both and five decades under any wrong term; points where the
piecewise-constant mask, clip or window may switch inside the stencil (the loose set of the restatement) are left out."""
import os
import re

import numpy as np
import pytest
import torch

from sample_grad_cases import CASES, CASE_IDS, case_inputs, case_reference
from sample_grad_engine import OracleSampleGradEngine, block_at, eval_at, model_state
from sample_engine import OracleSampleEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
from test_view_render_cpu import _image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_float64_restatement_against_central_differences(i, blended):
    c = case_inputs(i, blended)
    ref = case_reference(i, blended)[1]
    n, grid = c["shape"], c["grid"]
    d = len(n)
    T = np.float64
    st = model_state(c["p"], c["active"], c["cfg"], T)
    idx = np.flatnonzero(ref["inside"])
    g, u = ref["g"][idx], ref["u"][idx].astype(T)
    h = 1e-5
    fd = np.zeros((idx.size, d, ref["v"].shape[1]))
    for l in range(d):
        if n[l] < 2:
            continue
        step = np.zeros(d)
        step[l] = h / (n[l] - 1)
        vp = eval_at(st, n, grid, g, u + step, c["beta"], T)[0]
        vm = eval_at(st, n, grid, g, u - step, c["beta"], T)[0]
        fd[:, l] = (vp - vm) / (2 * h)
    J = ref["jac"][idx]
    tight = ~ref["loose"][idx]
    scale = np.abs(J).max()
    err = np.abs(J - fd)[tight].max() / scale
    print(f"max |J| {scale:.3f} per pixel, analytic vs central differences {err:.2e} of it outside the loose set, "
          f"loose share {ref['loose'].mean():.2e}, near the floor of the normaliser {ref['floor'].mean():.2e}, Jacobians that are not 0 {(np.abs(J).max(axis=(1, 2)) > 0).mean():.2f}")
    assert scale > 0.05 and tight.mean() > 0.9
    assert err <= 1e-7


def test_float32_restatement_against_autograd():
    """torch autograd of a float32 restatement of v(u) on one block, mask and clip flags detached.  Both sides are float32 with
    different association: the measured float32-vs-float64 distance of the restatement is below 2e-6 absolute at max |J| of 0.2
    .. 0.8 per pixel, so 1e-4 of max |dv / du| is two decades over rounding and four under a wrong term."""
    for opt in (None, "train_inverse_cov"):
        i = 0 if opt is None else [k for k, cs in enumerate(CASES) if cs[3] == opt][0]
        c = case_inputs(i, False)
        T = np.float32
        st = model_state(c["p"], c["active"], c["cfg"], T)
        b = 5
        rng = np.random.default_rng(3)
        u = rng.uniform(-0.03, 1.03, size=(400, 2)).astype(T)
        v, dv, wt, _, _ = block_at(st, np.full(400, b), u, T)
        A, mu, nu, gam, coef = (torch.from_numpy(np.ascontiguousarray(st[k][b])) for k in ("A", "mu", "nu", "gam", "coef"))
        ut = torch.from_numpy(u).requires_grad_(True)
        r = ut[:, None, :] - mu[None]                                      # (M, K, d)
        z = torch.einsum("mkl,klj->mkj", r, A)
        maha = (z * r).sum(-1) if st["ic"] else (z * z).sum(-1)
        g = coef[None] * torch.exp(-0.5 * maha)
        S = g.sum(1)
        w = g / torch.clamp(S, min=10e-12)[:, None]
        wtt = w * (w > float(st["tau"])).detach().to(w.dtype)
        e = nu[None] + torch.einsum("klc,ml->mkc", gam, ut)
        y = torch.einsum("mk,mkc->mc", wtt, e)
        yc = y.detach().clamp(0.0, float(st["vmax"]))
        vt = torch.where(yc == y.detach(), y, yc)
        J = np.stack([torch.autograd.grad(vt[:, ch].sum(), ut, retain_graph=True)[0].numpy() for ch in range(vt.shape[1])], axis=-1)
        assert np.abs(vt.detach().numpy() - v).max() < 1e-5 and (wt > 0).any() and (v > 0).any()
        scale = np.abs(dv).max()
        print(f"{opt}: max |dv/du| {scale:.3f}, restatement vs autograd {np.abs(J - dv).max() / scale:.2e} of it")
        assert np.abs(J - dv).max() <= 1e-4 * scale


# ---------------------------------------------------------------------------------------------------------------
# the facade on the CPU engine
# ---------------------------------------------------------------------------------------------------------------
IDENT = [[1, 0, 0], [0, 1, 0]]


@pytest.fixture(scope="module")
def fitted():
    b = blk.synthetic_blocks(15, (16, 16), 3, 99)
    img = blk.blocks_to_image(b, (48, 80), (16, 16))[:44, :75]
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True,
             engine_factory=OracleSampleGradEngine)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(3, val_iter=3)
    return s


def _rotation(deg, zoom, E, L):
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    M = np.array([[c, -s], [s, c]])
    return np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)


def test_facade_shapes_round_trip_and_values(fitted):
    s = fitted
    A = _rotation(17, 1.7, (31, 29), (44, 75))
    pts = blk.warp_points(A, (31, 29))
    J = s.sample_grad(pts)
    assert J.shape == (31, 29, 2, 3) and J.dtype == np.float32 and np.abs(J).max() > 1e-3
    assert s.sample_grad(pts.reshape(-1, 2)).shape == (31 * 29, 2, 3) and s.sample_grad(pts[3, 4]).shape == (2, 3)
    assert s.sample_grad(np.zeros((0, 2), np.float32)).shape == (0, 2, 3)
    assert np.array_equal(s.sample_grad(pts.astype(np.float64).tolist()), J)                 # array-like
    dev = s.sample_grad(torch.from_numpy(pts), to_host=False)                                 # device tensor in, tensor out
    assert torch.is_tensor(dev) and dev.dtype == torch.float32 and np.array_equal(dev.numpy(), J)
    Jv, V = s.sample_grad(pts, want_values=True, blend=2)
    assert V.shape == (31, 29, 3) and V.dtype == np.float32 and not np.array_equal(Jv, J)
    # the value before the lattice rounds onto what sample() returns
    lat = s.sample(pts, blend=2)
    assert np.abs(V - lat).max() <= 0.5 / 255 + 1e-6
    out = s.sample_grad(np.array([[44.0, 10.0], [-0.01, 5.0], [np.nan, 5.0]], np.float32), want_values=True)
    assert (out[0] == 0).all() and (out[1] == 0).all()
    for kw in [dict(points=pts[..., :1]), dict(points=pts, blend=9), dict(points=pts, blend=(1, 2, 3)), dict(points=pts, blend=float("nan"))]:
        with pytest.raises(ValueError):
            s.sample_grad(**kw)


def test_render_warp_grad(fitted):
    s = fitted
    A = _rotation(-31, 0.8, (40, 50), (44, 75))
    src = s.render_warp_grad(A, (40, 50), blend=2)
    view = s.render_warp_grad(A, (40, 50), wrt="view", blend=2)
    assert src.shape == (40, 50, 2, 3) and view.shape == src.shape
    assert np.array_equal(src, s.sample_grad(blk.warp_points(A, (40, 50)), blend=2))
    want = np.einsum("...lc,lm->...mc", src.astype(np.float64), A[:, :2])
    assert np.abs(view - want).max() <= 1e-6 * np.abs(want).max() and not np.allclose(view, src)
    ident = s.render_warp_grad(IDENT, (44, 75))
    assert np.array_equal(ident, s.sample_grad(blk.warp_points(IDENT, (44, 75))))
    assert np.array_equal(s.render_warp_grad(IDENT, (44, 75), wrt="view"), ident)
    dv, vv = s.render_warp_grad(A, (40, 50), wrt="view", want_values=True, to_host=False)
    assert torch.is_tensor(dv) and torch.is_tensor(vv) and tuple(vv.shape) == (40, 50, 3) and np.array_equal(dv.numpy(), s.render_warp_grad(A, (40, 50), wrt="view"))
    with pytest.raises(ValueError):
        s.render_warp_grad(A, (40, 50), wrt="pixels")


def test_an_engine_without_the_method_raises():
    s = Smoe(_image(32, 48), train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True,
             engine_factory=OracleSampleEngine)
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_grad()")):
        s.sample_grad(np.zeros((1, 2), np.float32))
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_grad()")):
        s.render_warp_grad(IDENT, (4, 4))


# ---------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------
def test_smoe_sample_grad_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_sample_grad\s*\(", src)
    assert re.search(r"float\*\s+jac,\s*float\*\s+values,\s*int32_t\*\s+block,\s*void\*\s+stream", src)
    assert hasattr(lib, "smoe_sample_grad") and "smoe_sample_grad" in _lib.EXPORTS
    bl = (C.c_float * 3)(1.0, 1.0, 0.0)
    rc = lib.smoe_sample_grad(None, None, None, None, None, None, 5, bl, None, None, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_sample_grad" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
