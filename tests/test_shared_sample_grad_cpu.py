"""CPU tests of the shared-mode point derivative's host layer: the numpy restatement (tests/shared_sample_grad_engine.py)
against ``oracle.smoe_oracle.forward``, against central differences and against torch autograd on the 13 parity cases,
``SharedSmoe.eval_points_grad`` / ``eval_view_grad`` / ``eval_warp_grad`` driven through the oracle-backed stand-in engine,
two gloo ranks against one, and what the two C entry points check without a handle.

Central differences: h = 1e-5 source pixels in float64 image units, own batch held fixed, on the float64 restatement.  The
truncation error of a central difference is h^2 f''' / 6 and its rounding error eps64 |v| / h ~ 2e-11; the block models
reached 4.3e-10 of max |J|.  Measured here over the 13 cases: 1.0e-10 to 5.4e-10 of max |J| (0.07 .. 0.41 per pixel),
so the bound is 1e-8: an order of magnitude above the measurement and six decades under any wrong term.  Points where the
piecewise-constant mask or clip may switch inside the stencil (the loose set, and points whose y lies within 1e-4 of a clip
edge) are left out."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sample_grad_engine import model_state
from shared_sample_engine import shared_points_reference
from shared_sample_grad_cases import CASES, CASE_IDS, case, loose_of
from shared_sample_grad_engine import OracleSharedSampleGradEngine, shared_points_grad_reference
from shared_sample_engine import OracleSharedSampleEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
from test_shared_render_cpu import _image
from test_view_render_cpu import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 1e-8


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_float64_restatement_is_the_oracle_forward_and_its_derivative(i):
    c = case(i)
    ref = c["ref64"]
    loose = loose_of(c)
    inside, bid, u = c["inside"], c["bid"], c["u"]
    # y is oracle.forward's y on the same points, batch by batch
    fw = shared_points_reference(c["p"], c["lists"], u, bid, c["cfg"], np.float64)
    dy = np.abs(ref["y"] - fw["y"]).max()
    assert dy <= 1e-12, dy
    assert np.array_equal(ref["wt"] > 0, fw["wt"] > 0)
    empty = inside & ~c["lists"][np.maximum(bid, 0)].any(axis=1)
    assert empty.any() and not loose[empty].any() and (ref["v"][empty] == 0).all() and (ref["jac"][empty] == 0).all()
    assert (ref["v"][~inside] == 0).all() and (ref["jac"][~inside] == 0).all() and (ref["batch"][~inside] == -1).all()
    for r in (ref, c["ref32"]):
        assert np.isfinite(r["jac"]).all() and np.isfinite(r["v"]).all()
    # central differences of v, own batch held fixed
    shape = c["shape"]
    d = len(shape)
    h = 1e-5
    idx = np.flatnonzero(inside)
    u64 = u[idx].astype(np.float64)
    fd = np.zeros((idx.size, d, c["C"]))
    for l in range(d):
        step = np.zeros(d)
        step[l] = h / (shape[l] - 1)
        vp = shared_points_grad_reference(c["p"], c["lists"], u64 + step, bid[idx], shape, c["cfg"], np.float64)["v"]
        vm = shared_points_grad_reference(c["p"], c["lists"], u64 - step, bid[idx], shape, c["cfg"], np.float64)["v"]
        fd[:, l] = (vp - vm) / (2 * h)
    J = ref["jac"][idx]
    y = ref["y"][idx]
    vmax = float(model_state(c["p"], np.ones((1, c["K"]), bool), c["cfg"], np.float64)["vmax"])
    near_clip = ((np.abs(y) < 1e-4) | (np.abs(y - vmax) < 1e-4)).any(axis=1) & (ref["wt"][idx] > 0).any(axis=1)
    tight = ~loose[idx] & ~near_clip
    scale = np.abs(J).max()
    err = np.abs(J - fd)[tight].max() / scale
    clipped = (ref["v"] != ref["y"]).any(axis=1)[idx]
    print(f"{CASE_IDS[i]}: y vs oracle.forward {dy:.1e}; max |J| {scale:.3f} per pixel, analytic vs central differences {err:.2e} "
          f"of it; loose share {loose.mean():.2e}, outside {1 - inside.mean():.3f}, clip acts {clipped.mean():.3f}, "
          f"floor {ref['floor'].mean():.2e}")
    assert scale > 0.05 and tight.mean() > 0.9
    assert err <= FD_BOUND


def test_float32_restatement_against_autograd():
    """torch autograd of a float32 restatement of v(u) with one batch's list, mask and clip flags detached.  Both sides are
    float32 with different association; 1e-4 of max |dv / du| is two decades over rounding and four under a wrong term (the
    bound of tests/test_sample_grad_cpu.py)."""
    for i in (1, [k for k, cs in enumerate(CASES) if cs[2] == "train_inverse_cov"][0]):
        c = case(i)
        T = np.float32
        st = model_state(c["p"], np.ones((1, c["K"]), bool), c["cfg"], T)
        b = 3
        u = np.random.default_rng(3).uniform(-0.03, 1.03, size=(400, 2)).astype(T)
        ref = shared_points_grad_reference(c["p"], c["lists"], u, np.full(400, b), (2, 2), c["cfg"], T)   # du_dx = 1
        A, mu, nu, gam = (torch.from_numpy(np.ascontiguousarray(st[k][0])) for k in ("A", "mu", "nu", "gam"))
        coef = torch.from_numpy(np.where(c["lists"][b], st["coef"][0], T(0)))
        ut = torch.from_numpy(u).requires_grad_(True)
        r = ut[:, None, :] - mu[None]
        z = torch.einsum("mkl,klj->mkj", r, A)
        maha = (z * r).sum(-1) if st["ic"] else (z * z).sum(-1)
        g = coef[None] * torch.exp(-0.5 * maha)
        w = g / torch.clamp(g.sum(1), min=10e-12)[:, None]
        wtt = w * (w > float(st["tau"])).detach().to(w.dtype)
        e = nu[None] + torch.einsum("klc,ml->mkc", gam, ut)
        y = torch.einsum("mk,mkc->mc", wtt, e)
        yc = y.detach().clamp(0.0, float(st["vmax"]))
        vt = torch.where(yc == y.detach(), y, yc)
        J = np.stack([torch.autograd.grad(vt[:, ch].sum(), ut, retain_graph=True)[0].numpy() for ch in range(vt.shape[1])], axis=-1)
        assert np.abs(vt.detach().numpy() - ref["v"]).max() < 1e-5 and (ref["wt"] > 0).any() and (ref["v"] > 0).any()
        scale = np.abs(ref["jac"]).max()
        print(f"{CASE_IDS[i]}: max |dv/du| {scale:.3f}, restatement vs autograd {np.abs(J - ref['jac']).max() / scale:.2e} of it")
        assert np.abs(J - ref["jac"]).max() <= 1e-4 * scale


# ---------------------------------------------------------------------------------------------------------------
# the facade through the oracle engine
# ---------------------------------------------------------------------------------------------------------------
def _make(img, bs, kpd, factory=OracleSharedSampleGradEngine, **kw):
    s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
                   engine_factory=factory, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


@pytest.fixture(scope="module")
def fitted():
    s = _make(_image((48, 64), C=3, seed=6), (16, 16), (6, 8), use_yuv=True)
    s.train(4, val_iter=2, ukl_iter=2)
    return s


def _centres(shape):
    return np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) + 0.5 for s in shape], indexing="ij"), axis=-1)


def _rotation(deg, zoom, E, L):
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    M = np.array([[c, -s], [s, c]])
    return np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)


def test_shared_smoe_has_the_three_methods_and_no_aliases():
    for name in ("eval_points_grad", "eval_view_grad", "eval_warp_grad"):
        assert hasattr(SharedSmoe, name)
    for name in ("sample_grad", "render_warp_grad", "render_view_grad"):
        assert not hasattr(SharedSmoe, name)


def test_facade_shapes_round_trip_and_values(fitted):
    s = fitted
    A = _rotation(17, 1.7, (31, 29), (48, 64))
    pts = blk.warp_points(A, (31, 29))
    J = s.eval_points_grad(pts)
    assert J.shape == (31, 29, 2, 3) and J.dtype == np.float32 and np.abs(J).max() > 1e-3
    assert s.eval_points_grad(pts.reshape(-1, 2)).shape == (31 * 29, 2, 3) and s.eval_points_grad(pts[3, 4]).shape == (2, 3)
    assert s.eval_points_grad(np.zeros((0, 2), np.float32)).shape == (0, 2, 3)
    assert np.array_equal(s.eval_points_grad(pts.astype(np.float64).tolist()), J)            # array-like
    dev = s.eval_points_grad(torch.from_numpy(pts), to_host=False)                            # tensor in, tensor out
    assert torch.is_tensor(dev) and dev.dtype == torch.float32 and np.array_equal(dev.numpy(), J)
    Jv, V = s.eval_points_grad(pts, want_values=True)
    assert V.shape == (31, 29, 3) and V.dtype == np.float32 and np.array_equal(Jv, J)
    # the value before the lattice, put on the lattice, is what eval_points returns
    lat = s.eval_points(pts)
    assert np.abs(np.floor(V * 255 + 0.5) / 255 - lat).max() <= 1e-6
    free = s.eval_points_grad(pts, use_lists=False)
    assert free.shape == J.shape and np.abs(free - J).max() < 0.1 * np.abs(J).max()            # the pruned kernels hardly count
    out = s.eval_points_grad(np.array([[48.0, 10.0], [-0.01, 5.0], [np.nan, 5.0]], np.float32), want_values=True)
    assert (out[0] == 0).all() and (out[1] == 0).all()


def test_the_whole_image_view_at_1x_is_the_pixel_centres(fitted):
    s = fitted
    Jp, Vp = s.eval_points_grad(_centres((48, 64)), want_values=True)
    Jv, Vv = s.eval_view_grad(None, want_values=True)
    assert Jv.shape == (48, 64, 2, 3) and np.array_equal(Jv, Jp) and np.array_equal(Vv, Vp)
    assert np.array_equal(s.eval_view_grad([None, (0, 64)], scale=1), Jp)
    assert np.abs(np.floor(Vp.astype(np.float64) * 255 + 0.5) / 255 - s.get_reconstruction()).max() <= 1e-6
    win = s.eval_view_grad([(5.25, 30.5), (17.0, 49.75)], size=(19, 23), to_host=False)
    assert torch.is_tensor(win) and tuple(win.shape) == (19, 23, 2, 3)
    assert tuple(s.eval_view_grad(None, size=(2, 3)).shape) == (2, 3, 2, 3)


def test_eval_warp_grad(fitted):
    s = fitted
    A = _rotation(-31, 0.8, (40, 50), (48, 64))
    src = s.eval_warp_grad(A, (40, 50))
    view = s.eval_warp_grad(A, (40, 50), wrt="view")
    assert src.shape == (40, 50, 2, 3) and view.shape == src.shape
    assert np.array_equal(src, s.eval_points_grad(blk.warp_points(A, (40, 50))))
    want = np.einsum("...lc,lm->...mc", src.astype(np.float64), A[:, :2])
    assert np.abs(view - want).max() <= 1e-6 * np.abs(want).max() and not np.allclose(view, src)
    ident = [[1, 0, 0], [0, 1, 0]]
    assert np.array_equal(s.eval_warp_grad(ident, (48, 64), wrt="view"), s.eval_points_grad(_centres((48, 64))))
    dv, vv = s.eval_warp_grad(A, (40, 50), wrt="view", want_values=True, to_host=False)
    assert torch.is_tensor(dv) and torch.is_tensor(vv) and tuple(vv.shape) == (40, 50, 3) and np.array_equal(dv.numpy(), view)


def test_argument_errors(fitted):
    s = fitted
    for bad in ([(0, 49), None], [(-1, 4), None], [(5, 5), None], [None], [None, None, None]):
        with pytest.raises(ValueError, match="eval_view_grad"):
            s.eval_view_grad(bad)
    with pytest.raises(ValueError):
        s.eval_view_grad(None, size=(8, 8), scale=2)
    with pytest.raises(ValueError):
        s.eval_view_grad(None, size=(8, 0))
    with pytest.raises(ValueError):
        s.eval_points_grad(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        s.eval_warp_grad(np.eye(3)[:2], (8, 8), wrt="pixels")
    with pytest.raises(TypeError):
        s.eval_points_grad(np.zeros((4, 2), np.float32), blend=1.0)
    plain = _make(_image((32, 48), seed=5), (16, 16), (3, 4), factory=OracleSharedSampleEngine)
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_grad()")):
        plain.eval_points_grad(np.zeros((1, 2), np.float32))
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no render_view_grad()")):
        plain.eval_view_grad(None)


# ---------------------------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
from shared_sample_grad_engine import OracleSharedSampleGradEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
ws = int(os.environ.get("WORLD_SIZE", "1"))
if ws > 1:
    dist.init_process_group(backend="gloo")
b = blk.synthetic_blocks(15, (16, 16), 1, 99)
img = blk.blocks_to_image(b, (48, 80), (16, 16))
s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=[4, 6], batch_size=[16, 16], use_determinant=True,
               engine_factory=OracleSharedSampleGradEngine)
s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
s.train(4, val_iter=2, ukl_iter=2)
c, sn = np.cos(np.deg2rad(17)) / 1.3, np.sin(np.deg2rad(17)) / 1.3
M = np.array([[c, -sn], [sn, c]])
A = np.concatenate([M, (np.array([24.0, 40.0]) - M @ np.array([25.0, 40.0]))[:, None]], axis=1)
warp, val = s.eval_warp_grad(A, (50, 80), wrt="view", want_values=True)
out = {"warp": warp, "val": val, "view": s.eval_view_grad([(5.5, 40), (16, 70)], size=(33, 41)),
       "free": s.eval_points_grad(blk.warp_points(A, (50, 80)), use_lists=False),
       "lens": [int(m.sum()) for m in s.kernel_list_per_batch], "span": (s.lo, s.hi)}
ranks = [out]
if ws > 1:
    ranks = [None] * ws
    dist.all_gather_object(ranks, out)
if ws == 1 or dist.get_rank() == 0:
    pickle.dump(ranks, open(sys.argv[2], "wb"))
if ws > 1:
    dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_evaluate_what_one_rank_evaluates(tmp_path):
    w = tmp_path / "worker.py"
    w.write_text(WORKER)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    one = str(tmp_path / "one.pkl")
    subprocess.check_call([sys.executable, str(w), ROOT, one], env=env, timeout=300)
    two = str(tmp_path / "two.pkl")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(w), ROOT, two],
                          env=env, timeout=600)
    (a,), (b, b1) = pickle.load(open(one, "rb")), pickle.load(open(two, "rb"))
    assert a["span"] == (0, 15) and b["span"] == (0, 8) and b1["span"] == (8, 15)
    assert min(a["lens"]) < 24, "no list was pruned: the gather of the lists would not show"
    assert np.abs(a["warp"]).max() > 1e-3 and not np.array_equal(a["warp"], a["free"])
    for k in ("warp", "val", "view", "free"):
        assert np.array_equal(b[k], b1[k]), k                                  # the same on every rank, bit for bit
        # against one rank: two ranks sum the gradients of the fit in another order, so the parameters differ in their last
        # bits -- invisible on the 8-bit lattice of eval_points, visible in a float32 derivative.  Four Adam steps of float32
        # sums reordered move a parameter by a few 1e-7 of itself and a slope of up to ~50 per unit carries that into J:
        # 1e-4 of max |J| is a decade over that and three under a list that was not gathered
        err = np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()
        print(f"{k}: two ranks vs one {err:.2e} of the maximum")
        assert err <= 1e-4, k


# ---------------------------------------------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_check_their_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_shared_sample_grad\s*\(", src) and re.search(r"\bint\s+smoe_shared_render_view_grad\s*\(", src)
    assert len(re.findall(r"float\*\s+jac,\s*float\*\s+values,\s*int32_t\*\s+batch,\s*void\*\s+stream", src)) == 2
    for name in ("smoe_shared_sample_grad", "smoe_shared_render_view_grad"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.smoe_shared_sample_grad.argtypes) == 9 and len(lib.smoe_shared_render_view_grad.argtypes) == 10
    rc = lib.smoe_shared_sample_grad(None, None, None, None, 5, None, None, None, None)
    err = lib.smoe_last_error()
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_sample_grad" in err and b"handle" in err
    ext = (C.c_int32 * 3)(4, 4, 1)
    rc = lib.smoe_shared_render_view_grad(None, None, None, ext, None, None, None, None, None, None)
    err = lib.smoe_last_error()
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_render_view_grad" in err and b"handle" in err
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
