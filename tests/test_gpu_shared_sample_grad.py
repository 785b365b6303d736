"""GPU tests of the shared-mode point derivative (smoe_shared_sample_grad / smoe_shared_render_view_grad through the C ABI):
parity with the CPU restatement on the 13 rotated point sets, consistency with smoe_shared_sample, independence of the order
of the points, ownership at the batch boundaries, ragged counts with guard bytes, views, the argument checks with a real
handle, and the facade.

Parity criterion = tests/test_gpu_sample_grad.py's.  The restatement (tests/shared_sample_grad_engine.py) is evaluated in
float32 and float64; with ``e32 = max |J32 - J64|`` outside the loose set, the kernel must satisfy ``|J_gpu - J64| <= F * e32``
there, and ``values`` against ``v64`` with their own ``e32``.  F: the hardware exp2 / reciprocal are 1-ulp approximations where
numpy rounds correctly, and the kernel forms the slope from the gate's z' = u A' - c (a difference of products) where the
restatement forms it from u - mu; more than four bits (16) would be a wrong term.  F is twice the largest ratio measured on the
MI355X, rounded up to a power of two (profiles/render/shared_sample_grad_parity.txt has every case).  The loose share is a
condition on the inputs that the restatement alone has to meet first: < 0.01.  Loose points must be finite; outside points are
0 / 0 / -1 and the points of the batch with the empty list 0 / 0 / its id, exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from render_cases import _dev_axes, _guarded
from shared_sample_engine import point_mapping
from shared_sample_grad_cases import CASES, CASE_IDS, case, loose_of
from shared_sample_grad_engine import shared_points_grad_reference
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks
from test_gpu_shared_render import EMPTY, IMAGES, _dev, _dev_lists, _engine, _grid, _name, _setup
from test_gpu_shared_sample import _centres, _dev_view, _pts, _view_tables

pytestmark = pytest.mark.gpu

F = 8.0
SENT = -7.0


def _bits32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _lattice(v):
    """float32 values before the lattice -> smoe_shared_sample's float image in the kernel's arithmetic (precision 8):
    floorf(fmaf(v, inv_scale, 0.5f)) * scale with scale = 1.0f / 255 and inv_scale = 1.0f / scale.  The product of two float32
    and the 0.5 are exact in float64, so one rounding to float32 is the fused multiply-add."""
    scale = np.float32(1) / np.float32(255)
    inv = np.float32(1) / scale
    k = np.floor((v.astype(np.float64) * np.float64(inv) + 0.5).astype(np.float32))
    return (k * scale).astype(np.float32)


def _bound(dJ, dV, ref32, ref64, loose, what):
    eJ = np.abs(ref32["jac"].astype(np.float64) - ref64["jac"])[~loose].max()
    eV = np.abs(ref32["v"].astype(np.float64) - ref64["v"])[~loose].max()
    print(f"{what}: max |J| {np.abs(ref64['jac']).max():.3f} per pixel; J: e32 {eJ:.2e}, kernel {dJ[~loose].max():.2e}, ratio "
          f"{dJ[~loose].max() / eJ:.2f}; values: e32 {eV:.2e}, kernel {dV[~loose].max():.2e}, ratio {dV[~loose].max() / eV:.2f}; "
          f"loose share {loose.mean():.2e}, on the loose set J {dJ[loose].max() if loose.any() else 0:.2e}")
    assert (dJ[~loose] <= F * eJ).all(), dJ[~loose].max() / eJ
    assert (dV[~loose] <= F * eV).all(), dV[~loose].max() / eV


# ---------------------------------------------------------------------------------------------------------------
# 1. + 2. parity with the restatement, consistency with smoe_shared_sample
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_parity_and_consistency(i):
    c = case(i)
    loose = loose_of(c)                                        # asserts the cap on the restatement alone
    ref32, ref64, inside, bid = c["ref32"], c["ref64"], c["inside"], c["bid"]
    eng = _engine(c["shape"], c["bshape"], c["C"], c["K"], c["mus_grid"], **c["kw"])
    dp, dl, dpts = _dev(c["p"]), _dev_lists(c["lists"]), _pts(c["pts"])
    jac, val, bk = eng.sample_grad(dp, dl, dpts, want_values=True, want_batch=True)
    img = eng.sample(dp, dl, dpts)
    torch.cuda.synchronize()
    N, d = c["pts"].shape
    assert tuple(jac.shape) == (N, d, c["C"]) and tuple(val.shape) == (N, c["C"]) and bk.dtype == torch.int32
    J, V, B = jac.cpu().numpy(), val.cpu().numpy(), bk.cpu().numpy()
    assert np.array_equal(B, bid)                              # point_mapping's ids, -1 outside
    assert (J[~inside] == 0).all() and (V[~inside] == 0).all() and (B[~inside] == -1).all()
    dead = bid == EMPTY
    assert dead.any() and (J[dead] == 0).all() and (V[dead] == 0).all() and (B[dead] == EMPTY).all()
    assert np.isfinite(J).all() and np.isfinite(V).all()
    assert np.abs(J).max() > 0.05
    # values put on the lattice are smoe_shared_sample's float image, bit for bit, at EVERY point
    assert np.array_equal(_lattice(V).view(np.uint32), _bits32(img))
    dJ = np.abs(J.astype(np.float64) - ref64["jac"]).max(axis=(1, 2))
    dV = np.abs(V.astype(np.float64) - ref64["v"]).max(axis=1)
    _bound(dJ, dV, ref32, ref64, loose, CASE_IDS[i])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. a point's result does not depend on its place in the list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[1], IMAGES[2], IMAGES[3]], ids=[_name(c) for c in (IMAGES[1], IMAGES[2], IMAGES[3])])
def test_order_independence(image):
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    rng = np.random.default_rng(17)
    pts = (rng.uniform(-0.03, 1.03, size=(6000, len(shape))) * np.array(shape)).astype(np.float32)
    perm = rng.permutation(pts.shape[0])
    _, bid, _ = point_mapping(pts, shape, bshape)
    assert len(np.unique(bid[perm][:1024])) > NB // 2         # a workgroup meets many batches, a lane several

    def run(a):
        r = eng.sample_grad(dp, dl, _pts(a), want_values=True, want_batch=True)
        torch.cuda.synchronize()
        return [_bits32(t) for t in r]

    base = run(pts)
    third = np.arange(0, pts.shape[0], 3)
    for sel in (perm, np.arange(1, pts.shape[0]), third, np.array([4321])):
        got = run(pts[sel])
        for g, b in zip(got, base):
            assert np.array_equal(g, b[sel])
    assert (base[2].view(np.int32)[bid < 0] == -1).all() and np.abs(base[0].view(np.float32)).max() > 0.01
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. ownership at the batch boundaries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[0], IMAGES[4]], ids=[_name(c) for c in (IMAGES[0], IMAGES[4])])
def test_ownership_at_batch_boundaries(image):
    """the disjoint parity lists of tests/test_gpu_shared_sample.py: neighbours on either axis list disjoint kernels, so the
    Jacobian with the owner's list differs from the one with the neighbour's"""
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, _, _ = _setup(shape, bshape, C_, kpd)
    p["pis"] = np.abs(p["pis"]) + np.float32(0.01)
    p["A_diagonal"] = np.ascontiguousarray(np.broadcast_to(np.eye(2, dtype=np.float32) * 1.5, p["A_diagonal"].shape))
    p["A_corr"] = np.zeros_like(p["A_corr"])
    grid = _grid(shape, bshape)
    colour = np.add.outer(np.arange(grid[0]), np.arange(grid[1])).reshape(-1) % 2
    lists = (np.arange(K)[None, :] % 2) == colour[:, None]
    eng = _engine(shape, bshape, C_, K)
    S0, S1, n0, n1 = shape[0], shape[1], bshape[0], bshape[1]
    pts, want, other = [], [], []
    mid1, mid0 = np.float32(n1 * 1.5), np.float32(n0 * 0.5)
    for g in range(1, grid[0]):
        on = np.float32(g * n0)
        pts += [[on, mid1], [np.nextafter(on, np.float32(-np.inf)), mid1]]
        want += [g * grid[1] + 1, (g - 1) * grid[1] + 1]
        other += [(g - 1) * grid[1] + 1, g * grid[1] + 1]
    for g in range(1, grid[1]):
        on = np.float32(g * n1)
        pts += [[mid0, on], [mid0, np.nextafter(on, np.float32(-np.inf))]]
        want += [g, g - 1]
        other += [g - 1, g]
    for k in (1, 8, 17):
        pts += [[np.float32(S0 - 2.0 ** -k), mid1], [mid0, np.float32(S1 - 2.0 ** -k)]]
        want += [(grid[0] - 1) * grid[1] + 1, grid[1] - 1]
        other += [(grid[0] - 2) * grid[1] + 1, grid[1] - 2]
    pts = np.array(pts, dtype=np.float32)
    want, other = np.array(want), np.array(other)
    inside, bid, u = point_mapping(pts, shape, bshape)
    assert inside.all() and np.array_equal(bid, want) and (colour[want] != colour[other]).all()
    jac, val, bk = eng.sample_grad(_dev(p), _dev_lists(lists), _pts(pts), want_values=True, want_batch=True)
    torch.cuda.synchronize()
    J, V = jac.cpu().numpy().astype(np.float64), val.cpu().numpy().astype(np.float64)
    assert np.array_equal(bk.cpu().numpy(), want)
    own32, own64, nb64 = (shared_points_grad_reference(p, lists, u, b, shape, cfg, T)
                          for b, T in ((want, np.float32), (want, np.float64), (other, np.float64)))
    loose = own64["loose"]
    assert not loose.any()
    _bound(np.abs(J - own64["jac"]).max(axis=(1, 2)), np.abs(V - own64["v"]).max(axis=1), own32, own64, loose, _name(image))
    gap = np.abs(own64["jac"] - nb64["jac"]).max(axis=(1, 2))
    assert (np.abs(J - nb64["jac"]).max(axis=(1, 2)) > 0.5 * gap).all() and (gap > 1e-4).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. counts, guard bytes, no lists, points outside
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[1], IMAGES[3]], ids=[_name(c) for c in (IMAGES[1], IMAGES[3])])
def test_counts_and_guard_bytes(image):
    from steered_mixture_of_experts_amd import _lib
    shape, bshape, C_, kpd = image
    d = len(shape)
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    lib = _lib.load()
    dp, dl = _dev(p), _dev_lists(lists)
    cp = eng._cparams(dp)
    rng = np.random.default_rng(23)
    allp = (rng.uniform(-0.02, 1.02, size=(3077, d)) * np.array(shape)).astype(np.float32)
    dpts = _pts(allp)
    full = [t.cpu().numpy() for t in eng.sample_grad(dp, dl, dpts, want_values=True, want_batch=True)]
    torch.cuda.synchronize()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(n, jac, values, batch, lists_t=dl):
        return lib.smoe_shared_sample_grad(eng._h, C.byref(cp), vp(lists_t), vp(dpts), n, vp(jac), vp(values), vp(batch), None)

    for n in (1, 255, 257, 1025, 3077):
        for shift in (0, 1, 3):                                # 16-byte aligned bases, and offset by one / three elements
            jbuf, jview = _guarded((n, d, C_), torch.float32, SENT, shift=shift)
            vbuf, vview = _guarded((n, C_), torch.float32, SENT, shift=shift)
            bbuf, bview = _guarded((n,), torch.int32, 77, shift=shift)
            jbuf2, jview2 = _guarded((n, d, C_), torch.float32, SENT, shift=shift)
            assert call(n, jview, vview, bview) == 0, lib.smoe_last_error()
            assert call(n, jview2, None, None) == 0, lib.smoe_last_error()                # without values / batch
            torch.cuda.synchronize()
            for view, want in ((jview, full[0]), (vview, full[1]), (bview, full[2]), (jview2, full[0])):
                assert np.array_equal(_bits32(view), want[:n].view(np.uint32)), (n, shift)
            for b, fill, size in ((jbuf, SENT, n * d * C_), (vbuf, SENT, n * C_), (bbuf, 77, n), (jbuf2, SENT, n * d * C_)):
                flat = b.cpu().numpy()
                assert (flat[:64 + shift] == fill).all() and (flat[64 + shift + size:] == fill).all(), (n, shift)
    # num_points == 0: a no-op that needs no pointers
    assert lib.smoe_shared_sample_grad(eng._h, C.byref(cp), None, None, 0, None, None, None, None) == 0
    assert tuple(eng.sample_grad(dp, dl, dpts[:0]).shape) == (0, d, C_)
    # lists = NULL equals all-ones lists, and differs from the sparse ones
    r1 = eng.sample_grad(dp, eng.new_lists(), dpts)
    r0 = eng.sample_grad(dp, None, dpts)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1) and not np.array_equal(r0.cpu().numpy(), full[0])
    # NaN, negative and >= S points
    bad = np.full((2 * d + 2, d), 1.5, np.float32)
    for l in range(d):
        bad[2 * l, l], bad[2 * l + 1, l] = -1e-6, shape[l]
    bad[2 * d, 0], bad[2 * d + 1, d - 1] = np.nan, np.inf
    j, v, b = eng.sample_grad(dp, dl, _pts(bad), want_values=True, want_batch=True)
    torch.cuda.synchronize()
    assert (j == 0).all() and (v == 0).all() and (b == -1).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. views
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[0], IMAGES[1], IMAGES[4]], ids=[_name(c) for c in (IMAGES[0], IMAGES[1], IMAGES[4])])
def test_views_of_a_2d_model(image):
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    whole = [(0.0, float(s)) for s in shape]
    inner = [(1.25, 1.25 + (shape[0] - 3)), (bshape[1] + 0.75, bshape[1] + 0.75 + (shape[1] - bshape[1] - 2))]
    thumb_E = [max(1, g // 2) for g in _grid(shape, bshape)]
    # the whole image at 1x (the pixel centres), a window that starts inside a batch, a thumbnail whose samples sit ON batch
    # boundaries: positions exact in float32 -- the same positions as points, bit for bit
    for w, e in ((whole, list(shape)), (inner, [2 * (shape[0] - 3), 2 * (shape[1] - bshape[1] - 2)]), (whole, thumb_E)):
        ax, ab, xs = _view_tables(shape, bshape, w, e)
        pts = np.stack(np.meshgrid(*xs, indexing="ij"), axis=-1).reshape(-1, 2)
        assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
        _, bid, u = point_mapping(pts, shape, bshape)          # the tables equal the point formula, bitwise
        tab_bid = np.ravel_multi_index(tuple(np.meshgrid(*ab, indexing="ij")), _grid(shape, bshape)).reshape(-1)
        tab_u = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)
        assert np.array_equal(bid, tab_bid) and np.array_equal(tab_u.view(np.uint32), u.view(np.uint32))
        vj, vv, vb = eng.render_view_grad(dp, dl, *_dev_view(ax, ab), want_values=True, want_batch=True)
        sj, sv, sb = eng.sample_grad(dp, dl, _pts(pts), want_values=True, want_batch=True)
        torch.cuda.synchronize()
        assert tuple(vj.shape) == tuple(e) + (2, C_) and tuple(vv.shape) == tuple(e) + (C_,) and tuple(vb.shape) == tuple(e)
        assert np.array_equal(_bits32(vj).reshape(-1, 2, C_), _bits32(sj)) and np.array_equal(_bits32(vv).reshape(-1, C_), _bits32(sv))
        assert np.array_equal(vb.cpu().numpy().reshape(-1), sb.cpu().numpy()) and np.abs(sj.cpu().numpy()).max() > 0.01
    eng.close()


def test_one_frame_of_the_3d_model():
    shape, bshape, C_, kpd = IMAGES[3]
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    sj, sv = eng.sample_grad(dp, dl, _pts(_centres(shape)), want_values=True)
    sj, sv = sj.reshape(shape + (3, C_)), sv.reshape(shape + (C_,))
    for t in (2, 5):                                           # a frame of the first and of the second batch on t
        win = [(0.0, float(shape[0])), (0.0, float(shape[1])), (float(t), float(t + 1))]
        ax, ab, _ = _view_tables(shape, bshape, win, [shape[0], shape[1], 1])
        vj, vv = eng.render_view_grad(dp, dl, *_dev_view(ax, ab), want_values=True)
        torch.cuda.synchronize()
        assert tuple(vj.shape) == (shape[0], shape[1], 1, 3, C_)
        assert np.array_equal(_bits32(vj)[:, :, 0], _bits32(sj[:, :, t].contiguous()))
        assert np.array_equal(_bits32(vv)[:, :, 0], _bits32(sv[:, :, t].contiguous()))
        assert np.abs(vj.cpu().numpy()[..., 2, :]).max() > 0.01                          # dv / dt
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the argument checks with a real handle
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_with_a_handle():
    """every refusal of the two entry points, and a correct call after each.  (The 160 KB LDS limit is the one a handle cannot
    reach: the plan's limit is checked on the host, tests/host/shared_sample_grad_args_driver.cpp.)"""
    from steered_mixture_of_experts_amd import _lib
    shape, bshape, C_, kpd = IMAGES[0]
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    lib = _lib.load()
    assert lib.smoe_abi_version() == 2
    dp, dl = _dev(p), _dev_lists(lists)
    cp = eng._cparams(dp)
    bad = eng._cparams(dp)
    bad.gamma_e = None
    dpts = _pts(_centres(shape)[:64])
    want = _bits32(eng.sample_grad(dp, dl, dpts))
    buf, view = _guarded((64, 2, C_), torch.float32, SENT)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def sample(h=eng._h, params=cp, pts=dpts, n=64, jac=view):
        return lib.smoe_shared_sample_grad(h, None if params is None else C.byref(params), vp(dl), vp(pts), n, vp(jac), None, None, None)

    def good(fn):
        buf.fill_(SENT)
        assert fn() == 0, lib.smoe_last_error()
        torch.cuda.synchronize()

    for kwargs, code, word in [(dict(h=C.c_void_p(None)), _lib.SMOE_ERR_INVALID, b"handle"),
                               (dict(params=None), _lib.SMOE_ERR_INVALID, b"p "), (dict(params=bad), _lib.SMOE_ERR_INVALID, b"p "),
                               (dict(pts=None), _lib.SMOE_ERR_INVALID, b"points"), (dict(jac=None), _lib.SMOE_ERR_INVALID, b"jac"),
                               (dict(n=-1), _lib.SMOE_ERR_INVALID, b"num_points"),
                               (dict(n=1 << 41), _lib.SMOE_ERR_UNSUPPORTED, b"2^31")]:
        buf.fill_(SENT)
        assert sample(**kwargs) == code, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_sample_grad" in err and word in err, (kwargs, err)
        torch.cuda.synchronize()
        assert (buf == SENT).all()                             # nothing was written
        good(sample)                                           # the call after a refused one succeeds
        assert np.array_equal(_bits32(view), want)
    assert sample(n=0, pts=None, jac=None) == 0                # a no-op
    ax, ab, _ = _view_tables(shape, bshape, [(0.0, 8.0), (0.0, 8.0)], (8, 8))
    dax, dab = _dev_view(ax, ab)
    vwant = _bits32(eng.render_view_grad(dp, dl, dax, dab))
    vbuf, vview = _guarded((8, 8, 2, C_), torch.float32, SENT)
    slots = lambda ts: (C.c_void_p * 3)(*([None if t is None else t.data_ptr() for t in ts] + [None] * (3 - len(ts))))
    ext3 = lambda e: (C.c_int32 * 3)(*(list(e) + [1] * (3 - len(e))))

    def view_grad(h=eng._h, params=cp, ext=ext3((8, 8)), axes=slots(dax), batches=slots(dab), jac=vview):
        return lib.smoe_shared_render_view_grad(h, None if params is None else C.byref(params), vp(dl), ext, axes, batches,
                                                vp(jac), None, None, None)

    for kwargs, code, word in [(dict(h=C.c_void_p(None)), _lib.SMOE_ERR_INVALID, b"handle"),
                               (dict(params=None), _lib.SMOE_ERR_INVALID, b"p "), (dict(ext=None), _lib.SMOE_ERR_INVALID, b"extent"),
                               (dict(axes=None), _lib.SMOE_ERR_INVALID, b"axis_coords"), (dict(batches=None), _lib.SMOE_ERR_INVALID, b"axis_batch"),
                               (dict(jac=None), _lib.SMOE_ERR_INVALID, b"jac"),
                               (dict(ext=ext3((8, 0))), _lib.SMOE_ERR_INVALID, b"extent[1]"),
                               (dict(axes=slots([dax[0], None])), _lib.SMOE_ERR_INVALID, b"axis_coords[1]"),
                               (dict(batches=slots([None, dab[1]])), _lib.SMOE_ERR_INVALID, b"axis_batch[0]"),
                               (dict(ext=ext3((2 ** 31 - 1, 2 ** 31 - 1))), _lib.SMOE_ERR_UNSUPPORTED, b"2^31")]:
        vbuf.fill_(SENT)
        assert view_grad(**kwargs) == code, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_render_view_grad" in err and word in err, (kwargs, err)
        torch.cuda.synchronize()
        assert (vbuf == SENT).all()
        assert view_grad() == 0, lib.smoe_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_bits32(vview), vwant)
    wide = _engine((16, (1 << 24) + 16), (16, 16), 1, 1)       # an axis the point form cannot resolve exactly in fp32
    wp = {k: torch.zeros_like(v[:1]) for k, v in dp.items()}
    wcp = wide._cparams(wp)
    assert sample(h=wide._h, params=wcp) == _lib.SMOE_ERR_UNSUPPORTED and b"2^24" in lib.smoe_last_error()
    wide.close()
    # the engine's own checks
    with pytest.raises(ValueError):
        eng.sample_grad(dp, dl[:3], dpts)
    with pytest.raises(ValueError):
        eng.sample_grad(dp, dl, dpts.cpu())
    with pytest.raises(ValueError):
        eng.sample_grad(dp, dl, dpts, out=torch.empty((64, C_, 2), device="cuda"))
    with pytest.raises(ValueError):
        eng.render_view_grad(dp, dl, dax, dab[:1])
    with pytest.raises(ValueError):
        eng.render_view_grad(dp, dl, dax, [dab[0], dab[1][:4]])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. the facade on the device
# ---------------------------------------------------------------------------------------------------------------
def test_facade_on_the_device():
    from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
    shape, bshape, C_ = (64, 96), (32, 32), 3
    b = synthetic_blocks(24, (16, 16), C_, 3)
    img = blk.blocks_to_image(b, shape, (16, 16))
    s = SharedSmoe(img, kernels_per_dim=[6, 8], train_inverse_cov=False, batch_size=list(bshape), use_determinant=True, use_yuv=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(0.01))
    s.train(6, val_iter=3, ukl_iter=3)
    rec = s.render()
    centres = _centres(shape).reshape(shape + (2,))
    J, V = s.eval_points_grad(centres, want_values=True)
    assert J.shape == shape + (2, C_) and V.shape == rec.shape and J.dtype == np.float32 and np.abs(J).max() > 1e-3
    assert np.array_equal(_lattice(V).view(np.uint32), rec.view(np.uint32))              # render(), bit for bit
    Jv, Vv = s.eval_view_grad(None, want_values=True)
    assert np.array_equal(Jv.view(np.uint32), J.view(np.uint32)) and np.array_equal(Vv.view(np.uint32), V.view(np.uint32))
    c, sn = np.cos(np.deg2rad(30)) / 1.3, np.sin(np.deg2rad(30)) / 1.3
    M = np.array([[c, -sn], [sn, c]])
    A = np.concatenate([M, (np.array([32.0, 48.0]) - M @ np.array([30.0, 45.0]))[:, None]], axis=1)
    src = s.eval_warp_grad(A, (60, 90))
    view, vals = s.eval_warp_grad(A, (60, 90), wrt="view", want_values=True, to_host=False)
    assert view.is_cuda and vals.is_cuda and tuple(view.shape) == (60, 90, 2, C_)
    want = np.einsum("...lc,lm->...mc", src.astype(np.float64), M)
    assert np.abs(view.cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max() and (src == 0).all(axis=(2, 3)).any()
    assert np.array_equal(_lattice(vals.cpu().numpy()).view(np.uint32), s.eval_warp(A, (60, 90)).view(np.uint32))
