"""GPU tests of the point derivative (smoe_sample_grad through the C ABI and the facade): independence of a point from the list
it comes in and from the path the workgroup takes (staged / direct records), blend against plain, parity with the numpy
restatement (tests/sample_grad_engine.py) on rotated point sets, consistency with smoe_sample, bounds / alignment / argument
checks with a real handle, and the facade.

Parity criterion.  The restatement is evaluated in float32 and float64; with ``e32 = max |J32 - J64|`` outside the loose set
(tests/sample_grad_engine.py), the kernel must satisfy ``|J_gpu - J64| <= F * e32`` there, and ``values`` against ``v64`` with
their own ``e32``.  F: the hardware exp2 / reciprocal are 1-ulp approximations where numpy rounds correctly and the kernel's
fused multiply-adds associate differently, so the kernel may sit a few times farther from float64 than numpy's float32 does;
more than four bits (16) would be a wrong term.  F is twice the largest ratio measured on the MI355X, rounded up to a power of
two: 2.64 for J (16x16 C 3, blend 2; 0.66 ... 1.91 elsewhere), 1.79 for the values, so F = 8
(profiles/render/sample_grad_parity.txt lists the ratios per case).  Condition on the inputs, asserted on the restatement
alone before the GPU is compared: loose share < 0.01.  Loose points must be finite; outside points are 0 / 0 / -1 exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import smoe_oracle as o
from render_cases import _guarded, _image
from sample_grad_cases import CASES, CASE_IDS, case_inputs, case_reference
from steered_mixture_of_experts_amd import blocks as blk
from test_gpu_render_view import _open
from test_gpu_sample import _dev, _rotated

pytestmark = pytest.mark.gpu

F = 8.0


def _grad(eng, dp, act, grid, shape, pts, **kw):
    """Jacobian, values, block of the points (host array or device tensor) on the blocks' whole footprint"""
    length = [g * n for g, n in zip(grid, shape)]
    return eng.sample_grad(dp, act, grid, length, pts if torch.is_tensor(pts) else _dev(pts), want_values=True, want_block=True, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. independence: a point's result does not depend on the list it comes in, nor on the path its workgroup takes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_a_point_owes_nothing_to_the_other_points_or_to_the_path(beta, monkeypatch):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    monkeypatch.delenv("SMOE_SAMPLE_RECORDS", raising=False)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    assert int(np.prod(grid)) == 12
    length = [g * n for g, n in zip(grid, shape)]
    pts = _rotated(shape, grid, (61, 83), 17.0, 1.7)
    inside, g, _u = blk.point_blocks(pts, shape, grid, length)
    assert inside.all()
    own = np.ravel_multi_index(tuple(g.T), grid)
    assert len(np.unique(own)) == 12
    # sorted by block: the staged path by construction -- the record budget of this triple holds all 12 blocks
    order = np.argsort(own, kind="stable")
    base = [t.cpu().numpy() for t in _grad(eng, dp, act, grid, shape, pts[order], blend=beta)]
    assert base[0].shape == (len(pts), 2, C_) and (base[2] == own[order]).all() and base[0].any() and base[1].any()

    def same(res, index, what):
        for a, b in zip(res, base):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b[index].view(np.uint8)), what

    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    same(_grad(eng, dp, act, grid, shape, pts, blend=beta), inv, "row-major order")
    perm = np.random.default_rng(11).permutation(len(pts))
    same(_grad(eng, dp, act, grid, shape, pts[perm], blend=beta), inv[perm], "a random permutation")
    same(_grad(eng, dp, act, grid, shape, pts[::3], blend=beta), inv[::3], "every third point")
    same(_grad(eng, dp, act, grid, shape, pts[17:18], blend=beta), inv[17:18], "one point")
    # the direct path by construction: every workgroup's 512 shuffled points span more than 4 blocks, and 0 never stages
    for lo in range(0, len(perm), 512):
        gg = g[perm[lo:lo + 512]]
        assert np.prod(gg.max(axis=0) - gg.min(axis=0) + 1) > 4
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "4")
    same(_grad(eng, dp, act, grid, shape, pts[perm], blend=beta), inv[perm], "shuffled, at most 4 records staged")
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "0")
    same(_grad(eng, dp, act, grid, shape, pts[order], blend=beta), np.arange(len(order)), "sorted, nothing staged")
    same(_grad(eng, dp, act, grid, shape, pts, blend=beta), inv, "row-major, nothing staged")
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. blend against plain: outside every band the blended call has the bits of the plain one
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 3], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_points_outside_every_band_have_the_bits_of_the_plain_call(i):
    c = case_inputs(i, True)
    eng, dp, act, grid, _ = _open(tuple(c["shape"]), c["C"], c["kpd"], c["opt"])
    plain = [t.cpu().numpy() for t in _grad(eng, dp, act, grid, c["shape"], c["pts"])]
    blend = [t.cpu().numpy() for t in _grad(eng, dp, act, grid, c["shape"], c["pts"], blend=c["beta"])]
    # the neighbour weights of the restatement's float32 windows
    from blend_render_engine import axis_weights
    inside, g, u = blk.point_blocks(c["pts"], c["shape"], c["grid"], c["length"])
    bl = [float(v) for v in np.atleast_1d(c["beta"])]
    bl = bl * len(c["shape"]) if len(bl) == 1 else bl
    free = inside.copy()
    for l, n in enumerate(c["shape"]):
        w = axis_weights(n, u[:, l], bl[l])
        there = (g[:, l] + np.where(w > 0, 1, -1) >= 0) & (g[:, l] + np.where(w > 0, 1, -1) < grid[l])
        free &= ~((np.abs(w) > 0) & there)
    assert 0.1 < free[inside].mean() < 0.9
    for a, b in zip(plain, blend):
        assert np.array_equal(a[free].view(np.uint8), b[free].view(np.uint8))
    assert not np.array_equal(plain[0][inside & ~free], blend[0][inside & ~free])          # the blend acts
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. / 4. rotated point sets against the restatement; consistency with smoe_sample
# ---------------------------------------------------------------------------------------------------------------
def rotated_conditions(ref, ref64, n_out, npts):
    """The condition on the inputs, asserted on the restatement alone: the blocks of the two precisions agree, ``n_out`` points
    lie outside, loose share < 0.01, and numpy's float32 differs from float64 outside the loose set.  Returns (loose, outside,
    eJ, eV)."""
    outside = ref64["block"] < 0
    loose = ref64["loose"]
    assert outside.sum() == n_out and np.array_equal(ref64["block"], ref["block"])
    print(f"restatement: loose share {loose.mean():.2e}, near the floor of the normaliser {ref64['floor'].mean():.2e}, "
          f"outside {outside.sum()} of {npts}")
    assert loose.mean() < 0.01
    eJ = np.abs(ref["jac"].astype(np.float64) - ref64["jac"])[~loose].max()
    eV = np.abs(ref["v"].astype(np.float64) - ref64["v"])[~loose].max()
    assert eJ > 0 and eV > 0
    return loose, outside, eJ, eV


def judge_rotated(ref64, loose, outside, eJ, eV, jac, val, bk, img):
    """the criterion of the module's docstring on the kernel's Jacobian, values and block ids, and the values against
    smoe_sample's image ``img`` (host arrays)"""
    assert jac.shape == ref64["jac"].shape and val.shape == ref64["v"].shape
    dJ, dV = np.abs(jac - ref64["jac"]), np.abs(val - ref64["v"])
    print(f"kernel: max |J| {np.abs(ref64['jac']).max():.3f} per pixel; J: e32 {eJ:.2e}, kernel {dJ[~loose].max():.2e}, ratio "
          f"{dJ[~loose].max() / eJ:.2f}; values: e32 {eV:.2e}, kernel {dV[~loose].max():.2e}, ratio {dV[~loose].max() / eV:.2f}; "
          f"on the loose set J {dJ[loose].max() if loose.any() else 0:.2e}")
    assert np.isfinite(jac).all() and np.isfinite(val).all()
    assert (dJ[~loose] <= F * eJ).all(), dJ[~loose].max() / eJ
    assert (dV[~loose] <= F * eV).all(), dV[~loose].max() / eV
    assert np.array_equal(bk, ref64["block"])
    assert (jac[outside] == 0).all() and (val[outside] == 0).all() and (bk[outside] == -1).all()
    # consistency with smoe_sample: the value before the lattice rounds onto its image
    lsb = 1.0 / 255
    frac = (ref64["v"] * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    dd = np.abs(o.fake_quant01(val, 8, np.float32) - img)
    print(f"against smoe_sample: tie share {tie.mean():.2e}, samples that differ {(dd > 1e-7).mean():.2e}")
    assert (dd[~tie] < 1e-7).all(), dd[~tie].max()
    assert (dd <= lsb * 1.0001).all(), dd.max()


@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_rotated_points_against_the_restatement(i, blended):
    c = case_inputs(i, blended)
    ref, ref64 = case_reference(i, blended)
    shape, C_ = c["shape"], c["C"]
    loose, outside, eJ, eV = rotated_conditions(ref, ref64, c["n_out"], len(c["pts"]))

    eng, dp, act, grid, _ = _open(tuple(shape), C_, c["kpd"], c["opt"])
    jac, val, bk = _grad(eng, dp, act, grid, shape, c["pts"], blend=c["beta"])
    img = eng.sample(dp, act, grid, c["length"], _dev(c["pts"]), blend=c["beta"])
    torch.cuda.synchronize()
    jac, val, bk, img = jac.cpu().numpy(), val.cpu().numpy(), bk.cpu().numpy(), img.cpu().numpy()
    assert jac.shape == (len(c["pts"]), len(shape), C_) and val.shape == (len(c["pts"]), C_)
    judge_rotated(ref64, loose, outside, eJ, eV, jac, val, bk, img)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. / 6. bounds, alignment, argument checks with a handle
# ---------------------------------------------------------------------------------------------------------------
SENT = -7.0


def _raw_call(eng, dp, act, grid, length, blend=None):
    lib = eng.lib
    cp = eng._cparams(dp)
    d = len(grid)
    g3 = (C.c_int32 * 3)(*(list(grid) + [1] * (3 - d)))
    l3 = (C.c_int32 * 3)(*(list(length) + [1] * (3 - d)))
    bl = None
    if blend is not None:
        v = [float(x) for x in np.atleast_1d(blend)]
        bl = (C.c_float * 3)(*((v * d if len(v) == 1 else v) + [0.0] * (3 - d)))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points, n, jac, values=None, block=None, params=cp, grid_=g3, length_=l3, blend_=bl, handle=eng._h):
        return lib.smoe_sample_grad(handle, None if params is None else C.byref(params), C.c_void_p(act.data_ptr()), grid_, length_,
                                    ptr(points), n, blend_, ptr(jac), ptr(values), ptr(block), None)
    return call


@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_bounds_and_alignment(beta):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    length = [g * n for g, n in zip(grid, shape)]
    allpts = _rotated(shape, grid, (61, 83), -31.0, 0.8)                     # some of them outside
    assert not blk.point_blocks(allpts, shape, grid, length)[0].all()
    call = _raw_call(eng, dp, act, grid, length, beta)
    lib = eng.lib
    for N in (0, 1, 255, 257, 3 * 1024 + 5):
        pts = _dev(allpts[:N])
        if N:
            base, base_v, base_bk = _grad(eng, dp, act, grid, shape, pts, blend=beta)
        for shift in (0, 1, 3):
            jbuf, jview = _guarded((N, 2, C_), torch.float32, SENT, shift=shift)
            vbuf, vview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            bbuf, bview = _guarded((N,), torch.int32, -9, shift=shift)
            jonly, jonly_view = _guarded((N, 2, C_), torch.float32, SENT, shift=shift)
            assert call(pts, N, jview, vview, bview) == 0, lib.smoe_last_error()
            assert call(pts, N, jonly_view) == 0, lib.smoe_last_error()          # values and block are optional
            torch.cuda.synchronize()
            for b_, fill, n in [(jbuf, SENT, N * 2 * C_), (vbuf, SENT, N * C_), (bbuf, -9, N), (jonly, SENT, N * 2 * C_)]:
                flat = b_.cpu().numpy()
                assert (flat[:64 + shift] == fill).all() and (flat[64 + shift + n:] == fill).all(), (N, shift)   # nothing outside
            if N:
                assert torch.equal(jview.view(torch.int32), base.view(torch.int32)) and torch.equal(vview.view(torch.int32), base_v.view(torch.int32))
                assert torch.equal(bview, base_bk) and torch.equal(jonly_view.view(torch.int32), base.view(torch.int32))
                assert (bview != -9).all() and (jview != SENT).all() and (vview != SENT).all()
    eng.close()


def test_argument_checks_with_a_handle():
    from steered_mixture_of_experts_amd import _lib
    shape, C_, kpd = (16, 16), 3, (2, 2)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    length = [g * n for g, n in zip(grid, shape)]
    pts = _dev(_rotated(shape, grid, (61, 83), 17.0, 1.7)[:300])
    N = 300
    call = _raw_call(eng, dp, act, grid, length, 2)
    lib = eng.lib
    jbuf, jview = _guarded((N, 2, C_), torch.float32, SENT)
    vbuf, vview = _guarded((N, C_), torch.float32, SENT)
    bbuf, bview = _guarded((N,), torch.int32, -9)
    i3 = lambda v: (C.c_int32 * 3)(*v)
    f3 = lambda v: (C.c_float * 3)(*v)
    invalid = [
        (dict(params=None), b"p "), (dict(points=None), b"points"), (dict(jac=None), b"jac"), (dict(grid_=None), b"grid"),
        (dict(length_=None), b"length"), (dict(grid_=i3([0, 4, 1])), b"grid[0]"), (dict(grid_=i3([65536, 65536, 1])), b"2^31"),
        (dict(length_=i3([48, 0, 1])), b"length[1]"), (dict(length_=i3([49, 64, 1])), b"length[0]"),
        (dict(n=-1), b"num_points"), (dict(blend_=f3([float("nan"), 0.0, 0.0])), b"blend[0]"),
        (dict(blend_=f3([1.0, -0.5, 0.0])), b"blend[1]"), (dict(blend_=f3([1.0, shape[1] / 2 + 0.01, 0.0])), b"blend[1]"),
        (dict(handle=None), b"handle"),
    ]
    unsupported = [
        (dict(grid_=i3([3, 2 ** 20 + 1, 1])), b"2^24"),                        # block origins would not be exact in fp32
        (dict(n=2 ** 40), b"2^31"),                                            # 2^31 workgroups; refused before anything is read
    ]
    for cases, code in ((invalid, _lib.SMOE_ERR_INVALID), (unsupported, _lib.SMOE_ERR_UNSUPPORTED)):
        for kwargs, word in cases:
            kw = dict(points=pts, n=N, jac=jview, values=vview, block=bview)
            kw.update(kwargs)
            assert call(**kw) == code, kwargs
            assert word in lib.smoe_last_error() and b"smoe_sample_grad" in lib.smoe_last_error(), (kwargs, lib.smoe_last_error())
    # no points: nothing is needed, nothing is written
    assert call(None, 0, None) == 0 and call(pts, 0, jview, vview, bview) == 0
    torch.cuda.synchronize()
    assert (jbuf == SENT).all() and (vbuf == SENT).all() and (bbuf == -9).all()
    # blend NULL and all zero: the plain derivative
    plain = eng.sample_grad(dp, act, grid, length, pts)
    assert torch.equal(eng.sample_grad(dp, act, grid, length, pts, blend=0.0), plain)
    assert not torch.equal(eng.sample_grad(dp, act, grid, length, pts, blend=2), plain)
    for bad in [dict(points=pts[:, :1].contiguous()), dict(points=pts.cpu()), dict(points=pts.double()), dict(grid=[3]),
                dict(blend=(1, 2, 3)), dict(out=torch.empty((N, 2, C_ + 1), device="cuda"))]:
        kw = dict(params=dp, active=act, grid=grid, length=length, points=pts)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.sample_grad(**kw)
    assert lib.smoe_abi_version() == 2
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the facade
# ---------------------------------------------------------------------------------------------------------------
def test_facade_on_the_device():
    from steered_mixture_of_experts_amd.smoe import Adam, Smoe
    img = _image(40, 56, 3)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(4, val_iter=4)
    c, sn = np.cos(np.deg2rad(17)) / 4, np.sin(np.deg2rad(17)) / 4
    M = np.array([[c, -sn], [sn, c]])
    A = np.concatenate([M, (np.array([20.0, 28.0]) - M @ np.array([60.0, 75.0]))[:, None]], axis=1)
    pts = blk.warp_points(A, (120, 150))
    dpts = torch.from_numpy(pts).cuda()
    jac, val = s.sample_grad(dpts, blend=2, to_host=False, want_values=True)
    assert torch.is_tensor(jac) and jac.is_cuda and jac.dtype == torch.float32 and tuple(jac.shape) == (120, 150, 2, 3)
    assert val.is_cuda and tuple(val.shape) == (120, 150, 3) and jac.abs().max() > 1e-3
    # the engine call behind it
    params, active, center = s._whole_model(False)
    ej, ev = s._engine.sample_grad(params, active, s.grid, [40, 56], dpts.reshape(-1, 2), blend=[2.0, 2.0], want_values=True, center_grid=center)
    assert torch.equal(jac.reshape(-1, 2, 3), ej) and torch.equal(val.reshape(-1, 3), ev)
    assert np.array_equal(s.sample_grad(pts, blend=2), jac.cpu().numpy())                     # host array in, host array out
    assert not torch.equal(jac, s.sample_grad(dpts, to_host=False))
    src = s.render_warp_grad(A, (120, 150), blend=2, to_host=False)
    assert torch.equal(src, jac)
    view = s.render_warp_grad(A, (120, 150), wrt="view", blend=2, to_host=False)
    want = torch.einsum("...lc,lm->...mc", jac, torch.from_numpy(M.astype(np.float32)).cuda())
    assert view.is_cuda and torch.equal(view, want)
    # the value before the lattice rounds onto sample()'s image; the padding of the ragged image is outside
    lat = s.sample(dpts, blend=2, to_host=False)
    assert (val - lat).abs().max() <= 0.5 / 255 + 1e-6
    pad = s.render_warp_grad([[1, 0, 0], [0, 1, 0]], (48, 64))
    assert pad.shape == (48, 64, 2, 3) and (pad[40:] == 0).all() and (pad[:, 56:] == 0).all() and pad[:40, :56].any()
    with pytest.raises(ValueError):
        s.sample_grad(pts[..., :1])
