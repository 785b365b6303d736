"""GPU tests of the point decoder (smoe_sample through the C ABI and the facade): bit-identity with smoe_render /
smoe_render_blend on the pixel centres, independence of a point from the list it comes in and from the path the workgroup takes
(staged / direct records), parity with the numpy restatement (tests/sample_engine.py) on rotated point sets, bounds / alignment
/ argument checks with a real handle, and the facade.

Parity criterion on rotated sets = the project's existing one (tests/test_gpu_render_view.py): with
``frac = (v64 * 255 + 0.5) mod 1`` from the float64 restatement, samples are identical (< 1e-7) where ``frac`` is farther than
2e-4 from 0 / 1 and differ by at most one LSB elsewhere.  A sample is loose as well -- held to the one-LSB bound only -- if in
any block with weight on it some kernel's float64 gate lies within 1e-6 of the influence threshold.  Condition on the inputs,
asserted on the restatement alone before the GPU is compared: loose share < 0.01 and no float32-vs-float64 difference of the
restatement outside the loose set."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from render_cases import _axes, _dev_axes, _guarded, _image
from sample_engine import sample_reference
from steered_mixture_of_experts_amd import blocks as blk
from test_gpu_render import SHAPES
from test_gpu_render_view import _model, _open

pytestmark = pytest.mark.gpu


def _centres(extent):
    """every pixel centre of an image of ``extent`` pixels, as points [N, d]"""
    d = len(extent)
    return blk.warp_points(np.concatenate([np.eye(d), np.zeros((d, 1))], axis=1), extent).reshape(-1, d)


def _rotated(shape, grid, E, deg, zoom):
    """x = R(deg) / zoom (i + 0.5 - E / 2) + L / 2 on the first two axes, x_t = i_t L_t / E_t on the third; L: the blocks'
    footprint"""
    d = len(shape)
    L = np.array([g * n for g, n in zip(grid, shape)], dtype=np.float64)
    Ef = np.array(E, dtype=np.float64)
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    A = np.zeros((d, d + 1))
    A[:2, :2] = [[c, -s], [s, c]]
    A[:2, d] = L[:2] / 2 - A[:2, :2] @ (Ef[:2] / 2)
    if d == 3:
        A[2, 2] = L[2] / Ef[2]
        A[2, 3] = -0.5 * A[2, 2]
    return blk.warp_points(A, E).reshape(-1, d)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sample(eng, dp, act, grid, shape, pts, **kw):
    """values, argmax, block of the points (host array or device tensor) on the blocks' whole footprint"""
    length = [g * n for g, n in zip(grid, shape)]
    return eng.sample(dp, act, grid, length, pts if torch.is_tensor(pts) else _dev(pts), want_argmax=True, want_block=True, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. / 2. identity with smoe_render and smoe_render_blend on the training lattice
# ---------------------------------------------------------------------------------------------------------------
LATTICE = [(s[0], s[1], tuple(s[2]), None) for s in SHAPES] \
    + [((16, 16), 3, (2, 2), name) for name in ("train_inverse_cov", "mode2", "mode2_centre_grid")]
LATTICE_IDS = ["x".join(map(str, c[0])) + f"-c{c[1]}-k" + "x".join(map(str, c[2])) + (f"-{c[3]}" if c[3] else "") for c in LATTICE]


def _expected_blocks(shape, grid, extent):
    pos = np.stack(np.meshgrid(*[np.arange(e) // n for e, n in zip(extent, shape)], indexing="ij"), axis=-1).reshape(-1, len(shape))
    return np.ravel_multi_index(tuple(pos.T), grid).astype(np.int32)


@pytest.mark.parametrize("case", LATTICE, ids=LATTICE_IDS)
def test_pixel_centres_are_render_on_the_training_lattice(case):
    shape, C_, kpd, opt = case
    eng, dp, act, grid, keep = _open(shape, C_, kpd, opt)
    extent = [g * n for g, n in zip(grid, shape)]
    axes = _dev_axes(_axes(shape, shape))
    img, am = eng.render(dp, act, axes, grid, extent, want_argmax=True)
    u8 = eng.render(dp, act, axes, grid, extent, dtype=torch.uint8)
    pts = _dev(_centres(extent))
    val, sam, sbk = _sample(eng, dp, act, grid, shape, pts)
    vu8 = eng.sample(dp, act, grid, extent, pts, dtype=torch.uint8)
    torch.cuda.synchronize()
    assert tuple(val.shape) == (pts.shape[0], C_) and val.dtype == torch.float32 and sam.dtype == torch.uint8 and sbk.dtype == torch.int32
    assert torch.equal(val.view(torch.int32), img.reshape(-1, C_).view(torch.int32))    # bit for bit
    assert torch.equal(vu8, u8.reshape(-1, C_)) and torch.equal(sam, am.reshape(-1))
    assert (am != 255).any()
    assert np.array_equal(sbk.cpu().numpy(), _expected_blocks(shape, grid, extent))
    eng.close()


@pytest.mark.parametrize("case", LATTICE, ids=LATTICE_IDS)
def test_pixel_centres_are_render_blend_on_the_training_lattice(case):
    shape, C_, kpd, opt = case
    beta = (2, 2, 1) if len(shape) == 3 else 2
    eng, dp, act, grid, keep = _open(shape, C_, kpd, opt)
    extent = [g * n for g, n in zip(grid, shape)]
    axes = _dev_axes(_axes(shape, shape))
    img, am = eng.render_blend(dp, act, axes, grid, extent, beta, want_argmax=True)
    u8 = eng.render_blend(dp, act, axes, grid, extent, beta, dtype=torch.uint8)
    plain = eng.render(dp, act, axes, grid, extent)
    pts = _dev(_centres(extent))
    val, sam, sbk = _sample(eng, dp, act, grid, shape, pts, blend=beta)
    vu8 = eng.sample(dp, act, grid, extent, pts, blend=beta, dtype=torch.uint8)
    torch.cuda.synchronize()
    assert not torch.equal(img, plain)                                                  # the blend acts
    assert torch.equal(val.view(torch.int32), img.reshape(-1, C_).view(torch.int32))
    assert torch.equal(vu8, u8.reshape(-1, C_)) and torch.equal(sam, am.reshape(-1))
    assert np.array_equal(sbk.cpu().numpy(), _expected_blocks(shape, grid, extent))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. independence: a point's result does not depend on the list it comes in, nor on the path its workgroup takes
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
    # sorted by block: the staged path by construction -- the record budget of this triple holds all 12 blocks, so whatever
    # box a workgroup's points span fits it (csrc/smoe_sample.hip.h: sample_layout)
    order = np.argsort(own, kind="stable")
    base = [t.cpu().numpy() for t in _sample(eng, dp, act, grid, shape, pts[order], blend=beta)]
    assert (base[2] == own[order]).all() and (base[1] != 255).any() and base[0].any()

    def same(res, index, what):
        for a, b in zip(res, base):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b[index].view(np.uint8)), what

    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    same(_sample(eng, dp, act, grid, shape, pts, blend=beta), inv, "row-major order")
    perm = np.random.default_rng(11).permutation(len(pts))
    same(_sample(eng, dp, act, grid, shape, pts[perm], blend=beta), inv[perm], "a random permutation")
    same(_sample(eng, dp, act, grid, shape, pts[::3], blend=beta), inv[::3], "every third point")
    same(_sample(eng, dp, act, grid, shape, pts[17:18], blend=beta), inv[17:18], "one point")
    # the direct path by construction: every workgroup's 1024 shuffled points span more than 4 blocks, and 0 never stages
    for lo in range(0, len(perm), 1024):
        gg = g[perm[lo:lo + 1024]]
        assert np.prod(gg.max(axis=0) - gg.min(axis=0) + 1) > 4
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "4")
    same(_sample(eng, dp, act, grid, shape, pts[perm], blend=beta), inv[perm], "shuffled, at most 4 records staged")
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "0")
    same(_sample(eng, dp, act, grid, shape, pts[order], blend=beta), np.arange(len(order)), "sorted, nothing staged")
    same(_sample(eng, dp, act, grid, shape, pts, blend=beta), inv, "row-major, nothing staged")
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. rotated point sets against the restatement
# ---------------------------------------------------------------------------------------------------------------
ROTATED = [
    # block shape, C, kernels per dim, output E, degrees, zoom, points outside
    ((16, 16), 3, (2, 2), (61, 83), 17.0, 1.7, 0),
    ((16, 16), 1, (2, 2), (61, 83), 17.0, 1.7, 0),
    ((32, 32), 3, (2, 4), (75, 90), -31.0, 0.8, 746),
    ((16, 16, 4), 3, (2, 2, 1), (40, 50, 5), 17.0, 1.3, 570),
    ((7, 5), 1, (2, 2), (33, 29), 40.0, 1.5, 170),
]


@functools.lru_cache(maxsize=None)
def _rotated_reference(i, blended):
    shape, C_, kpd, E, deg, zoom, _ = ROTATED[i]
    cfg, p, K, active, grid, kw, _ = _model(shape, C_, kpd)
    pts = _rotated(shape, grid, E, deg, zoom)
    beta = ((2, 2, 1) if len(shape) == 3 else 2) if blended else None
    length = [g * n for g, n in zip(grid, shape)]
    ref = sample_reference(p, active, list(shape), list(grid), length, pts, beta, cfg, np.float32)
    ref64 = sample_reference(p, active, list(shape), list(grid), length, pts, beta, cfg, np.float64)
    return pts, beta, ref, ref64


def rotated_conditions(ref, ref64, n_out, npts):
    """The condition on the inputs, asserted on the restatement alone: the blocks of the two precisions agree, ``n_out`` points
    lie outside, loose share < 0.01 and no float32-vs-float64 difference outside the loose set.  Returns (loose, outside)."""
    outside = ref["block"] < 0
    assert outside.sum() == n_out and np.array_equal(ref64["block"], ref["block"])
    frac = (ref64["v"] * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    loose = tie | ref64["near_tau"][..., None]
    print(f"restatement: tie share {tie.mean():.2e}, loose share {loose.mean():.2e}, points in a band {ref['banded'].mean():.2f}, "
          f"up to {ref['nblocks'].max()} blocks per point, inside points with no block left "
          f"{((ref['nblocks'] == 0) & ~outside).sum()}, outside {outside.sum()} of {npts}")
    assert loose.mean() < 0.01
    assert (np.abs(ref["recon"] - ref64["recon"])[~loose] < 1e-7).all()
    return loose, outside


def judge_rotated(ref, ref64, loose, outside, img, u8, am, bk):
    """the criterion of the module's docstring on the kernel's float image, uint8 image, kernel map and block ids (host arrays)"""
    lsb = 1.0 / 255
    assert img.shape == ref["recon"].shape
    dd = np.abs(img - ref["recon"].astype(np.float32))
    print(f"kernel: max difference outside the loose set {dd[~loose].max():.3e}, overall {dd.max():.3e}, "
          f"samples that differ {(dd > 1e-7).mean():.2e}")
    assert (dd[~loose] < 1e-7).all(), dd[~loose].max()
    assert (dd <= lsb * 1.0001).all(), dd.max()
    assert np.array_equal(u8, np.rint(img * 255).astype(np.uint8))
    assert np.array_equal(bk, ref["block"])
    # outside points: 0 / 255 / -1 exactly
    assert (img[outside] == 0).all() and (u8[outside] == 0).all() and (am[outside] == 255).all() and (bk[outside] == -1).all()
    # the kernel map is the own block's first maximum, wherever the float64 gates are clear of the threshold (and, with more
    # than one kernel, the two largest are 1e-6 apart)
    wt = ref64["wt0"]
    want_am = np.where(wt.max(axis=-1) > 0, wt.argmax(axis=-1), 255)
    clear = ~ref64["near_tau"]
    if wt.shape[-1] > 1:
        clear = clear & (np.sort(wt, axis=-1)[..., -1] - np.sort(wt, axis=-1)[..., -2] > 1e-6)
    assert np.array_equal(am[clear], want_am[clear])


@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(ROTATED)), ids=[f"case{i + 1}" for i in range(len(ROTATED))])
def test_rotated_points_against_the_restatement(i, blended):
    shape, C_, kpd, E, deg, zoom, n_out = ROTATED[i]
    pts, beta, ref, ref64 = _rotated_reference(i, blended)
    loose, outside = rotated_conditions(ref, ref64, n_out, len(pts))

    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    img, am, bk = _sample(eng, dp, act, grid, shape, pts, blend=beta)
    u8 = eng.sample(dp, act, grid, [g * n for g, n in zip(grid, shape)], _dev(pts), blend=beta, dtype=torch.uint8)
    torch.cuda.synchronize()
    img, u8, am, bk = img.cpu().numpy(), u8.cpu().numpy(), am.cpu().numpy(), bk.cpu().numpy()
    assert img.shape == (len(pts), C_)
    judge_rotated(ref, ref64, loose, outside, img, u8, am, bk)
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

    def call(points, n, values, argmax=None, block=None, fmt=0, params=cp, grid_=g3, length_=l3, blend_=bl, handle=eng._h):
        return lib.smoe_sample(handle, None if params is None else C.byref(params), C.c_void_p(act.data_ptr()), grid_, length_,
                               ptr(points), n, blend_, ptr(values), fmt, ptr(argmax), ptr(block), None)
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
            base, base_am, base_bk = _sample(eng, dp, act, grid, shape, pts, blend=beta)
            base_u8 = eng.sample(dp, act, grid, length, pts, blend=beta, dtype=torch.uint8)
        for shift in (0, 1, 3):
            buf, view = _guarded((N, C_), torch.float32, SENT, shift=shift)
            abuf, aview = _guarded((N,), torch.uint8, 77, shift=shift)
            bbuf, bview = _guarded((N,), torch.int32, -9, shift=shift)
            bufu, viewu = _guarded((N, C_), torch.uint8, 201, shift=shift)
            assert call(pts, N, view, aview, bview) == 0, lib.smoe_last_error()
            assert call(pts, N, viewu, fmt=1) == 0, lib.smoe_last_error()
            torch.cuda.synchronize()
            for b_, fill, n in [(buf, SENT, N * C_), (abuf, 77, N), (bbuf, -9, N), (bufu, 201, N * C_)]:
                flat = b_.cpu().numpy()
                assert (flat[:64 + shift] == fill).all() and (flat[64 + shift + n:] == fill).all(), (N, shift)   # nothing outside
            if N:
                assert torch.equal(view.view(torch.int32), base.view(torch.int32)) and torch.equal(aview, base_am)
                assert torch.equal(bview, base_bk) and torch.equal(viewu, base_u8)
                assert (bview != -9).all() and (view != SENT).all()
    eng.close()


def test_argument_checks_with_a_handle():
    from steered_mixture_of_experts_amd import _lib
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    shape, C_, kpd = (16, 16), 3, (2, 2)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    length = [g * n for g, n in zip(grid, shape)]
    pts = _dev(_rotated(shape, grid, (61, 83), 17.0, 1.7)[:300])
    N = 300
    call = _raw_call(eng, dp, act, grid, length, 2)
    lib = eng.lib
    buf, view = _guarded((N, C_), torch.float32, SENT)
    abuf, aview = _guarded((N,), torch.uint8, 77)
    bbuf, bview = _guarded((N,), torch.int32, -9)
    i3 = lambda v: (C.c_int32 * 3)(*v)
    f3 = lambda v: (C.c_float * 3)(*v)
    invalid = [
        (dict(params=None), b"p "), (dict(points=None), b"points"), (dict(values=None), b"values"), (dict(grid_=None), b"grid"),
        (dict(length_=None), b"length"), (dict(grid_=i3([0, 4, 1])), b"grid[0]"), (dict(grid_=i3([65536, 65536, 1])), b"2^31"),
        (dict(length_=i3([48, 0, 1])), b"length[1]"), (dict(length_=i3([49, 64, 1])), b"length[0]"), (dict(fmt=7), b"image_format"),
        (dict(n=-1), b"num_points"), (dict(blend_=f3([float("nan"), 0.0, 0.0])), b"blend[0]"),
        (dict(blend_=f3([1.0, -0.5, 0.0])), b"blend[1]"), (dict(blend_=f3([1.0, shape[1] / 2 + 0.01, 0.0])), b"blend[1]"),
        (dict(handle=None), b"handle"),
    ]
    unsupported = [
        (dict(grid_=i3([3, 2 ** 20 + 1, 1])), b"2^24"),                        # block origins would not be exact in fp32
        (dict(n=2 ** 41), b"2^31"),                                            # 2^31 workgroups; refused before anything is read
    ]
    for cases, code in ((invalid, _lib.SMOE_ERR_INVALID), (unsupported, _lib.SMOE_ERR_UNSUPPORTED)):
        for kwargs, word in cases:
            kw = dict(points=pts, n=N, values=view, argmax=aview, block=bview)
            kw.update(kwargs)
            assert call(**kw) == code, kwargs
            assert word in lib.smoe_last_error() and b"smoe_sample" in lib.smoe_last_error(), (kwargs, lib.smoe_last_error())
    # no points: nothing is needed, nothing is written
    assert call(None, 0, None) == 0 and call(pts, 0, view, aview, bview) == 0
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (abuf == 77).all() and (bbuf == -9).all()
    # uint8 output needs a lattice of at most 8 bits
    K = int(dp["pis"].shape[1])
    eng10 = BlockEngine(EngineConfig(block_shape=shape, channels=C_, kernels=K, use_yuv=True, precision=10))
    call10 = _raw_call(eng10, dp, act, grid, length)
    assert call10(pts, N, view, fmt=1) == _lib.SMOE_ERR_UNSUPPORTED and b"precision" in lib.smoe_last_error()
    assert call10(pts, N, view) == 0, lib.smoe_last_error()
    # blend NULL and all zero: the plain decoder
    plain = eng.sample(dp, act, grid, length, pts)
    assert torch.equal(eng.sample(dp, act, grid, length, pts, blend=0.0), plain)
    assert not torch.equal(eng.sample(dp, act, grid, length, pts, blend=2), plain)
    for bad in [dict(points=pts[:, :1].contiguous()), dict(points=pts.cpu()), dict(points=pts.double()), dict(grid=[3]), dict(dtype=torch.float64),
                dict(blend=(1, 2, 3)), dict(out=torch.empty((N, C_ + 1), device="cuda"))]:
        kw = dict(params=dp, active=act, grid=grid, length=length, points=pts)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.sample(**kw)
    assert lib.smoe_abi_version() == 2
    torch.cuda.synchronize()
    eng10.close()
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
    recon = s.get_reconstruction()
    ident = [[1, 0, 0], [0, 1, 0]]
    out, ids = s.render_warp(ident, (40, 56), want_argmax=True)
    base, bids = s.render(want_argmax=True)
    assert out.shape == (40, 56, 3) and np.array_equal(out, recon) and np.array_equal(out, base) and np.array_equal(ids, bids)
    assert np.array_equal(s.render_warp(ident, (40, 56), blend=2), s.render(blend=2))
    # the padding of the ragged image is outside
    pad, pids = s.render_warp(ident, (48, 64), want_argmax=True)
    assert np.array_equal(pad[:40, :56], recon) and (pad[40:] == 0).all() and (pad[:, 56:] == 0).all()
    assert (pids[40:] == -1).all() and (pids[:, 56:] == -1).all()
    c, sn = np.cos(np.deg2rad(17)) / 4, np.sin(np.deg2rad(17)) / 4
    M = np.array([[c, -sn], [sn, c]])
    A = np.concatenate([M, (np.array([20.0, 28.0]) - M @ np.array([60.0, 75.0]))[:, None]], axis=1)
    warp, wid = s.render_warp(A, (120, 150), blend=2, to_host=False, want_argmax=True)
    pts = blk.warp_points(A, (120, 150))
    val, vid = s.sample(torch.from_numpy(pts).cuda(), blend=2, to_host=False, want_argmax=True)
    assert torch.is_tensor(warp) and warp.is_cuda and wid.is_cuda and wid.dtype == torch.int64 and tuple(warp.shape) == (120, 150, 3)
    assert torch.equal(warp, val) and torch.equal(wid, vid)
    assert np.array_equal(s.sample(pts, blend=2), warp.cpu().numpy())
    assert not torch.equal(warp, s.render_warp(A, (120, 150), to_host=False))
    u8 = s.render_warp(A, (120, 150), blend=2, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(warp.cpu().numpy() * 255).astype(np.uint8))
    with pytest.raises(ValueError):
        s.sample(pts[..., :1])
