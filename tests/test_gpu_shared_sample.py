"""GPU tests of the shared-mode point and viewport decoders (smoe_shared_sample / smoe_shared_render_view through the C ABI):
bit-identity with smoe_shared_render at its own sample positions, independence of the order of the points, ownership at the
batch boundaries, uint8 / no lists / ragged counts with guard bytes, parity with the CPU restatement on a rotated point set,
views, the argument checks with a real handle, and the facade.

Criterion against the restatement = tests/test_gpu_shared_render.py's: with ``frac = (clip(y64, 0, 1) * 255 + 0.5) mod 1`` from
the float64 restatement, values are identical (< 1e-7) where ``frac`` is farther than 2e-4 from 0 / 1 and no float64 gate lies
within 1e-6 of the influence threshold; at most one LSB elsewhere; the share of such loose samples is capped at 0.01 -- a
condition on the inputs that the restatement alone has to meet first."""
import ctypes as C

import numpy as np
import pytest
import torch

from render_cases import _dev_axes, _guarded
from shared_sample_engine import point_ids, point_mapping, shared_points_reference
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks
from test_gpu_sample import _rotated
from test_gpu_shared_render import EMPTY, IMAGES, OPTIONS, TAU, _dev, _dev_lists, _engine, _grid, _name, _setup, _tables

pytestmark = pytest.mark.gpu

SENT = -7.0


def _centres(shape, scale=1):
    """the sample positions of render_axis(S, scale * S) in source pixels, [prod(scale * shape), d] (exact in float32)"""
    ax = [((np.arange(scale * s, dtype=np.float64) + 0.5) / scale).astype(np.float32) for s in shape]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, len(shape))


def _pts(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits32(t):
    return t.cpu().numpy().view(np.uint32)


def _view_tables(shape, bshape, win, E):
    """per axis the coordinate table, the batch table and the sample positions, as SharedSmoe.eval_view makes them"""
    axes, batches, xs = [], [], []
    for S, n, (lo, hi), e in zip(shape, bshape, win, E):
        axes.append(blk.view_axis(S, 1, S, lo, hi, e)[3])
        first, nblocks, start, _ = blk.view_axis(n, S // n, S, lo, hi, e)
        batches.append((first + np.repeat(np.arange(nblocks), np.diff(start))).astype(np.int32))
        xs.append(lo + (np.arange(e, dtype=np.float64) + 0.5) * ((hi - lo) / e))
    return axes, batches, xs


def _dev_view(axes, batches):
    return _dev_axes(axes), [torch.from_numpy(b).cuda() for b in batches]


# ---------------------------------------------------------------------------------------------------------------
# 1. the render's own positions as points: bit for bit
# ---------------------------------------------------------------------------------------------------------------
IDENTITY = [c + ("plain", {}) for c in IMAGES] + [IMAGES[1] + (n, kw) for n, kw in OPTIONS]


@pytest.mark.parametrize("case", IDENTITY, ids=[_name(c) + "-" + c[4] for c in IDENTITY])
def test_render_positions_as_points_are_the_render(case):
    shape, bshape, C_, kpd, name, kw = case
    img, p, cfg, K, NB, lists, mus_grid = _setup(shape, bshape, C_, kpd, name, **kw)
    eng = _engine(shape, bshape, C_, K, mus_grid, **kw)
    dp, dl = _dev(p), _dev_lists(lists)
    for scale in (1, 2):
        extent = [scale * s for s in shape]
        want, want_ids = eng.render(dp, dl, _dev_axes(_tables(shape, extent)), [scale * b for b in bshape], want_argmax=True)
        pts = _centres(shape, scale)
        out, ids = eng.sample(dp, dl, _pts(pts), want_argmax=True)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (pts.shape[0], C_) and out.dtype == torch.float32 and ids.dtype == torch.int32
        assert np.array_equal(_bits32(out), _bits32(want).reshape(-1, C_)), scale                 # bit for bit
        assert np.array_equal(ids.cpu().numpy(), want_ids.cpu().numpy().reshape(-1)), scale
        _, bid, _ = point_mapping(pts, shape, bshape)
        dead = bid == EMPTY
        assert dead.sum() == scale ** len(shape) * int(np.prod(bshape))
        assert (ids.cpu().numpy()[dead] == -1).all() and (out.cpu().numpy()[dead] == 0).all()     # the empty list: 0 / -1
        assert (ids.cpu().numpy()[~dead] >= 0).mean() > 0.99
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. a point's result does not depend on its place in the list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[1], IMAGES[2], IMAGES[3]], ids=[_name(c) for c in (IMAGES[1], IMAGES[2], IMAGES[3])])
def test_order_independence(image):
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    # off-lattice positions all over the image, some outside
    rng = np.random.default_rng(17)
    pts = (rng.uniform(-0.03, 1.03, size=(6000, len(shape))) * np.array(shape)).astype(np.float32)
    base, bids = eng.sample(dp, dl, _pts(pts), want_argmax=True)
    perm = rng.permutation(pts.shape[0])                       # a workgroup meets many batches, a lane several
    shuf, sids = eng.sample(dp, dl, _pts(pts[perm]), want_argmax=True)
    drop, dids = eng.sample(dp, dl, _pts(pts[1:]), want_argmax=True)       # everything one lane slot and one element on
    torch.cuda.synchronize()
    inside, bid, _ = point_mapping(pts, shape, bshape)
    assert 0.8 < inside.mean() < 0.99 and len(np.unique(bid[perm][:1024])) > NB // 2
    assert np.array_equal(_bits32(shuf), _bits32(base)[perm]) and np.array_equal(sids.cpu().numpy(), bids.cpu().numpy()[perm])
    assert np.array_equal(_bits32(drop), _bits32(base)[1:]) and np.array_equal(dids.cpu().numpy(), bids.cpu().numpy()[1:])
    b, i = base.cpu().numpy(), bids.cpu().numpy()
    assert (b[~inside] == 0).all() and (i[~inside] == -1).all() and (i[inside & (bid != EMPTY)] >= 0).mean() > 0.99
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. ownership at the batch boundaries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[0], IMAGES[4]], ids=[_name(c) for c in (IMAGES[0], IMAGES[4])])
def test_ownership_at_batch_boundaries(image):
    """batch (g0, g1) lists the kernels k with k % 2 == (g0 + g1) % 2 only -- neighbours on either axis have disjoint lists --,
    so the parity of a point's id names the batch that evaluated it"""
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, _, _ = _setup(shape, bshape, C_, kpd)
    p["pis"] = np.abs(p["pis"]) + np.float32(0.01)             # every kernel counts
    p["A_diagonal"] = np.ascontiguousarray(np.broadcast_to(np.eye(2, dtype=np.float32) * 1.5, p["A_diagonal"].shape))
    p["A_corr"] = np.zeros_like(p["A_corr"])                   # wide round kernels: some listed kernel has influence
    grid = _grid(shape, bshape)
    colour = np.add.outer(np.arange(grid[0]), np.arange(grid[1])).reshape(-1) % 2
    lists = (np.arange(K)[None, :] % 2) == colour[:, None]
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    S0, S1, n0, n1 = shape[0], shape[1], bshape[0], bshape[1]
    pts, want = [], []
    mid1 = np.float32(n1 * 1.5)
    for g in range(1, grid[0]):                                # boundaries of the first axis, second axis inside batch 1
        on = np.float32(g * n0)
        pts += [[on, mid1], [np.nextafter(on, np.float32(-np.inf)), mid1]]
        want += [g * grid[1] + 1, (g - 1) * grid[1] + 1]
    mid0 = np.float32(n0 * 0.5)
    for g in range(1, grid[1]):                                # boundaries of the second axis, first axis inside batch 0
        on = np.float32(g * n1)
        pts += [[mid0, on], [mid0, np.nextafter(on, np.float32(-np.inf))]]
        want += [g, g - 1]
    for k in (1, 8, 17):                                       # just inside the far edges
        pts += [[np.float32(S0 - 2.0 ** -k), mid1], [mid0, np.float32(S1 - 2.0 ** -k)], [0.0, 0.0], [-0.0, mid1]]
        want += [(grid[0] - 1) * grid[1] + 1, grid[1] - 1, 0, 1]
    n_in = len(pts)
    pts += [[np.nan, 1], [1, np.nan], [-1e-6, 1], [1, -3], [S0, 1], [1, S1], [np.nextafter(np.float32(S0), np.float32(np.inf)), 1],
            [np.inf, 1], [-np.inf, 1], [1e30, 1e30]]
    pts = np.array(pts, dtype=np.float32)
    assert np.float32(S0 - 2.0 ** -17) < S0                    # the positions near the edge are representable
    inside, bid, _ = point_mapping(pts, shape, bshape)
    assert inside[:n_in].all() and not inside[n_in:].any() and bid[:n_in].tolist() == want     # the host statement agrees
    out, ids = eng.sample(dp, dl, _pts(pts), want_argmax=True)
    torch.cuda.synchronize()
    out, ids = out.cpu().numpy(), ids.cpu().numpy()
    assert (ids[:n_in] >= 0).all(), "a point without influence would not show its batch"
    assert (ids[:n_in] % 2 == colour[np.array(want)]).all(), (ids[:n_in], want)
    assert (out[n_in:] == 0).all() and (ids[n_in:] == -1).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. no lists, uint8, ragged counts, guard bytes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[1], IMAGES[3]], ids=[_name(c) for c in (IMAGES[1], IMAGES[3])])
def test_counts_formats_and_guard_bytes(image):
    from steered_mixture_of_experts_amd import _lib
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    lib = _lib.load()
    dp, dl = _dev(p), _dev_lists(lists)
    cp = eng._cparams(dp)
    rng = np.random.default_rng(23)
    allp = (rng.uniform(-0.02, 1.02, size=(1025, len(shape))) * np.array(shape)).astype(np.float32)
    dpts = _pts(allp)
    full, full_ids = eng.sample(dp, dl, dpts, want_argmax=True)
    torch.cuda.synchronize()
    full, full_ids = full.cpu().numpy(), full_ids.cpu().numpy()

    def call(n, values, arg, fmt=0, lists_t=dl):
        return lib.smoe_shared_sample(eng._h, C.byref(cp), None if lists_t is None else C.c_void_p(lists_t.data_ptr()),
                                      C.c_void_p(dpts.data_ptr()), n, C.c_void_p(values.data_ptr()), fmt,
                                      None if arg is None else C.c_void_p(arg.data_ptr()), None)

    for n in (1, 255, 1024, 1025):
        for shift in (0, 1):                                   # 16-byte aligned base, and offset by one element
            buf, view = _guarded((n, C_), torch.float32, SENT, shift=shift)
            abuf, aview = _guarded((n,), torch.int32, 77, shift=shift)
            assert call(n, view, aview) == 0, lib.smoe_last_error()
            ubuf, uview = _guarded((n, C_), torch.uint8, 201, shift=shift)
            assert call(n, uview, None, fmt=1) == 0, lib.smoe_last_error()
            torch.cuda.synchronize()
            got, gids = view.cpu().numpy(), aview.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), full[:n].view(np.uint32)), (n, shift)
            assert np.array_equal(gids, full_ids[:n]), (n, shift)
            assert np.array_equal(uview.cpu().numpy(), np.rint(got * 255).astype(np.uint8)), (n, shift)
            for b, fill, size in ((buf, SENT, n * C_), (abuf, 77, n), (ubuf, 201, n * C_)):
                flat = b.cpu().numpy()
                assert (flat[:64 + shift] == fill).all() and (flat[64 + shift + size:] == fill).all(), (n, shift)
    # lists = NULL equals all-ones lists, and differs from the sparse ones
    r1 = eng.sample(dp, eng.new_lists(), dpts)
    r0 = eng.sample(dp, None, dpts)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1) and not np.array_equal(r0.cpu().numpy(), full)
    # num_points == 0: a no-op that needs no pointers
    assert lib.smoe_shared_sample(eng._h, C.byref(cp), None, None, 0, None, 0, None, None) == 0
    assert tuple(eng.sample(dp, dl, dpts[:0]).shape) == (0, C_)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. a rotated point set against the restatement
# ---------------------------------------------------------------------------------------------------------------
ROTATED = [(IMAGES[1], (112, 168), {}), (IMAGES[2], (88, 112), {}), (IMAGES[3], (40, 56, 7), {}),
           (IMAGES[1], (112, 168), dict(train_inverse_cov=True))]


def _points_reference(image, kw, pts=None, u=None, bid=None):
    """the float32 / float64 restatement of a point set (or of coordinates and batch ids) and the loose set; asserts the
    conditions the inputs have to meet by themselves"""
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd, **kw)
    inside = None
    if pts is not None:
        inside, bid, u = point_mapping(pts, shape, bshape)
    ref = shared_points_reference(p, lists, u, bid, cfg, np.float32)
    ref64 = shared_points_reference(p, lists, u, bid, cfg, np.float64)
    frac = (np.clip(ref64["y"], 0, 1) * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    near_tau = (np.abs(ref64["w"] - TAU) < 1e-6).any(axis=1)[:, None]
    loose = np.broadcast_to(tie | near_tau, tie.shape)
    d32 = np.abs(ref["recon"] - ref64["recon"])[~loose]
    print(f"oracle: tie share {tie.mean():.2e}, loose share {loose.mean():.2e}, fp32 vs fp64 outside the loose set {d32.max():.2e}")
    assert loose.mean() < 0.01
    assert (d32 < 1e-7).all()
    return dict(p=p, K=K, lists=lists, ref=ref, ref64=ref64, loose=loose, inside=inside, bid=bid)


def _assert_point_parity(got, ids, R):
    dd = np.abs(got - R["ref"]["recon"].astype(np.float32))
    lo = R["loose"]
    print(f"kernel: max difference outside the loose set {dd[~lo].max():.3e}, overall {dd.max():.3e}, "
          f"values that differ {(dd > 1e-7).mean():.2e}")
    assert (dd[~lo] < 1e-7).all(), dd[~lo].max()
    assert (dd <= 1.0001 / 255).all(), dd.max()
    srt = np.sort(R["ref64"]["wt"], axis=1)
    shaky = ((srt[:, -1] - srt[:, -2]) < 1e-6) | (np.abs(R["ref64"]["w"] - TAU) < 1e-6).any(axis=1)
    assert ((ids == point_ids(R["ref"]["wt"])) | shaky).all()


@pytest.mark.parametrize("case", ROTATED, ids=[_name(c[0]) + ("-ic" if c[2] else "") for c in ROTATED])
def test_rotated_points_against_the_restatement(case):
    image, E, kw = case
    shape, bshape, C_, kpd = image
    pts = _rotated(bshape, _grid(shape, bshape), E, 22.5, 1.7)
    R = _points_reference(image, kw, pts=pts)
    assert 0.5 < R["inside"].mean() < 1.0                      # the view leaves the image at its corners
    eng = _engine(shape, bshape, C_, R["K"], **kw)
    out, ids = eng.sample(_dev(R["p"]), _dev_lists(R["lists"]), _pts(pts), want_argmax=True)
    torch.cuda.synchronize()
    out, ids = out.cpu().numpy(), ids.cpu().numpy()
    assert (out[~R["inside"]] == 0).all() and (ids[~R["inside"]] == -1).all()
    _assert_point_parity(out, ids, R)
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
    # the whole image at 1x is the render on the training lattice
    ax, ab, _ = _view_tables(shape, bshape, whole, shape)
    v1, i1 = eng.render_view(dp, dl, *_dev_view(ax, ab), want_argmax=True)
    r1, ri1 = eng.render(dp, dl, _dev_axes(_tables(shape, shape)), bshape, want_argmax=True)
    u8 = eng.render_view(dp, dl, *_dev_view(ax, ab), dtype=torch.uint8)
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(v1), _bits32(r1)) and torch.equal(i1, ri1)
    assert np.array_equal(u8.cpu().numpy(), np.rint(v1.cpu().numpy() * 255).astype(np.uint8))
    # an aligned 2x window is the crop of the 2x render, bit for bit
    n0, n1 = bshape
    win = [(float(n0), float(shape[0])), (float(n1 // 2 if n1 % 2 == 0 else n1), float(shape[1] - n1))]
    E = [int(2 * (hi - lo)) for lo, hi in win]
    ax, ab, _ = _view_tables(shape, bshape, win, E)
    v2, i2 = eng.render_view(dp, dl, *_dev_view(ax, ab), want_argmax=True)
    r2, ri2 = eng.render(dp, dl, _dev_axes(_tables(shape, [2 * s for s in shape])), [2 * b for b in bshape], want_argmax=True)
    torch.cuda.synchronize()
    crop = tuple(slice(int(2 * lo), int(2 * hi)) for lo, hi in win)
    assert np.array_equal(_bits32(v2), _bits32(r2[crop].contiguous())) and torch.equal(i2, ri2[crop])
    # a window that starts inside a batch, and a thumbnail with fewer samples than batches (its samples sit ON batch
    # boundaries): positions exact in float32 -- the same positions as points, bit for bit
    inner = [(1.25, 1.25 + (shape[0] - 3)), (bshape[1] + 0.75, bshape[1] + 0.75 + (shape[1] - bshape[1] - 2))]
    thumb_E = [max(1, g // 2) for g in _grid(shape, bshape)]
    for w, e in ((inner, [2 * (shape[0] - 3), 2 * (shape[1] - bshape[1] - 2)]), (whole, thumb_E)):
        ax, ab, xs = _view_tables(shape, bshape, w, e)
        pts = np.stack(np.meshgrid(*xs, indexing="ij"), axis=-1).reshape(-1, 2)
        assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
        v, vi = eng.render_view(dp, dl, *_dev_view(ax, ab), want_argmax=True)
        s, si = eng.sample(dp, dl, _pts(pts), want_argmax=True)
        torch.cuda.synchronize()
        _, bid, u = point_mapping(pts, shape, bshape)
        tab_bid = np.ravel_multi_index(tuple(np.meshgrid(*ab, indexing="ij")), _grid(shape, bshape)).reshape(-1)
        assert np.array_equal(bid, tab_bid)                    # the two host statements of ownership agree
        assert np.array_equal(_bits32(v).reshape(-1, C_), _bits32(s)) and np.array_equal(vi.cpu().numpy().reshape(-1), si.cpu().numpy())
    # a window whose positions are not exact in float32: the restatement on the view's own tables
    win = [(shape[0] / 7, shape[0] * 0.83), (shape[1] / 3, shape[1] * 0.9)]
    E = [37, 53]
    ax, ab, _ = _view_tables(shape, bshape, win, E)
    u = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)
    bid = np.ravel_multi_index(tuple(np.meshgrid(*ab, indexing="ij")), _grid(shape, bshape)).reshape(-1)
    R = _points_reference(image, {}, u=u, bid=bid)
    v, vi = eng.render_view(dp, dl, *_dev_view(ax, ab), want_argmax=True)
    torch.cuda.synchronize()
    _assert_point_parity(v.cpu().numpy().reshape(-1, C_), vi.cpu().numpy().reshape(-1), R)
    eng.close()


def test_one_frame_of_the_3d_model():
    shape, bshape, C_, kpd = IMAGES[3]
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    r, ri = eng.render(dp, dl, _dev_axes(_tables(shape, shape)), bshape, want_argmax=True)
    for t in (2, 5):                                           # a frame of the first and of the second batch on t
        win = [(0.0, float(shape[0])), (0.0, float(shape[1])), (float(t), float(t + 1))]
        ax, ab, _ = _view_tables(shape, bshape, win, [shape[0], shape[1], 1])
        v, vi = eng.render_view(dp, dl, *_dev_view(ax, ab), want_argmax=True)
        torch.cuda.synchronize()
        assert tuple(v.shape) == (shape[0], shape[1], 1, C_)
        assert np.array_equal(_bits32(v)[:, :, 0], _bits32(r[:, :, t].contiguous())) and torch.equal(vi[:, :, 0], ri[:, :, t])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the argument checks with a real handle
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_with_a_handle():
    """every refusal of the two entry points.  (The 160 KB LDS limit is the one a handle cannot reach: smoe_shared_create takes at
    most 8192 kernels, 54 KB here; the plan's limit is checked on the host, tests/host/shared_sample_args_driver.cpp.)"""
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
    buf, view = _guarded((64, C_), torch.float32, SENT)
    abuf, aview = _guarded((64,), torch.int32, 77)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def sample(h=eng._h, params=cp, pts=dpts, n=64, values=view, fmt=0):
        return lib.smoe_shared_sample(h, None if params is None else C.byref(params), vp(dl), vp(pts), n, vp(values), fmt,
                                      vp(aview), None)

    for kwargs, code, word in [(dict(h=C.c_void_p(None)), _lib.SMOE_ERR_INVALID, b"handle"),
                               (dict(params=None), _lib.SMOE_ERR_INVALID, b"p "), (dict(params=bad), _lib.SMOE_ERR_INVALID, b"p "),
                               (dict(pts=None), _lib.SMOE_ERR_INVALID, b"points"), (dict(values=None), _lib.SMOE_ERR_INVALID, b"values"),
                               (dict(n=-1), _lib.SMOE_ERR_INVALID, b"num_points"), (dict(fmt=7), _lib.SMOE_ERR_INVALID, b"image_format"),
                               (dict(n=1 << 41), _lib.SMOE_ERR_UNSUPPORTED, b"2^31")]:
        assert sample(**kwargs) == code, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_sample" in err and word in err, (kwargs, err)
    assert sample(n=0, pts=None, values=None) == 0             # a no-op
    ax, ab, _ = _view_tables(shape, bshape, [(0.0, 8.0), (0.0, 8.0)], (8, 8))
    dax, dab = _dev_view(ax, ab)
    vbuf, vview = _guarded((8, 8, C_), torch.float32, SENT)
    slots = lambda ts: (C.c_void_p * 3)(*([None if t is None else t.data_ptr() for t in ts] + [None] * (3 - len(ts))))
    ext3 = lambda e: (C.c_int32 * 3)(*(list(e) + [1] * (3 - len(e))))

    def render_view(h=eng._h, params=cp, ext=ext3((8, 8)), axes=slots(dax), batches=slots(dab), image=vview, fmt=0):
        return lib.smoe_shared_render_view(h, None if params is None else C.byref(params), vp(dl), ext, axes, batches, vp(image),
                                           fmt, None, None)

    for kwargs, code, word in [(dict(h=C.c_void_p(None)), _lib.SMOE_ERR_INVALID, b"handle"),
                               (dict(params=None), _lib.SMOE_ERR_INVALID, b"p "), (dict(ext=None), _lib.SMOE_ERR_INVALID, b"extent"),
                               (dict(axes=None), _lib.SMOE_ERR_INVALID, b"axis_coords"), (dict(batches=None), _lib.SMOE_ERR_INVALID, b"axis_batch"),
                               (dict(image=None), _lib.SMOE_ERR_INVALID, b"image"), (dict(fmt=7), _lib.SMOE_ERR_INVALID, b"image_format"),
                               (dict(ext=ext3((8, 0))), _lib.SMOE_ERR_INVALID, b"extent[1]"),
                               (dict(axes=slots([dax[0], None])), _lib.SMOE_ERR_INVALID, b"axis_coords[1]"),
                               (dict(batches=slots([None, dab[1]])), _lib.SMOE_ERR_INVALID, b"axis_batch[0]"),
                               (dict(ext=ext3((2 ** 31 - 1, 2 ** 31 - 1))), _lib.SMOE_ERR_UNSUPPORTED, b"2^31")]:
        assert render_view(**kwargs) == code, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_render_view" in err and word in err, (kwargs, err)
    eng10 = _engine(shape, bshape, C_, K, precision=10)
    assert sample(h=eng10._h, fmt=1) == _lib.SMOE_ERR_UNSUPPORTED and b"precision" in lib.smoe_last_error()
    assert render_view(h=eng10._h, fmt=1) == _lib.SMOE_ERR_UNSUPPORTED and b"precision" in lib.smoe_last_error()
    eng10.close()
    wide = _engine((16, (1 << 24) + 16), (16, 16), 1, 1)       # an axis the point decoder cannot resolve exactly in fp32
    wp = {k: torch.zeros_like(v[:1]) for k, v in dp.items()}
    wcp = wide._cparams(wp)
    assert sample(h=wide._h, params=wcp) == _lib.SMOE_ERR_UNSUPPORTED and b"2^24" in lib.smoe_last_error()
    wide.close()
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (abuf == 77).all() and (vbuf == SENT).all()         # nothing was written
    # the engine's own checks
    with pytest.raises(ValueError):
        eng.sample(dp, dl[:3], dpts)
    with pytest.raises(ValueError):
        eng.sample(dp, dl, dpts.cpu())
    with pytest.raises(ValueError):
        eng.render_view(dp, dl, dax, dab[:1])
    with pytest.raises(ValueError):
        eng.render_view(dp, dl, dax, [dab[0], dab[1][:4]])
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
    rec, rids = s.render(want_argmax=True)
    assert np.array_equal(rec.view(np.uint32), s.get_reconstruction().view(np.uint32))
    centres = _centres(shape).reshape(shape + (2,))
    out, ids = s.eval_points(centres, want_argmax=True)
    assert out.shape == rec.shape and np.array_equal(out.view(np.uint32), rec.view(np.uint32)) and np.array_equal(ids, rids)
    assert np.array_equal(s.eval_view(None).view(np.uint32), rec.view(np.uint32))
    big = s.render(scale=2)
    crop, cids = s.eval_view([(16, 48), (8, 88)], scale=2, want_argmax=True)
    assert crop.shape == (64, 160, 3) and np.array_equal(crop.view(np.uint32), big[32:96, 16:176].view(np.uint32))
    assert cids.dtype == np.int64 and (cids >= 0).mean() > 0.99
    t, tid = s.eval_points(centres, to_host=False, want_argmax=True)
    assert t.is_cuda and tid.is_cuda and tid.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), rec)
    tv = s.eval_view([(16, 48), (8, 88)], scale=2, to_host=False, dtype=np.uint8)
    assert tv.is_cuda and np.array_equal(tv.cpu().numpy(), np.rint(crop * 255).astype(np.uint8))
    ident = s.eval_warp([[1, 0, 0], [0, 1, 0]], shape)
    assert np.array_equal(ident.view(np.uint32), rec.view(np.uint32))
    free = s.eval_points(centres, use_lists=False)
    assert np.array_equal(free, s.render(use_lists=False))
