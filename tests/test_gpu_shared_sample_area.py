"""GPU tests of the area-averaged decoder of whole-image models (smoe_shared_sample_area through the C ABI): one tap against
smoe_shared_sample_grad / smoe_shared_sample, the fused call against the composition it replaces (smoe_shared_sample_grad at
``blocks.area_taps``' positions and the ordered float32 mean) bit for bit, pixel-centre boxes, parity with the float64
restatement, independence of the order of the points, kernel lists, centres outside, ragged counts with guard bytes, the
facade, and the argument checks with a real handle.

Parity criterion = tests/test_gpu_sample_area.py's.  The restatement (tests/shared_sample_area_engine.py) is evaluated in
float32 and float64; with ``e32 = max |mean32 - mean64|`` outside the loose set, the kernel must satisfy
``|mean_gpu - mean64| <= F_SA * e32`` there.  F_SA is twice the largest ratio measured on the MI355X over the 13 cases, rounded
up to a power of two (profiles/render/shared_sample_area_parity.txt has every case).  The loose share is a condition on the
inputs that the restatement alone has to meet first: < 0.03."""
import ctypes as C

import numpy as np
import pytest
import torch

from render_cases import _guarded
from sample_area_engine import masked_mean
from shared_sample_area_cases import CASES, CASE_IDS, area_reference, case, loose_of, rotated_footprint
from shared_sample_engine import point_mapping
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks
from test_gpu_shared_render import EMPTY, IMAGES, _dev, _dev_lists, _engine, _grid, _name, _setup
from test_gpu_shared_sample import _centres, _dev_view, _pts, _view_tables
from test_gpu_shared_sample_grad import _bits32, _lattice

pytestmark = pytest.mark.gpu

F_SA = 4.0                                          # largest ratio measured: 1.91 (48x64-c3-b16x32); doubled, up to a power of two
SENT = -7.0
TILE = 512                                          # SSA_TILE: taps per workgroup; P = TILE // prod(taps) points


def _area(eng, dp, dl, pts, F, taps, dtype=torch.float32):
    """the four planes of one call, on the host"""
    r = eng.sample_area(dp, dl, _pts(pts), F, taps, dtype=dtype, want_mean=True, want_count=True, want_batch=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in r]


def _composed(eng, dp, dl, pts, F, taps):
    """what the parent can do for the same result: smoe_shared_sample_grad's values at the materialised taps, the ordered
    float32 mean over the inside ones.  Returns (mean, count, the taps' batches [N, T])."""
    with np.errstate(invalid="ignore", over="ignore"):
        tp = blk.area_taps(np.asarray(pts, np.float32), F, taps)
    N, nt, d = tp.shape
    _, val, bk = eng.sample_grad(dp, dl, _pts(tp.reshape(-1, d)), want_values=True, want_batch=True)
    torch.cuda.synchronize()
    V, B = val.cpu().numpy().reshape(N, nt, -1), bk.cpu().numpy().reshape(N, nt)
    mean, cnt = masked_mean(V, B >= 0, np.float32)
    return mean, cnt, B


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# 1. one tap, arbitrary finite F
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_one_tap_is_the_point(i):
    c = case(i)
    d = len(c["shape"])
    eng = _engine(c["shape"], c["bshape"], c["C"], c["K"], c["mus_grid"], **c["kw"])
    dp, dl, dpts = _dev(c["p"]), _dev_lists(c["lists"]), _pts(c["pts"])
    F = np.random.default_rng(11 + i).normal(size=(d, d)) * 40
    val, mean, cnt, bk = _area(eng, dp, dl, c["pts"], F, 1)
    _, gv, gb = eng.sample_grad(dp, dl, dpts, want_values=True, want_batch=True)
    img, img8 = eng.sample(dp, dl, dpts), eng.sample(dp, dl, dpts, dtype=torch.uint8)
    torch.cuda.synchronize()
    assert _same(mean, gv.cpu().numpy()) and np.array_equal(bk, gb.cpu().numpy()) and np.array_equal(bk, c["bid"])
    assert cnt.dtype == np.uint8 and np.array_equal(cnt, c["inside"].astype(np.uint8)) and not c["inside"].all()
    assert _same(val, img.cpu().numpy()) and np.abs(val).max() > 0.1
    val8 = _area(eng, dp, dl, c["pts"], F, [1] * d, dtype=torch.uint8)[0]
    assert val8.dtype == np.uint8 and np.array_equal(val8, img8.cpu().numpy()) and val8.max() > 25
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. + 4. the fused call against the composition, bit for bit; against float64
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_fused_is_the_composition_and_parity_with_float64(i):
    c = case(i)
    ref, ref64 = area_reference(i)
    loose = loose_of(ref, ref64)                               # asserts the cap on the restatement alone
    F, taps = rotated_footprint(i)
    nt = int(np.prod(taps))
    eng = _engine(c["shape"], c["bshape"], c["C"], c["K"], c["mus_grid"], **c["kw"])
    dp, dl = _dev(c["p"]), _dev_lists(c["lists"])
    val, mean, cnt, bk = _area(eng, dp, dl, c["pts"], F, taps)
    cmean, ccnt, ctb = _composed(eng, dp, dl, c["pts"], F, taps)
    # 2. bit for bit the ordered float32 mean of smoe_shared_sample_grad's values at the taps; cells in several batches included
    assert _same(mean, cmean) and np.array_equal(cnt, ccnt) and np.array_equal(cnt, ref["count"])
    assert np.array_equal(ctb, ref["tap_batch"]) and np.array_equal(bk, ref["batch"])
    meets = np.array([len(np.unique(b[b >= 0])) for b in ctb])
    assert (meets > 1).mean() > 0.02 and meets.max() >= 2 and ((cnt > 0) & (cnt < nt)).any()
    assert ((bk < 0) & (cnt > 0)).any() and (mean[cnt == 0] == 0).all() and (val[cnt == 0] == 0).all()
    assert np.isfinite(mean).all() and _same(val, _lattice(mean))
    # 4. against float64, outside the loose set
    e32 = np.abs(ref["mean"].astype(np.float64) - ref64["mean"])[~loose].max()
    dm = np.abs(mean.astype(np.float64) - ref64["mean"]).max(axis=1)
    print(f"{CASE_IDS[i]}: e32 {e32:.2e}, kernel {dm[~loose].max():.2e}, ratio {dm[~loose].max() / e32:.2f}; loose share "
          f"{loose.mean():.2e}, on the loose set {dm[loose].max() if loose.any() else 0:.2e}; cells in more than one batch "
          f"{(meets > 1).mean():.3f} (up to {meets.max()}), with taps outside {((cnt > 0) & (cnt < nt)).mean():.3f}")
    assert (dm[~loose] <= F_SA * e32).all(), dm[~loose].max() / e32
    # outside ties and loose points the F32 image is the lattice of mean64
    levels = 2 ** c["cfg"].precision - 1
    frac = (np.clip(ref64["mean"], 0, 1) * levels + 0.5) % 1
    tie = (np.minimum(frac, 1 - frac) < 2e-4).any(axis=1)
    want = np.floor(np.clip(ref64["mean"], 0, 1) * levels + 0.5) / levels
    keep = ~tie & ~loose
    assert keep.mean() > 0.9 and np.abs(val.astype(np.float64) - want)[keep].max() < 1e-6
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. pixel-centre boxes
# ---------------------------------------------------------------------------------------------------------------
BOXES = [(IMAGES[0], 2), (IMAGES[0], 4), (IMAGES[4], 2), (IMAGES[4], 4), (IMAGES[3], 2)]


@pytest.mark.parametrize("image,s", BOXES, ids=[_name(b[0]) + f"-box{b[1]}" for b in BOXES])
def test_pixel_centre_boxes(image, s):
    """F = diag(s), taps = s at the centres s (i + 0.5): the taps are the pixel centres, exactly, and the mean is the ordered
    float32 sum of their values over the count.  The ragged 21 x 25 image with 7 x 5 batches gives cells that cross batch
    borders and cells with taps outside."""
    shape, bshape, C_, kpd = image
    d = len(shape)
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    E = [-(-n // s) for n in shape]
    cen = np.stack(np.meshgrid(*[s * (np.arange(e, dtype=np.float32) + 0.5) for e in E], indexing="ij"), axis=-1).reshape(-1, d)
    val, mean, cnt, bk = _area(eng, dp, dl, cen, np.diag([float(s)] * d), s)
    _, pv = eng.sample_grad(dp, dl, _pts(_centres(shape)), want_values=True)
    torch.cuda.synchronize()
    pv = pv.cpu().numpy().reshape(tuple(shape) + (C_,))
    # the pixels of every cell, row-major over the box (last axis fastest)
    cell = np.stack(np.meshgrid(*[np.arange(e) for e in E], indexing="ij"), axis=-1).reshape(-1, 1, d)
    off = np.stack(np.meshgrid(*[np.arange(s)] * d, indexing="ij"), axis=-1).reshape(1, -1, d)
    pix = cell * s + off
    inside = (pix < np.array(shape)).all(axis=-1)
    V = pv[tuple(np.minimum(pix[..., l], shape[l] - 1) for l in range(d))]
    want, wcnt = masked_mean(V, inside, np.float32)
    assert _same(mean, want) and np.array_equal(cnt, wcnt) and _same(val, _lattice(want)) and np.abs(mean).max() > 0.1
    _, pb, _ = point_mapping(pix.reshape(-1, d).astype(np.float32) + np.float32(0.5), shape, bshape)
    pb = pb.reshape(inside.shape)
    meets = np.array([len(np.unique(b[m])) for b, m in zip(pb, inside)])
    if image is IMAGES[4]:
        assert meets.max() == 2 ** d and (wcnt < s ** d).any() and (wcnt > 0).all()
    else:
        assert meets.max() == 1 and (wcnt == s ** d).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. a point owes nothing to the others
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [(3, 3), (8, 8)], ids=["T9", "T64"])
def test_a_point_owes_nothing_to_the_others(taps):
    shape, bshape, C_, kpd = IMAGES[1]
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    rng = np.random.default_rng(17)
    pts = (rng.uniform(-0.05, 1.05, size=(1500, 2)) * np.array(shape)).astype(np.float32)
    F = np.array([[5.0, -2.0], [2.0, 5.0]])
    perm = rng.permutation(pts.shape[0])
    base = _area(eng, dp, dl, pts, F, taps)
    assert base[2].max() == int(np.prod(taps)) and (base[2] < base[2].max()).any() and (base[3] < 0).any() and np.abs(base[1]).max() > 0.1
    # the first point dropped: every point moves to another lane and another workgroup boundary (P does not divide by T = 9)
    for sel in (perm, np.arange(1, pts.shape[0]), np.arange(0, pts.shape[0], 3), np.array([1234])):
        got = _area(eng, dp, dl, pts[sel], F, taps)
        for g, b in zip(got, base):
            assert g.dtype == b.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(b[sel]).view(np.uint8))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. lists
# ---------------------------------------------------------------------------------------------------------------
def test_no_lists_three_chunks_and_the_empty_batch():
    shape, bshape, C_, kpd = IMAGES[2]                         # K = 144: three staging chunks without lists
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    assert K == 144
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    rng = np.random.default_rng(29)
    pts = (rng.uniform(-0.03, 1.03, size=(700, 2)) * np.array(shape)).astype(np.float32)
    F = np.array([[3.0, 1.0], [-1.0, 3.0]])
    sparse = _area(eng, dp, dl, pts, F, (3, 2))
    ones = eng.sample_area(dp, eng.new_lists(), _pts(pts), F, (3, 2), want_mean=True, want_count=True, want_batch=True)
    none = eng.sample_area(dp, None, _pts(pts), F, (3, 2), want_mean=True, want_count=True, want_batch=True)
    torch.cuda.synchronize()
    for a, b in zip(ones, none):
        assert torch.equal(a, b)
    assert not _same(none[1].cpu().numpy(), sparse[1]) and np.array_equal(none[2].cpu().numpy(), sparse[2])
    cm, cc, _ = _composed(eng, dp, None, pts, F, (3, 2))
    assert _same(none[1].cpu().numpy(), cm) and np.array_equal(sparse[2], cc)
    # cells wholly in the batch with the empty list: mean 0, count = the taps inside the image
    g = np.unravel_index(EMPTY, _grid(shape, bshape))
    lo = np.array([g[0] * bshape[0], g[1] * bshape[1]], np.float32)
    assert lo[1] == 0
    cells = np.array([lo + np.array([8.0, 16.0], np.float32), lo + np.array([8.0, 1.0], np.float32)], np.float32)
    val, mean, cnt, bk = _area(eng, dp, dl, cells, np.diag([4.0, 4.0]), 4)
    assert (val == 0).all() and (mean == 0).all() and cnt.tolist() == [16, 12] and bk.tolist() == [EMPTY, EMPTY]
    free = _area(eng, dp, None, cells, np.diag([4.0, 4.0]), 4)
    assert (free[1] > 0).any() and free[2].tolist() == [16, 12]
    eng.close()


@pytest.mark.parametrize("image", [IMAGES[0], IMAGES[4]], ids=[_name(c) for c in (IMAGES[0], IMAGES[4])])
def test_every_tap_carries_the_list_of_its_own_batch(image):
    """disjoint lists in neighbouring batches (tests/test_gpu_shared_sample_grad.py) and cells centred on the batch corners
    g nb: the four taps of a cell lie in four batches with two disjoint lists"""
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, _, _ = _setup(shape, bshape, C_, kpd)
    p["pis"] = np.abs(p["pis"]) + np.float32(0.01)
    p["A_diagonal"] = np.ascontiguousarray(np.broadcast_to(np.eye(2, dtype=np.float32) * 1.5, p["A_diagonal"].shape))
    p["A_corr"] = np.zeros_like(p["A_corr"])
    grid = _grid(shape, bshape)
    colour = np.add.outer(np.arange(grid[0]), np.arange(grid[1])).reshape(-1) % 2
    lists = (np.arange(K)[None, :] % 2) == colour[:, None]
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    cen = np.stack(np.meshgrid(*[np.arange(1, g, dtype=np.float32) * n for g, n in zip(grid, bshape)], indexing="ij"),
                   axis=-1).reshape(-1, 2)
    F = np.diag([2.0, 2.0])
    val, mean, cnt, bk = _area(eng, dp, dl, cen, F, 2)
    cm, cc, tb = _composed(eng, dp, dl, cen, F, 2)
    assert (cnt == 4).all() and all(len(np.unique(b)) == 4 for b in tb) and np.array_equal(bk, tb[:, 3])   # the centre: the last tap's
    assert all(sorted(colour[b].tolist()) == [0, 0, 1, 1] for b in tb)
    assert _same(mean, cm) and np.array_equal(cnt, cc) and np.abs(mean).max() > 0.05
    # with one list for all four taps -- the centre's, or its neighbour's -- the mean is another
    for col in (0, 1):
        one = np.broadcast_to(lists[np.flatnonzero(colour == col)[0]], lists.shape)
        other = _area(eng, dp, _dev_lists(np.ascontiguousarray(one)), cen, F, 2)[1]
        assert (np.abs(other - mean).max(axis=1) > 1e-4).mean() > 0.5
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. centres outside
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [IMAGES[1], IMAGES[3]], ids=[_name(c) for c in (IMAGES[1], IMAGES[3])])
def test_centres_outside(image):
    shape, bshape, C_, kpd = image
    d = len(shape)
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    dp, dl = _dev(p), _dev_lists(lists)
    F, taps = np.diag([2.0] * d), 2
    far = np.full((3 * d, d), 3.0, np.float32)
    for l in range(d):
        far[3 * l, l], far[3 * l + 1, l], far[3 * l + 2, l] = np.nan, -1e6, shape[l] + 40.0
    far = np.concatenate([far, np.full((1, d), np.inf, np.float32), np.full((1, d), 3e38, np.float32)])
    val, mean, cnt, bk = _area(eng, dp, dl, far, F, taps)
    assert (val == 0).all() and (mean == 0).all() and (cnt == 0).all() and (bk == -1).all()
    # just outside on one axis: the taps at -0.75 are outside, those at 0.25 inside
    near = np.full((2 * d, d), 3.0, np.float32)
    for l in range(d):
        near[2 * l, l], near[2 * l + 1, l] = -0.25, shape[l] + 0.25
    val, mean, cnt, bk = _area(eng, dp, dl, near, F, taps)
    cm, cc, _ = _composed(eng, dp, dl, near, F, taps)
    assert (bk == -1).all() and (cnt == 2 ** (d - 1)).all() and np.array_equal(cnt, cc)
    assert _same(mean, cm) and (np.abs(mean).max(axis=1) > 0).any() and _same(val, _lattice(mean))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. bounds and alignment
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [(3, 3), (8, 8)], ids=["T9", "T64"])
def test_counts_and_guard_bytes(taps):
    from steered_mixture_of_experts_amd import _lib
    shape, bshape, C_, kpd = IMAGES[1]
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    lib = _lib.load()
    dp, dl = _dev(p), _dev_lists(lists)
    cp = eng._cparams(dp)
    rng = np.random.default_rng(23)
    allp = (rng.uniform(-0.04, 1.04, size=(3077, 2)) * np.array(shape)).astype(np.float32)
    dpts = _pts(allp)
    Fh = np.array([[4.0, -1.5], [1.5, 4.0]], np.float32)
    full = _area(eng, dp, dl, allp, Fh, taps)
    full8 = _area(eng, dp, dl, allp, Fh, taps, dtype=torch.uint8)[0]
    assert full[2].max() == int(np.prod(taps)) and (full[3] < 0).any() and full8.max() > 25
    Fc, tc = (C.c_float * 4)(*Fh.reshape(-1).tolist()), (C.c_int32 * 2)(*taps)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    P = TILE // int(np.prod(taps))
    assert TILE % int(np.prod(taps)) == (8 if taps == (3, 3) else 0)           # T = 9 does not divide the tile
    for n in (0, 1, P - 1, P, P + 1, 3077):
        for shift in (0, 1, 3):                                # 16-byte aligned bases, and offset by one / three elements
            for fmt, vdt, vfill, want in ((_lib.SMOE_IMAGE_F32, torch.float32, SENT, full[0]), (_lib.SMOE_IMAGE_U8, torch.uint8, 0x5A, full8)):
                vbuf, vview = _guarded((n, C_), vdt, vfill, shift=shift)
                mbuf, mview = _guarded((n, C_), torch.float32, SENT, shift=shift)
                cbuf, cview = _guarded((n,), torch.uint8, 0x5A, shift=shift)
                bbuf, bview = _guarded((n,), torch.int32, 77, shift=shift)
                rc = lib.smoe_shared_sample_area(eng._h, C.byref(cp), vp(dl), vp(dpts), n, Fc, tc, vp(vview), fmt, vp(mview),
                                                 vp(cview), vp(bview), None)
                assert rc == 0, lib.smoe_last_error()
                torch.cuda.synchronize()
                for view, w in ((vview, want), (mview, full[1]), (cview, full[2]), (bview, full[3])):
                    got = view.cpu().numpy()
                    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(w[:n]).view(np.uint8)), (n, shift, fmt)
                for b, fill, size in ((vbuf, vfill, n * C_), (mbuf, SENT, n * C_), (cbuf, 0x5A, n), (bbuf, 77, n)):
                    flat = b.cpu().numpy()
                    assert (flat[:64 + shift] == fill).all() and (flat[64 + shift + size:] == fill).all(), (n, shift, fmt)
    # single planes: the others are not touched, because they are not there
    n = P + 1
    mbuf, mview = _guarded((n, C_), torch.float32, SENT)
    assert lib.smoe_shared_sample_area(eng._h, C.byref(cp), vp(dl), vp(dpts), n, Fc, tc, None, 0, vp(mview), None, None, None) == 0
    vbuf, vview = _guarded((n, C_), torch.float32, SENT)
    assert lib.smoe_shared_sample_area(eng._h, C.byref(cp), vp(dl), vp(dpts), n, Fc, tc, vp(vview), 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert _same(mview.cpu().numpy(), full[1][:n]) and _same(vview.cpu().numpy(), full[0][:n])
    # num_points == 0: a no-op that needs no pointers
    assert lib.smoe_shared_sample_area(eng._h, C.byref(cp), None, None, 0, Fc, tc, None, 0, None, None, None, None) == 0
    assert tuple(eng.sample_area(dp, dl, dpts[:0], Fh, taps).shape) == (0, C_)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. the facade on the device
# ---------------------------------------------------------------------------------------------------------------
def test_facade_on_the_device():
    from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
    shape, bshape, C_ = (64, 96), (32, 32), 3
    b = synthetic_blocks(24, (16, 16), C_, 3)
    img = blk.blocks_to_image(b, shape, (16, 16))
    s = SharedSmoe(img, kernels_per_dim=[6, 8], train_inverse_cov=False, batch_size=list(bshape), use_determinant=True, use_yuv=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(0.01))
    s.train(6, val_iter=3, ukl_iter=3)
    eng, params, lists = s._engine, s._params, s._render_lists(False)

    def engine(pts, F, taps, **kw):
        r = eng.sample_area(params, lists, _pts(np.asarray(pts, np.float32).reshape(-1, 2)), F, list(taps), **kw)
        torch.cuda.synchronize()
        return r

    c, sn = np.cos(np.deg2rad(30)) / 0.3, np.sin(np.deg2rad(30)) / 0.3
    M = np.array([[c, -sn], [sn, c]])
    A = np.concatenate([M, (np.array([32.0, 48.0]) - M @ np.array([12.0, 16.0]))[:, None]], axis=1)
    pts = blk.warp_points(A, (24, 32))
    v, m, n = s.eval_points_area(pts, M, taps=(3, 3), want_mean=True, want_count=True)
    ev, em, en = engine(pts, M, (3, 3), want_mean=True, want_count=True)
    assert v.shape == (24, 32, C_) and _same(v.reshape(-1, C_), ev.cpu().numpy()) and _same(m.reshape(-1, C_), em.cpu().numpy())
    assert np.array_equal(n.reshape(-1), en.cpu().numpy()) and n.max() == 9 and n.min() < 9
    w = s.eval_warp(A, (24, 32), taps=3)
    assert _same(w, v) and not np.array_equal(w, s.eval_warp(A, (24, 32)))
    auto = s.eval_warp(A, (24, 32), taps="auto", to_host=False)
    assert auto.is_cuda and _same(auto.cpu().numpy().reshape(-1, C_), engine(pts, M, blk.footprint_taps(M)).cpu().numpy())
    # a 1/4 view: the lattice of the ordered 4 x 4 means of the values at the pixel centres
    E = (16, 24)
    view = s.eval_view(None, size=E, taps=(4, 4))
    cen = np.stack(np.meshgrid(blk.view_positions(0.0, 64.0, 16), blk.view_positions(0.0, 96.0, 24), indexing="ij"), axis=-1)
    assert _same(view.reshape(-1, C_), engine(cen, np.diag([4.0, 4.0]), (4, 4)).cpu().numpy())
    assert _same(view, s.eval_view(None, size=E, taps="auto")) and _same(view, s.eval_view(None, scale=0.25, taps=4))
    _, V = s.eval_points_grad(_centres(shape).reshape(shape + (2,)), want_values=True)
    box = V.reshape(16, 4, 24, 4, C_).swapaxes(1, 2).reshape(16 * 24, 16, C_)
    want, _ = masked_mean(box, np.ones(box.shape[:2], bool), np.float32)
    assert _same(view.reshape(-1, C_), _lattice(want))
    assert np.array_equal(s.eval_view(None, size=E, taps=4, dtype=np.uint8), np.rint(view * 255).astype(np.uint8))
    # taps=None and all ones: today's eval_view, bit for bit
    win = [(5.25, 30.5), (17.0, 49.75)]
    ax, ab, _ = _view_tables(shape, bshape, win, (19, 23))
    today = eng.render_view(params, lists, *_dev_view(ax, ab))
    torch.cuda.synchronize()
    for tp in (None, 1, (1, 1)):
        assert _same(s.eval_view(win, size=(19, 23), taps=tp), today.cpu().numpy())
    with pytest.raises(ValueError):
        s.eval_view(None, size=E, taps=4, want_argmax=True)


# ---------------------------------------------------------------------------------------------------------------
# 10. the argument checks with a real handle
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_with_a_handle():
    """every refusal of the entry point, and a correct call after each.  (The 160 KB LDS limit is the one a handle cannot
    reach: the plan's limit is checked on the host, tests/host/shared_sample_area_args_driver.cpp.)"""
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
    dpts = _pts(_centres(shape)[1000:1064] * 1.01)
    Fh = np.array([[3.0, -1.0], [1.0, 3.0]], np.float32)
    want = [_bits32(t) for t in eng.sample_area(dp, dl, dpts, Fh, (3, 2), want_mean=True)]
    vbuf, vview = _guarded((64, C_), torch.float32, SENT)
    mbuf, mview = _guarded((64, C_), torch.float32, SENT)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    farr = lambda a: (C.c_float * 4)(*[float(x) for x in np.asarray(a).reshape(-1)])
    tarr = lambda a: (C.c_int32 * 2)(*a)
    nanF, infF = Fh.copy(), Fh.copy()
    nanF[1, 0], infF[0, 1] = np.nan, np.inf

    def area(h=eng._h, params=cp, pts=dpts, n=64, F=farr(Fh), taps=tarr((3, 2)), values=vview, fmt=0, mean=mview):
        return lib.smoe_shared_sample_area(h, None if params is None else C.byref(params), vp(dl), vp(pts), n, F, taps,
                                           vp(values), fmt, vp(mean), None, None, None)

    INV, UNS = _lib.SMOE_ERR_INVALID, _lib.SMOE_ERR_UNSUPPORTED
    for kwargs, code, word in [(dict(h=C.c_void_p(None)), INV, b"handle"), (dict(params=None), INV, b"p "),
                               (dict(params=bad), INV, b"p "), (dict(pts=None), INV, b"points"),
                               (dict(F=None), INV, b"footprint"), (dict(taps=None), INV, b"taps"),
                               (dict(F=farr(nanF)), INV, b"footprint[1][0]"), (dict(F=farr(infF)), INV, b"footprint[0][1]"),
                               (dict(taps=tarr((0, 2))), INV, b"taps[0]"), (dict(taps=tarr((3, 17))), INV, b"taps[1]"),
                               (dict(taps=tarr((3, -1))), INV, b"taps[1]"), (dict(taps=tarr((9, 8))), INV, b"64"),
                               (dict(values=None, mean=None), INV, b"values or mean"), (dict(fmt=5), INV, b"image_format"),
                               (dict(n=-1), INV, b"num_points"), (dict(n=1 << 41), UNS, b"2^31")]:
        vbuf.fill_(SENT)
        mbuf.fill_(SENT)
        assert area(**kwargs) == code, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_sample_area" in err and word in err, (kwargs, err)
        torch.cuda.synchronize()
        assert (vbuf == SENT).all() and (mbuf == SENT).all()   # nothing was written
        assert area() == 0, lib.smoe_last_error()              # the call after a refused one succeeds
        torch.cuda.synchronize()
        assert np.array_equal(_bits32(vview), want[0]) and np.array_equal(_bits32(mview), want[1])
    assert area(n=0, pts=None, values=None, mean=None) == 0    # a no-op
    assert area(taps=tarr((16, 4))) == 0 and area(taps=tarr((1, 1))) == 0
    deep = _engine(shape, bshape, C_, K, precision=10)         # uint8 cannot hold a 10-bit lattice
    u8 = torch.empty((64, C_), dtype=torch.uint8, device="cuda")
    assert area(h=deep._h, values=u8, fmt=_lib.SMOE_IMAGE_U8) == UNS and b"precision" in lib.smoe_last_error()
    assert area(h=deep._h, values=None, fmt=_lib.SMOE_IMAGE_U8) == 0
    deep.close()
    wide = _engine((16, (1 << 24) + 16), (16, 16), 1, 1)       # an axis the point form cannot resolve exactly in fp32
    wp = {k: torch.zeros_like(v[:1]) for k, v in dp.items()}
    wcp = wide._cparams(wp)
    assert area(h=wide._h, params=wcp) == UNS and b"2^24" in lib.smoe_last_error()
    wide.close()
    torch.cuda.synchronize()
    # the engine's own checks
    with pytest.raises(ValueError):
        eng.sample_area(dp, dl[:3], dpts, Fh, (3, 2))
    with pytest.raises(ValueError):
        eng.sample_area(dp, dl, dpts.cpu(), Fh, (3, 2))
    with pytest.raises(ValueError):
        eng.sample_area(dp, dl, dpts, Fh, (3, 2), out=torch.empty((64, C_ + 1), device="cuda"))
    with pytest.raises(ValueError):
        eng.sample_area(dp, dl, dpts, Fh, (3, 2), dtype=torch.float64)
    for kw in (dict(footprint=Fh[:1]), dict(footprint=nanF), dict(taps=(3, 2, 2)), dict(taps=17), dict(taps=(9, 8))):
        args = dict(footprint=Fh, taps=(3, 2))
        args.update(kw)
        with pytest.raises(ValueError, match="sample_area"):
            eng.sample_area(dp, dl, dpts, **args)
    eng.close()
