"""GPU tests of the area-averaged point decoder (smoe_sample_area through the C ABI and the facade): one tap against
smoe_sample_grad, taps on pixel centres against the sum of smoe_sample_grad's values in the stated order, rotated footprints
against the float64 restatement (tests/sample_area_engine.py), independence of a point from the list it comes in and from the
path its workgroup takes, centres outside the image, guarded buffers, and the facade.

Parity criterion of the rotated footprints.  The restatement is evaluated in float32 and float64; with ``e32 = max |mean32 -
mean64|`` outside the loose set, the kernel must satisfy ``|mean_gpu - mean64| <= F_A * e32`` there.  The hardware exp2 /
reciprocal are 1-ulp approximations where numpy rounds correctly and the kernel's fused multiply-adds associate differently, so
the kernel may sit a few times farther from float64 than numpy's float32 does.  F_A is twice the largest ratio measured on the
MI355X, rounded up to a power of two: 2.25 on the 16x16 C 3 blocks with blend 2 (0.91 ... 1.29 elsewhere), so F_A = 8
(profiles/render/sample_area_parity.txt lists the ratios per case).  Condition on the inputs, asserted on the restatement alone
before the GPU is compared: the loose share of the covered points is at most 0.03 (a point is loose if any of its taps is, in
either precision).  Loose points must be finite; counts and blocks are exact everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from render_cases import _guarded, _image
from sample_area_cases import LOOSE_CAP, area_reference, loose_of, rotated_footprint
from sample_grad_cases import CASES, CASE_IDS, case_inputs
from steered_mixture_of_experts_amd import blocks as blk
from test_gpu_render_view import _open
from test_gpu_sample import _dev, _rotated

pytestmark = pytest.mark.gpu

F_A = 8.0


def _area(eng, dp, act, grid, length, pts, F, taps, **kw):
    """lattice values, mean, count, block of the cell centres (host array or device tensor)"""
    return eng.sample_area(dp, act, grid, length, pts if torch.is_tensor(pts) else _dev(pts), F, taps, want_mean=True,
                           want_count=True, want_block=True, **kw)


def _lattice(mean):
    """the rounding of the point decoders on a float32 array: floor(fma(v, inv_scale, 0.5)) and that times scale.  The product
    of two float32 is exact in float64 and so is the sum with 0.5 at these magnitudes: one rounding to float32, as the fma's."""
    scale = np.float32(1) / np.float32(255)
    inv = np.float32(1) / scale
    kq = np.floor((mean.astype(np.float64) * np.float64(inv) + 0.5).astype(np.float32))
    return (kq * scale).astype(np.float32), kq.astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# 1. one tap: the point itself
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_one_tap_is_the_point_of_sample_grad(i, blended):
    c = case_inputs(i, blended)
    shape, d = c["shape"], len(c["shape"])
    F, _ = rotated_footprint(i)                                                # arbitrary and finite: one tap has offset 0
    eng, dp, act, grid, _ = _open(tuple(shape), c["C"], c["kpd"], c["opt"])
    pts = _dev(c["pts"])
    _, val, bk = eng.sample_grad(dp, act, grid, c["length"], pts, blend=c["beta"], want_values=True, want_block=True)
    img, mean, cnt, blk_ = _area(eng, dp, act, grid, c["length"], pts, F, [1] * d, blend=c["beta"])
    u8 = eng.sample_area(dp, act, grid, c["length"], pts, F, [1] * d, blend=c["beta"], dtype=torch.uint8)
    torch.cuda.synchronize()
    val, bk, img, mean, cnt, blk_, u8 = (t.cpu().numpy() for t in (val, bk, img, mean, cnt, blk_, u8))
    assert mean.shape == (len(c["pts"]), c["C"]) and val.any()
    assert np.array_equal(_bits(mean), _bits(val)) and np.array_equal(blk_, bk)
    assert (bk < 0).sum() == c["n_out"] and np.array_equal(cnt, (bk >= 0).astype(np.uint8))
    q, kq = _lattice(mean)
    assert img.dtype == np.float32 and u8.dtype == np.uint8
    assert np.array_equal(_bits(img), _bits(q)) and np.array_equal(u8, kq)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. taps on pixel centres: the sum of smoe_sample_grad's values in the stated order
# ---------------------------------------------------------------------------------------------------------------
def _box_cells(shape, grid, s):
    """the centres s (i + 0.5) of the cells of s pixels that cover the blocks' footprint, [N, d] float32, and the cells per axis"""
    E = [-(-g * n // s) for g, n in zip(grid, shape)]
    idx = np.stack(np.meshgrid(*[np.arange(e) for e in E], indexing="ij"), axis=-1).reshape(-1, len(shape))
    return (s * (idx + 0.5)).astype(np.float32), E


def _ragged(shape, grid):
    """the blocks' footprint minus 3 on each spatial axis"""
    return [g * n - (3 if l < 2 else 0) for l, (g, n) in enumerate(zip(grid, shape))]


@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_taps_on_pixel_centres_are_the_ordered_sum_of_sample_grad(i, blended):
    c = case_inputs(i, blended)
    shape, d = c["shape"], len(c["shape"])
    eng, dp, act, grid, _ = _open(tuple(shape), c["C"], c["kpd"], c["opt"])
    length = _ragged(shape, grid)
    for s in ((2,) if d == 3 else (2, 4)):
        pts, E = _box_cells(shape, grid, s)
        F, taps = np.diag([float(s)] * d), [s] * d
        tp = blk.area_taps(pts, F, taps)                                       # the pixel centres, exactly (tests/test_sample_area_cpu.py)
        assert np.array_equal(tp * 2, np.round(tp * 2)) and (np.round(tp * 2) % 2 == 1).all()
        nt = tp.shape[1]
        _, val, bk = eng.sample_grad(dp, act, grid, length, _dev(tp.reshape(-1, d)), blend=c["beta"], want_values=True, want_block=True)
        val, inside = val.reshape(len(pts), nt, c["C"]), (bk >= 0).reshape(len(pts), nt)
        acc = torch.zeros((len(pts), c["C"]), dtype=torch.float32, device="cuda")
        for t in range(nt):                                                    # the stated order: one fp32 add per inside tap
            acc = torch.where(inside[:, t, None], acc + val[:, t], acc)
        n_in = inside.sum(dim=1)
        want = torch.where(n_in[:, None] > 0, acc / n_in.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(acc))
        img, mean, cnt, _ = _area(eng, dp, act, grid, length, pts, F, taps, blend=c["beta"])
        torch.cuda.synchronize()
        # the number of pixel centres of the cell inside the ragged image, from integers
        per_axis = [np.clip(length[l] - s * np.arange(E[l]), 0, s) for l in range(d)]
        n_want = np.prod(np.stack(np.meshgrid(*per_axis, indexing="ij"), axis=-1).reshape(-1, d), axis=1)
        assert np.array_equal(cnt.cpu().numpy(), n_want.astype(np.uint8)) and np.array_equal(n_in.cpu().numpy(), n_want)
        assert (s != 2 or (n_want == 0).any()) and ((n_want > 0) & (n_want < nt)).any() and (n_want == nt).any()
        assert torch.equal(mean.view(torch.int32), want.view(torch.int32)), (s, (mean - want).abs().max().item())
        assert mean.abs().max() > 0.05 and np.array_equal(_bits(img.cpu().numpy()), _bits(_lattice(mean.cpu().numpy())[0]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. rotated footprints against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------
def rotated_conditions(ref, ref64):
    """The condition on the inputs, asserted on the restatement alone: the counts of the two precisions agree, the loose share
    of the covered points is at most LOOSE_CAP, no uncovered point is loose, and numpy's float32 differs from float64 on the
    tight points.  Returns (covered, loose, tight, e32)."""
    covered = ref64["count"] > 0
    loose = loose_of(ref, ref64)
    assert np.array_equal(ref["count"], ref64["count"]) and loose[covered].mean() <= LOOSE_CAP and not loose[~covered].any()
    tight = covered & ~loose
    e32 = np.abs(ref["mean"].astype(np.float64) - ref64["mean"])[tight].max()
    assert e32 > 0
    return covered, loose, tight, e32


def judge_rotated(label, taps, ref64, covered, loose, tight, e32, img, mean, cnt, bk):
    """the criterion of the module's docstring on the kernel's lattice image, mean, count and block ids (host arrays)"""
    dm = np.abs(mean - ref64["mean"])
    print(f"{label}: taps {'x'.join(map(str, taps))}, covered {covered.sum()} of {covered.size}, "
          f"partially {(covered & (ref64['count'] < ref64['inside'].shape[1])).sum()}, loose share of the covered {loose[covered].mean():.2e}, "
          f"near the floor of the normaliser {ref64['floor'].mean():.2e}; mean: e32 {e32:.2e}, kernel {dm[tight].max():.2e}, "
          f"ratio {dm[tight].max() / e32:.2f}; on the loose set {dm[loose].max() if loose.any() else 0:.2e}")
    assert np.isfinite(mean).all() and np.isfinite(img).all()
    assert np.array_equal(cnt, ref64["count"].astype(np.uint8)) and np.array_equal(bk, ref64["block"])
    assert (dm[tight] <= F_A * e32).all(), dm[tight].max() / e32
    assert (mean[~covered] == 0).all() and (img[~covered] == 0).all()
    # the image is the lattice of the float64 mean except at rounding ties
    frac = (ref64["mean"] * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    want = np.floor(ref64["mean"] * 255 + 0.5) / 255
    ok = ~tie & ~loose[:, None]
    assert (np.abs(img - want)[ok] < 1e-7).all(), np.abs(img - want)[ok].max()
    assert (np.abs(img - want) <= 1.0001 / 255)[~loose].all()


@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_rotated_footprints_against_the_restatement(i, blended):
    c = case_inputs(i, blended)
    ref, ref64 = area_reference(i, blended)
    F, taps = rotated_footprint(i)
    covered, loose, tight, e32 = rotated_conditions(ref, ref64)
    eng, dp, act, grid, _ = _open(tuple(c["shape"]), c["C"], c["kpd"], c["opt"])
    img, mean, cnt, bk = (t.cpu().numpy() for t in _area(eng, dp, act, grid, c["length"], c["pts"], F, taps, blend=c["beta"]))
    judge_rotated(f"{CASE_IDS[i]}-{'blend' if blended else 'plain'}", taps, ref64, covered, loose, tight, e32, img, mean, cnt, bk)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. independence: a point's result does not depend on the list it comes in, nor on the path its workgroup takes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_a_point_owes_nothing_to_the_other_points_or_to_the_path(beta, monkeypatch):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    monkeypatch.delenv("SMOE_SAMPLE_RECORDS", raising=False)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    assert int(np.prod(grid)) == 12
    length = [g * n for g, n in zip(grid, shape)]
    pts = _rotated(shape, grid, (61, 83), 17.0, 1.7)
    F, taps = rotated_footprint(0)
    inside, g, _u = blk.point_blocks(pts, shape, grid, length)
    own = np.ravel_multi_index(tuple(g.T), grid)
    assert inside.all() and len(np.unique(own)) == 12
    # sorted by block: the staged path -- the record budget of this triple holds all 12 blocks
    order = np.argsort(own, kind="stable")
    base = [t.cpu().numpy() for t in _area(eng, dp, act, grid, length, pts[order], F, taps, blend=beta)]
    assert base[1].shape == (len(pts), C_) and (base[3] == own[order]).all() and base[1].any() and base[2].max() == 6 and base[2].min() < 6

    def same(res, index, what):
        for a, b in zip(res, base):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b[index])), what

    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    same(_area(eng, dp, act, grid, length, pts, F, taps, blend=beta), inv, "row-major order")
    perm = np.random.default_rng(11).permutation(len(pts))
    same(_area(eng, dp, act, grid, length, pts[perm], F, taps, blend=beta), inv[perm], "a random permutation")
    same(_area(eng, dp, act, grid, length, pts[::3], F, taps, blend=beta), inv[::3], "every third point")
    same(_area(eng, dp, act, grid, length, pts[17:18], F, taps, blend=beta), inv[17:18], "one point")
    # the direct path by construction: 4 records never hold the box of 256 shuffled points, and 0 never stages
    for lo in range(0, len(perm), 256):
        gg = g[perm[lo:lo + 256]]
        assert np.prod(gg.max(axis=0) - gg.min(axis=0) + 1) > 4
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "4")
    same(_area(eng, dp, act, grid, length, pts[perm], F, taps, blend=beta), inv[perm], "shuffled, at most 4 records staged")
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "0")
    same(_area(eng, dp, act, grid, length, pts[order], F, taps, blend=beta), np.arange(len(order)), "sorted, nothing staged")
    same(_area(eng, dp, act, grid, length, pts, F, taps, blend=beta), inv, "row-major, nothing staged")
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. outside
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_centres_outside_the_image(beta):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    length = [g * n - 3 for g, n in zip(grid, shape)]                           # 45 x 61
    F, taps = np.diag([4.0, 4.0]), (4, 4)
    nan = float("nan")
    pts = np.array([[nan, 10.0], [10.0, nan], [nan, nan], [-1000.0, 10.0], [10.0, 1e30], [float("inf"), 3.0],
                    [-1.0, 30.0], [30.0, -1.0], [46.0, 30.0], [22.0, 62.0], [-1.5, -1.5], [22.0, 30.0]], np.float32)
    img, mean, cnt, bk = (t.cpu().numpy() for t in _area(eng, dp, act, grid, length, pts, F, taps, blend=beta))
    far = slice(0, 6)                                                          # NaN or no tap inside: 0 / 0 / count 0 / block -1
    assert (img[far] == 0).all() and (mean[far] == 0).all() and (cnt[far] == 0).all() and (bk[far] == -1).all()
    # a centre just outside with taps inside: their mean, block -1
    tp = blk.area_taps(pts, F, taps)
    inside = blk.point_blocks(tp, shape, grid, length)[0]
    assert list(inside.sum(axis=1)[6:]) == [4, 4, 4, 4, 1, 16] and np.array_equal(cnt, inside.sum(axis=1).astype(np.uint8))
    assert (bk[6:11] == -1).all() and bk[11] == 1 * grid[1] + 1
    _, val, vb = eng.sample_grad(dp, act, grid, length, _dev(tp.reshape(-1, 2)), blend=beta, want_values=True, want_block=True)
    val, vin = val.reshape(len(pts), 16, C_), (vb >= 0).reshape(len(pts), 16)
    assert np.array_equal(vin.cpu().numpy(), inside)
    acc = torch.zeros((len(pts), C_), dtype=torch.float32, device="cuda")
    for t in range(16):
        acc = torch.where(vin[:, t, None], acc + val[:, t], acc)
    want = (acc[6:] / vin[6:].sum(dim=1).to(torch.float32)[:, None]).cpu().numpy()
    assert np.array_equal(_bits(mean[6:]), _bits(want)) and (mean[6:].max(axis=1) > 0).all()
    assert np.array_equal(_bits(img), _bits(_lattice(mean)[0]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. guarded buffers
# ---------------------------------------------------------------------------------------------------------------
SENT = -7.0


@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_bounds_and_alignment(beta):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    length = [g * n for g, n in zip(grid, shape)]
    allpts = _rotated(shape, grid, (61, 83), -31.0, 0.8)                       # some of them outside
    assert not blk.point_blocks(allpts, shape, grid, length)[0].all()
    F, taps = rotated_footprint(0)
    lib, cp = eng.lib, eng._cparams(dp)
    g3, l3 = (C.c_int32 * 3)(*(list(grid) + [1])), (C.c_int32 * 3)(*(list(length) + [1]))
    cF, ct = (C.c_float * 4)(*[float(v) for v in F.reshape(-1)]), (C.c_int32 * 2)(*taps)
    bl = None if beta is None else (C.c_float * 3)(float(beta), float(beta), 0.0)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points, n, values, fmt, mean, count, block):
        return lib.smoe_sample_area(eng._h, C.byref(cp), C.c_void_p(act.data_ptr()), g3, l3, ptr(points), n, cF, ct, bl,
                                    ptr(values), fmt, ptr(mean), ptr(count), ptr(block), None)

    from steered_mixture_of_experts_amd import _lib
    for N in (0, 1, 255, 257, 3 * 1024 + 5):
        pts = _dev(allpts[:N])
        if N:
            base = _area(eng, dp, act, grid, length, pts, F, taps, blend=beta)
            base_u8 = eng.sample_area(dp, act, grid, length, pts, F, taps, blend=beta, dtype=torch.uint8)
        for shift in (0, 1, 3):
            vbuf, vview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            ubuf, uview = _guarded((N, C_), torch.uint8, 201, shift=shift)
            mbuf, mview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            cbuf, cview = _guarded((N,), torch.uint8, 199, shift=shift)
            bbuf, bview = _guarded((N,), torch.int32, -9, shift=shift)
            monly, monly_view = _guarded((N, C_), torch.float32, SENT, shift=shift)
            assert call(pts, N, vview, _lib.SMOE_IMAGE_F32, mview, cview, bview) == 0, lib.smoe_last_error()
            assert call(pts, N, uview, _lib.SMOE_IMAGE_U8, None, None, None) == 0, lib.smoe_last_error()    # the extras are optional
            assert call(pts, N, None, _lib.SMOE_IMAGE_F32, monly_view, None, None) == 0 or N == 0, lib.smoe_last_error()   # and so is values
            torch.cuda.synchronize()
            for b_, fill, n in [(vbuf, SENT, N * C_), (ubuf, 201, N * C_), (mbuf, SENT, N * C_), (cbuf, 199, N), (bbuf, -9, N),
                                (monly, SENT, N * C_)]:
                flat = b_.cpu().numpy()
                assert (flat[:64 + shift] == fill).all() and (flat[64 + shift + n:] == fill).all(), (N, shift)   # nothing outside
            if N:
                assert torch.equal(vview.view(torch.int32), base[0].view(torch.int32)) and torch.equal(uview, base_u8)
                assert torch.equal(mview.view(torch.int32), base[1].view(torch.int32)) and torch.equal(monly_view.view(torch.int32), base[1].view(torch.int32))
                assert torch.equal(cview, base[2]) and torch.equal(bview, base[3])
                assert (bview != -9).all() and (mview != SENT).all() and (vview != SENT).all() and (cview <= 6).all()
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
    params, active, center = s._whole_model(False)
    c, sn = 3 * np.cos(np.deg2rad(17)), 3 * np.sin(np.deg2rad(17))
    M = np.array([[c, -sn], [sn, c]])
    A = np.concatenate([M, (np.array([20.0, 28.0]) - M @ np.array([7.0, 9.0]))[:, None]], axis=1)
    pts = blk.warp_points(A, (14, 18))
    dpts = torch.from_numpy(pts).cuda()
    v, mean, cnt = s.sample_area(dpts, M, taps=(3, 3), blend=2, to_host=False, want_mean=True, want_count=True)
    assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (14, 18, 3) and tuple(mean.shape) == (14, 18, 3)
    assert cnt.dtype == torch.uint8 and tuple(cnt.shape) == (14, 18) and cnt.max() == 9 and cnt.min() < 9 and v.max() > 0.05
    # the engine call behind it
    ev, em, ec = s._engine.sample_area(params, active, s.grid, [40, 56], dpts.reshape(-1, 2), M, (3, 3), blend=[2.0, 2.0],
                                       want_mean=True, want_count=True, center_grid=center)
    assert torch.equal(v.reshape(-1, 3), ev) and torch.equal(mean.reshape(-1, 3).view(torch.int32), em.view(torch.int32)) and torch.equal(cnt.reshape(-1), ec)
    assert np.array_equal(s.sample_area(pts, M, blend=2), v.cpu().numpy())                    # host in, host out; auto = 3 x 3
    assert torch.equal(s.render_warp(A, (14, 18), taps=(3, 3), blend=2, to_host=False), v)
    assert torch.equal(s.render_warp(A, (14, 18), taps="auto", blend=2, to_host=False), v)
    assert torch.equal(s.render_warp(A, (14, 18), taps=1, blend=2, to_host=False), s.sample(dpts, blend=2, to_host=False))
    assert not torch.equal(s.render_warp(A, (14, 18), blend=2, to_host=False), v)
    u8 = s.sample_area(dpts, M, taps=(3, 3), blend=2, dtype=np.uint8, to_host=False)
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.round(v * 255).to(torch.uint8))
    # a 1/4 view of the ragged image: the lattice of the 4 x 4 means of the pixel centres
    view = s.render_view(None, size=(10, 14), taps=(4, 4), to_host=False)
    centres = np.stack(np.meshgrid(4 * (np.arange(10) + 0.5), 4 * (np.arange(14) + 0.5), indexing="ij"), axis=-1).astype(np.float32)
    tp = blk.area_taps(centres.reshape(-1, 2), np.diag([4.0, 4.0]), (4, 4))
    _, val = s._engine.sample_grad(params, active, s.grid, [40, 56], _dev(tp.reshape(-1, 2)), want_values=True, center_grid=center)
    val = val.reshape(140, 16, 3)
    acc = torch.zeros((140, 3), dtype=torch.float32, device="cuda")
    for t in range(16):
        acc = acc + val[:, t]
    want = _lattice((acc / 16.0).cpu().numpy())[0]
    assert tuple(view.shape) == (10, 14, 3) and np.array_equal(_bits(view.cpu().numpy().reshape(-1, 3)), _bits(want))
    ev = s._engine.sample_area(params, active, s.grid, [40, 56], _dev(centres.reshape(-1, 2)), np.diag([4.0, 4.0]), (4, 4), center_grid=center)
    assert torch.equal(view.reshape(-1, 3), ev)
    assert torch.equal(s.render_view(None, size=(10, 14), taps=(1, 1), to_host=False), s.render_view(None, size=(10, 14), to_host=False))
    assert not torch.equal(s.render_view(None, size=(10, 14), to_host=False), view)
    with pytest.raises(ValueError):
        s.sample_area(pts, M, taps=(9, 8))
