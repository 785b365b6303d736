"""GPU tests of the area-averaged decoder of whole-image models with per-point footprints (smoe_shared_sample_area_each through
the C ABI and the facade).  The specification is one sentence -- the result for a point is bit for bit that of
smoe_shared_sample_area called with that one point, its footprint and its taps -- and every comparison here is bitwise, so
there is no tolerance: broadcast footprints against smoe_shared_sample_area, three configurations mixed within every
wavefront, tap counts that do not divide a round, the tilt of every case (tests/shared_sample_area_each_cases.py) against the
composition on materialised taps (``blocks.area_taps_each``, smoe_shared_sample_grad's values and batches, the ordered fp32 sum
over the inside taps, one division), independence of a point from the list it comes in, kernel lists, void points, guarded and
unaligned buffers, every refusal of the entry point, and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

import sample_area_each_cases as block_each
from render_cases import _guarded
from sample_area_each_cases import each_of
from shared_sample_area_cases import rotated_footprint
from shared_sample_area_each_cases import CASES, CASE_IDS, SSE_POINTS, SSE_TILE, model, tilt_inputs
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks
from test_gpu_shared_render import EMPTY, IMAGES, _dev, _dev_lists, _engine, _grid, _name, _setup
from test_gpu_shared_sample import _centres, _pts

pytestmark = pytest.mark.gpu

SENT = -7.0
WANT = dict(want_mean=True, want_count=True, want_batch=True)


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _dv(a, conv):
    return a if torch.is_tensor(a) else conv(a)


def _each(eng, dp, dl, pts, foot, taps, dtype=torch.float32):
    """lattice values, mean, count, batch (host arrays or device tensors in, device tensors out)"""
    return eng.sample_area_each(dp, dl, _dv(pts, _pts), _dv(foot, _pts), _dv(taps, _u8), dtype=dtype, **WANT)


def _area(eng, dp, dl, pts, F, taps, dtype=torch.float32):
    return eng.sample_area(dp, dl, _dv(pts, _pts), F, list(taps), dtype=dtype, **WANT)


def _same(got, want, what=""):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a if a.dtype == torch.uint8 else a.view(torch.int32), b if b.dtype == torch.uint8 else b.view(torch.int32)), what


def _open(i):
    c = model(i)
    eng = _engine(c["shape"], c["bshape"], c["C"], c["K"], c["mus_grid"], **c["kw"])
    return c, eng, _dev(c["p"]), _dev_lists(c["lists"])


def _mixed(i, N):
    """point k takes configuration k % 3 of sample_area_each_cases.mixed_configs (of a block case with as many axes)"""
    d = len(CASES[i][0][0])
    j = next(j for j, bc in enumerate(block_each.CASES) if len(bc[0]) == d)
    cfgs = block_each.mixed_configs(j)
    foot = np.stack([cfgs[k % 3][0] for k in range(N)]).astype(np.float32)
    taps = np.array([cfgs[k % 3][1] for k in range(N)], np.uint8)
    return cfgs, foot, taps


def _lattice_k(mean):
    """the lattice index of float32 means in the kernel's arithmetic (precision 8), clamped to the index of the clip's end"""
    scale = np.float32(1) / np.float32(255)
    inv = np.float32(1) / scale
    return np.minimum(np.floor((mean.astype(np.float64) * np.float64(inv) + 0.5).astype(np.float32)), np.float32(255)), scale


def _composed(eng, dp, dl, t, Cn):
    """what the parent can do for the same result: every slot of every point through smoe_shared_sample_grad (a slot that holds
    no tap is NaN, hence outside), the ordered fp32 sum over the inside taps, one division.  (mean, count) on the device."""
    N, d = t["pts"].shape
    _, val, bk = eng.sample_grad(dp, dl, _pts(t["tp"].reshape(-1, d)), want_values=True, want_batch=True)
    val, tb = val.reshape(N, blk.AREA_TAPS, Cn), bk.reshape(N, blk.AREA_TAPS)
    assert np.array_equal(tb.cpu().numpy(), t["tap_batch"])
    inside = tb >= 0
    acc = torch.zeros((N, Cn), dtype=torch.float32, device="cuda")
    for s in range(blk.AREA_TAPS):                                             # the stated order: one fp32 add per inside tap
        acc = torch.where(inside[:, s, None], acc + val[:, s], acc)
    n_in = inside.sum(dim=1)
    mean = torch.where(n_in[:, None] > 0, acc / n_in.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(acc))
    return mean, n_in


# ---------------------------------------------------------------------------------------------------------------
# 1. broadcast: a constant footprint and constant taps are smoe_shared_sample_area
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_broadcast_footprints_are_shared_sample_area(i):
    c, eng, dp, dl = _open(i)
    F, taps = rotated_footprint(i)
    pts = _pts(c["pts"])
    Fe, te = each_of(len(c["pts"]), F, taps)
    want, got = _area(eng, dp, dl, pts, F, taps), _each(eng, dp, dl, pts, Fe, te)
    want8, got8 = _area(eng, dp, dl, pts, F, taps, torch.uint8), _each(eng, dp, dl, pts, Fe, te, torch.uint8)
    torch.cuda.synchronize()
    assert want[1].abs().max() > 0.05 and want[2].max() == int(np.prod(taps)) and got8[0].dtype == torch.uint8 and want8[0].max() > 25
    assert ((want[3] < 0) & (want[2] > 0)).any()
    _same(got, want)
    _same(got8, want8)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. three configurations mixed within every wavefront
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_mixed_configurations_within_a_wavefront(i):
    c, eng, dp, dl = _open(i)
    cfgs, foot, taps = _mixed(i, len(c["pts"]))
    got = _each(eng, dp, dl, c["pts"], foot, taps)
    for r, (F, tp) in enumerate(cfgs):
        want = _area(eng, dp, dl, np.ascontiguousarray(c["pts"][r::3]), F, tp)
        torch.cuda.synchronize()
        _same([g[r::3].contiguous() for g in got], want, f"configuration {r}")
        assert want[2].max() == int(np.prod(tp))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. tap counts that do not divide a round: a point's taps straddle rounds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,taps", [(1, (5, 3)), (1, (10, 6)), (3, (3, 3, 7)), (1, (8, 8))], ids=["T15", "T60", "T63", "T64"])
def test_round_boundaries(i, taps):
    c, eng, dp, dl = _open(i)
    d, T = len(c["shape"]), int(np.prod(taps))
    TILE = SSE_TILE[d]
    assert (TILE % T != 0) == (T != 64)
    F = rotated_footprint(i)[0] * np.float32(1.5)
    mid = len(c["pts"]) // 2
    tile = TILE // T                                                             # the points of the first round (T = 64: exactly one)
    for N in sorted({tile, tile + 1, SSE_POINTS - 1, SSE_POINTS, SSE_POINTS + 1, 3 * SSE_POINTS + 5}):
        pts = np.ascontiguousarray(c["pts"][mid:mid + N])
        Fe, te = each_of(N, F, taps)
        want, got = _area(eng, dp, dl, pts, F, taps), _each(eng, dp, dl, pts, Fe, te)
        torch.cuda.synchronize()
        _same(got, want, (N, taps))
        assert N < SSE_POINTS or (want[2].max() == T and want[1].abs().max() > 0.05)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. the tilt against the composition on materialised taps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_the_tilt_is_the_ordered_mean_of_shared_sample_grad_on_its_taps(i):
    t = tilt_inputs(i)
    c, eng, dp, dl = _open(i)
    d, N, Cn = len(c["shape"]), len(t["pts"]), c["C"]
    want, n_in = _composed(eng, dp, dl, t, Cn)
    img, mean, cnt, bk = _each(eng, dp, dl, t["pts"], t["foot"], t["taps"])
    u8 = eng.sample_area_each(dp, dl, _pts(t["pts"]), _pts(t["foot"]), _u8(t["taps"]), dtype=torch.uint8)
    plain = eng.sample(dp, dl, _pts(t["pts"]))
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), t["count"].astype(np.uint8)) and np.array_equal(n_in.cpu().numpy(), t["count"])
    assert np.array_equal(bk.cpu().numpy(), t["batch"].astype(np.int32))
    assert torch.equal(mean.view(torch.int32), want.view(torch.int32)), (mean - want).abs().max().item()
    kq, scale = _lattice_k(mean.cpu().numpy())
    assert mean.abs().max() > 0.05 and np.array_equal(u8.cpu().numpy(), kq.astype(np.uint8))
    assert np.array_equal(img.cpu().numpy().view(np.uint32), (kq * scale).astype(np.float32).view(np.uint32))
    # one-tap points are smoe_shared_sample_grad's values at the point itself, and smoe_shared_sample's image
    one = np.flatnonzero(t["valid"] & (t["ntap"] == 1))
    if d == 2:
        _, v1 = eng.sample_grad(dp, dl, _pts(t["pts"][one]), want_values=True)
        sel = torch.from_numpy(one).cuda()
        assert len(one) >= 100 and torch.equal(mean[sel].view(torch.int32), v1.view(torch.int32))
        assert torch.equal(img[sel].view(torch.int32), plain[sel].view(torch.int32)) and img[sel].max() > 0.05
    # behind the horizon: 0 / 0 / 0, no batch
    gone = torch.from_numpy(~t["valid"]).cuda()
    assert gone.any() and (img[gone] == 0).all() and (mean[gone] == 0).all() and (cnt[gone] == 0).all() and (bk[gone] == -1).all()
    # a centre outside the image with taps inside has their mean
    assert ((bk == -1) & (cnt > 0)).any() and (mean[(bk == -1) & (cnt > 0)].amax(dim=1) > 0).any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. independence: a point's result does not depend on the list it comes in
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 3, 5, 11], ids=[CASE_IDS[i] for i in (1, 3, 5, 11)])
def test_a_point_owes_nothing_to_the_other_points(i):
    """two plain images (two and three axes) and two option cases (train_inverse_cov, quantization_mode 3); Broadcast, Mixed and
    Tilt run all 13 cases"""
    t = tilt_inputs(i)
    c, eng, dp, dl = _open(i)
    pts, foot, taps = t["pts"], t["foot"], t["taps"]

    def run(index):
        r = _each(eng, dp, dl, pts[index], foot[index], taps[index])
        torch.cuda.synchronize()
        return [a.cpu().numpy() for a in r]

    allp = np.arange(len(pts))
    base = run(allp)
    assert base[1].any() and np.array_equal(base[2], t["count"].astype(np.uint8)) and t["ntap"].max() == 64 and base[2].max() > 8

    def same(res, index, what):
        for a, b in zip(res, base):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), np.ascontiguousarray(b[index]).view(np.uint8)), what

    perm = np.random.default_rng(11).permutation(len(pts))
    same(run(perm), perm, "a random permutation")
    same(run(allp[::3]), allp[::3], "every third point")
    same(run(allp[1:]), allp[1:], "the first point dropped: every round boundary moves")
    widest = int(np.argmax(np.abs(foot).reshape(len(pts), -1).max(axis=1)))
    ordinary = int(np.flatnonzero(t["valid"] & (t["count"] > 8))[17])
    for k in (ordinary, widest, int(np.flatnonzero(~t["valid"])[0])):
        same(run(allp[k:k + 1]), allp[k:k + 1], f"point {k} alone")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. lists
# ---------------------------------------------------------------------------------------------------------------
def test_no_lists_three_chunks_and_the_empty_batch():
    t = tilt_inputs(2)                                         # K = 144: three staging chunks without lists
    c, eng, dp, dl = _open(2)
    assert c["K"] == 144
    sparse = _each(eng, dp, dl, t["pts"], t["foot"], t["taps"])
    ones = _each(eng, dp, eng.new_lists(), t["pts"], t["foot"], t["taps"])
    none = _each(eng, dp, None, t["pts"], t["foot"], t["taps"])
    cm, cc = _composed(eng, dp, None, t, c["C"])
    torch.cuda.synchronize()
    _same(ones, none)
    assert not torch.equal(none[1], sparse[1]) and torch.equal(none[2], sparse[2]) and torch.equal(none[3], sparse[3])
    assert torch.equal(none[1].view(torch.int32), cm.view(torch.int32)) and torch.equal(none[2].to(torch.int64), cc)
    # cells wholly in the batch with the empty list: mean 0, count = the taps inside the image
    shape, bshape = c["shape"], c["bshape"]
    g = np.unravel_index(EMPTY, _grid(shape, bshape))
    lo = np.array([g[0] * bshape[0], g[1] * bshape[1]], np.float32)
    assert lo[1] == 0
    cells = np.array([lo + np.array([8.0, 16.0], np.float32), lo + np.array([8.0, 1.0], np.float32)], np.float32)
    foot = np.stack([np.diag([4.0, 4.0]), np.diag([3.0, 4.0])]).astype(np.float32)
    taps = np.array([[4, 4], [3, 4]], np.uint8)
    val, mean, cnt, bk = _each(eng, dp, dl, cells, foot, taps)
    assert (val == 0).all() and (mean == 0).all() and cnt.tolist() == [16, 9] and bk.tolist() == [EMPTY, EMPTY]
    free = _each(eng, dp, None, cells, foot, taps)
    assert (free[1] > 0).any() and free[2].tolist() == [16, 9]
    eng.close()


@pytest.mark.parametrize("image", [IMAGES[0], IMAGES[4]], ids=[_name(c) for c in (IMAGES[0], IMAGES[4])])
def test_every_tap_carries_the_list_of_its_own_batch(image):
    """disjoint lists in neighbouring batches (tests/test_gpu_shared_sample_area.py) and cells centred on the batch corners:
    the four taps of a cell lie in four batches with two disjoint lists; the footprints differ from point to point"""
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
    N = len(cen)
    size = (1.0 + 0.25 * (np.arange(N) % 5)).astype(np.float32)                 # 1 .. 2 pixels, neighbours differ
    foot = (np.eye(2, dtype=np.float32)[None] * size[:, None, None]).astype(np.float32)
    taps = np.full((N, 2), 2, np.uint8)
    tp, slot = blk.area_taps_each(cen, foot, taps)
    t = {"pts": cen, "tp": tp}
    from shared_sample_engine import point_mapping
    inside, tb, _ = point_mapping(tp.reshape(-1, 2), shape, bshape)
    t["tap_batch"] = np.where(inside.reshape(N, -1) & slot, tb.reshape(N, -1), -1)
    assert all(len(np.unique(b[:4])) == 4 and sorted(colour[b[:4]].tolist()) == [0, 0, 1, 1] for b in t["tap_batch"])
    val, mean, cnt, bk = _each(eng, dp, dl, cen, foot, taps)
    cm, cc = _composed(eng, dp, dl, t, C_)
    torch.cuda.synchronize()
    assert (cnt == 4).all() and np.array_equal(bk.cpu().numpy(), t["tap_batch"][:, 3])         # the centre: the last tap's batch
    assert torch.equal(mean.view(torch.int32), cm.view(torch.int32)) and mean.abs().max() > 0.05
    for col in (0, 1):                                           # with one list for all four taps the mean is another
        one = np.broadcast_to(lists[np.flatnonzero(colour == col)[0]], lists.shape)
        other = _each(eng, dp, _dev_lists(np.ascontiguousarray(one)), cen, foot, taps)[1]
        assert ((other - mean).abs().amax(dim=1) > 1e-4).float().mean() > 0.5
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. void points: ordinary inputs with a defined result
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 3, 10], ids=[CASE_IDS[i] for i in (1, 3, 10)])
def test_void_points(i):
    c, eng, dp, dl = _open(i)
    d, N = len(c["shape"]), len(c["pts"])
    cfgs, foot, taps = _mixed(i, N)
    base = [r.cpu().numpy() for r in _each(eng, dp, dl, c["pts"], foot, taps)]
    where = [0, SSE_POINTS - 1, SSE_POINTS, 255, 256, N - 1] + list(range(300, 420, 7))   # corners of workgroups, then interleaved
    f2, t2 = foot.copy(), taps.copy()
    for n, k in enumerate(where):
        kind = n % 5
        if kind == 0:
            t2[k, n % d] = 0
        elif kind == 1:
            t2[k, n % d] = 17
        elif kind == 2:
            t2[k] = (16, 5) + (1,) * (d - 2)
        elif kind == 3:
            f2[k, n % d, (n // d) % d] = np.nan
        else:
            f2[k, n % d, (n // d) % d] = np.inf if n % 2 else -np.inf
    void = np.zeros(N, bool)
    void[where] = True
    assert np.array_equal(blk.area_void_each(f2, t2), void) and not blk.area_void_each(foot, taps).any()
    got = [r.cpu().numpy() for r in _each(eng, dp, dl, c["pts"], f2, t2)]
    u8 = eng.sample_area_each(dp, dl, _pts(c["pts"]), _pts(f2), _u8(t2), dtype=torch.uint8).cpu().numpy()
    for a, b in zip(got[:3], base[:3]):
        assert (a[void] == 0).all() and np.array_equal(a[~void].view(np.uint8), b[~void].view(np.uint8))
    assert (u8[void] == 0).all() and np.array_equal(got[3], base[3]) and (base[2][void] > 0).any() and (base[3][void] >= 0).any()
    # every byte a tap count can hold
    tb = np.ones((256, d), np.uint8)
    tb[:, d - 1] = np.arange(256, dtype=np.uint8)
    pb = np.ascontiguousarray(c["pts"][N // 2:N // 2 + 256])
    fb = np.ascontiguousarray(np.broadcast_to(cfgs[1][0], (256, d, d)))
    gb = [r.cpu().numpy() for r in _each(eng, dp, dl, pb, fb, tb)]
    vb = blk.area_void_each(fb, tb)
    tpb, slot = blk.area_taps_each(pb, fb, tb)
    with np.errstate(invalid="ignore"):
        n_in = (blk.point_blocks(tpb, c["shape"], [1] * d, c["shape"])[0] & slot).sum(axis=1)
    assert vb.sum() == 256 - 16 and (gb[2][vb] == 0).all() and (gb[1][vb] == 0).all() and np.array_equal(gb[2], n_in) and n_in.max() > 8
    # void points only: workgroups without a single item
    g0 = [r.cpu().numpy() for r in _each(eng, dp, dl, c["pts"], foot, np.zeros((N, d), np.uint8))]
    assert not g0[0].any() and not g0[1].any() and not g0[2].any() and np.array_equal(g0[3], base[3])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. guarded buffers, unaligned inputs
# ---------------------------------------------------------------------------------------------------------------
def test_bounds_and_alignment():
    from steered_mixture_of_experts_amd import _lib
    c, eng, dp, dl = _open(1)
    C_, shape = c["C"], c["shape"]
    lib, cp = eng.lib, eng._cparams(dp)
    rng = np.random.default_rng(23)
    allpts = (rng.uniform(-0.04, 1.04, size=(3077, 2)) * np.array(shape)).astype(np.float32)
    _, allfoot, alltaps = _mixed(1, len(allpts))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points, n, foot, taps, values, fmt, mean, count, batch):
        return lib.smoe_shared_sample_area_each(eng._h, C.byref(cp), ptr(dl), ptr(points), n, ptr(foot), ptr(taps), ptr(values), fmt,
                                                ptr(mean), ptr(count), ptr(batch), None)

    assert call(None, 0, None, None, None, 0, None, None, None) == 0            # num_points == 0: a no-op that needs no pointers
    for N in (0, 1, SSE_POINTS - 1, SSE_POINTS, SSE_POINTS + 1, 3077):
        pts, foot, taps = _pts(allpts[:N]), _pts(allfoot[:N]), _u8(alltaps[:N])
        if N:
            base = _each(eng, dp, dl, pts, foot, taps)
            base_u8 = eng.sample_area_each(dp, dl, pts, foot, taps, dtype=torch.uint8)
            assert N < SSE_POINTS or ((base[3] < 0).any() and base[2].max() == 6)
            # footprints one to three floats off a 16-byte line, taps one to three bytes off a dword: the same bits
            fbuf = torch.zeros((N * 4 + 8,), dtype=torch.float32, device="cuda")
            tbuf = torch.zeros((N * 2 + 8,), dtype=torch.uint8, device="cuda")
            for fs, ts in ((1, 1), (0, 3), (3, 0), (2, 2)):
                fv, tv = fbuf[fs:fs + N * 4].view(N, 2, 2), tbuf[ts:ts + N * 2].view(N, 2)
                fv.copy_(foot)
                tv.copy_(taps)
                assert fv.data_ptr() % 16 == 4 * fs and tv.data_ptr() % 4 == ts and foot.data_ptr() % 16 == 0 and taps.data_ptr() % 4 == 0
                _same(_each(eng, dp, dl, pts, fv, tv), base, (N, fs, ts))
        else:
            assert tuple(eng.sample_area_each(dp, dl, pts, foot, taps).shape) == (0, C_)
        for shift in (0, 1, 3):
            vbuf, vview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            ubuf, uview = _guarded((N, C_), torch.uint8, 201, shift=shift)
            mbuf, mview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            cbuf, cview = _guarded((N,), torch.uint8, 199, shift=shift)
            bbuf, bview = _guarded((N,), torch.int32, -9, shift=shift)
            monly, monly_view = _guarded((N, C_), torch.float32, SENT, shift=shift)
            assert call(pts, N, foot, taps, vview, _lib.SMOE_IMAGE_F32, mview, cview, bview) == 0, lib.smoe_last_error()
            assert call(pts, N, foot, taps, uview, _lib.SMOE_IMAGE_U8, None, None, None) == 0, lib.smoe_last_error()    # the extras are optional
            assert call(pts, N, foot, taps, None, _lib.SMOE_IMAGE_F32, monly_view, None, None) == 0, lib.smoe_last_error()   # and so is values
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
# 9. the argument checks with a real handle
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_with_a_handle():
    """every refusal of the entry point, and a correct call after each.  (The 160 KB LDS limit is the one a handle cannot
    reach: the plan's limit is checked on the host, tests/host/shared_sample_area_each_args_driver.cpp.)"""
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
    _, fh, th = _mixed(0, 64)
    dfoot, dtaps = _pts(fh), _u8(th)
    want = [t.cpu().numpy().view(np.uint32) for t in eng.sample_area_each(dp, dl, dpts, dfoot, dtaps, want_mean=True)]
    vbuf, vview = _guarded((64, C_), torch.float32, SENT)
    mbuf, mview = _guarded((64, C_), torch.float32, SENT)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def each(h=eng._h, params=cp, pts=dpts, n=64, foot=dfoot, taps=dtaps, values=vview, fmt=0, mean=mview):
        return lib.smoe_shared_sample_area_each(h, None if params is None else C.byref(params), vp(dl), vp(pts), n, vp(foot), vp(taps),
                                                vp(values), fmt, vp(mean), None, None, None)

    INV, UNS = _lib.SMOE_ERR_INVALID, _lib.SMOE_ERR_UNSUPPORTED
    for kwargs, code, word in [(dict(h=C.c_void_p(None)), INV, b"handle"), (dict(params=None), INV, b"p "),
                               (dict(params=bad), INV, b"p "), (dict(pts=None), INV, b"points"),
                               (dict(foot=None), INV, b"footprints"), (dict(taps=None), INV, b"taps"),
                               (dict(values=None, mean=None), INV, b"values or mean"), (dict(fmt=5), INV, b"image_format"),
                               (dict(n=-1), INV, b"num_points"), (dict(n=1 << 41), UNS, b"2^31")]:
        vbuf.fill_(SENT)
        mbuf.fill_(SENT)
        assert each(**kwargs) == code, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_sample_area_each" in err and word in err, (kwargs, err)
        torch.cuda.synchronize()
        assert (vbuf == SENT).all() and (mbuf == SENT).all()   # nothing was written
        assert each() == 0, lib.smoe_last_error()              # the call after a refused one succeeds
        torch.cuda.synchronize()
        assert np.array_equal(vview.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(mview.cpu().numpy().view(np.uint32), want[1])
    assert each(n=0, pts=None, foot=None, taps=None, values=None, mean=None) == 0    # a no-op
    deep = _engine(shape, bshape, C_, K, precision=10)         # uint8 cannot hold a 10-bit lattice
    u8 = torch.empty((64, C_), dtype=torch.uint8, device="cuda")
    assert each(h=deep._h, values=u8, fmt=_lib.SMOE_IMAGE_U8) == UNS and b"precision" in lib.smoe_last_error()
    assert each(h=deep._h, values=None, fmt=_lib.SMOE_IMAGE_U8) == 0
    deep.close()
    wide = _engine((16, (1 << 24) + 16), (16, 16), 1, 1)       # an axis the point form cannot resolve exactly in fp32
    wp = {k: torch.zeros_like(v[:1]) for k, v in dp.items()}
    wcp = wide._cparams(wp)
    assert each(h=wide._h, params=wcp) == UNS and b"2^24" in lib.smoe_last_error()
    wide.close()
    torch.cuda.synchronize()
    # the engine's own checks
    for kw in (dict(lists=dl[:3]), dict(points=dpts.cpu()), dict(out=torch.empty((64, C_ + 1), device="cuda")), dict(dtype=torch.float64),
               dict(footprints=dfoot[:63]), dict(footprints=dfoot.double()), dict(footprints=dfoot.cpu()), dict(taps=dtaps[:63]),
               dict(taps=dtaps.to(torch.int32)), dict(taps=dtaps.cpu()), dict(taps=(3, 2))):
        args = dict(lists=dl, points=dpts, footprints=dfoot, taps=dtaps)
        args.update(kw)
        with pytest.raises(ValueError, match="sample_area_each"):
            eng.sample_area_each(dp, **args)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 10. the facade on the device
# ---------------------------------------------------------------------------------------------------------------
def test_facade_on_the_device():
    from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe, footprint_taps_each_torch, map_footprints_torch
    shape, bshape, C_ = (64, 96), (32, 32), 3
    b = synthetic_blocks(24, (16, 16), C_, 3)
    img = blk.blocks_to_image(b, shape, (16, 16))
    s = SharedSmoe(img, kernels_per_dim=[6, 8], train_inverse_cov=False, batch_size=list(bshape), use_determinant=True, use_yuv=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(0.01))
    s.train(6, val_iter=3, ukl_iter=3)
    eng, params, lists = s._engine, s._params, s._render_lists(False)
    E = (14, 18)
    M = np.array([[2.5, -1.0], [1.0, 2.75]])                                                    # dyadic: the map's differences are exact
    A = np.concatenate([M, (np.array([32.0, 48.0]) - M @ np.array([7.0, 9.0]))[:, None]], axis=1)
    H = np.concatenate([A, [[0.0, 0.0, 1.0]]], axis=0)
    warp = s.eval_warp(A, E, taps="auto", to_host=False)
    proj = s.eval_projective(H, E, to_host=False)
    assert proj.is_cuda and proj.dtype == torch.float32 and tuple(proj.shape) == (14, 18, 3) and torch.equal(proj, warp) and proj.max() > 0.05
    assert torch.equal(s.eval_projective(H, E, taps=None, to_host=False), s.eval_points(blk.warp_points(A, E), to_host=False))
    assert np.array_equal(s.eval_projective(H, E), warp.cpu().numpy())                          # host out
    # a tilted view: the engine call behind it, and the horizon
    Ht = H.copy()
    Ht[2, 0] = -1.0 / (0.9 * E[0])
    Ht[:2, :2] += np.outer([32.0, 48.0], Ht[2, :2])
    pts, foot, valid = blk.projective_points(Ht, E)
    taps = blk.footprint_taps_each(foot.reshape(-1, 2, 2))
    v, mean, cnt = s.eval_projective(Ht, E, to_host=False, want_mean=True, want_count=True)
    ev, em, ec = eng.sample_area_each(params, lists, _pts(pts.reshape(-1, 2)), _pts(foot.reshape(-1, 2, 2)), _u8(taps),
                                      want_mean=True, want_count=True)
    assert torch.equal(v.reshape(-1, 3), ev) and torch.equal(mean.reshape(-1, 3).view(torch.int32), em.view(torch.int32)) and torch.equal(cnt.reshape(-1), ec)
    gone = torch.from_numpy(~valid).cuda()
    assert gone.sum() == 18 and (v[gone] == 0).all() and (cnt[gone] == 0).all() and cnt.max() > 16 and len(np.unique(taps, axis=0)) > 4
    dp_, df_ = _pts(pts), _pts(foot)
    assert torch.equal(footprint_taps_each_torch(df_.reshape(-1, 2, 2)).cpu(), torch.from_numpy(taps))
    assert torch.equal(s.eval_points_area_each(dp_, df_, to_host=False), v)                     # device in: taps made on the device
    assert np.array_equal(s.eval_points_area_each(pts, foot), v.cpu().numpy())                  # host in, host out
    assert torch.equal(s.eval_points_area_each(dp_, df_, taps=_u8(taps.reshape(14, 18, 2)), to_host=False), v)
    u8 = s.eval_points_area_each(dp_, df_, dtype=np.uint8, to_host=False)
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.round(v * 255).to(torch.uint8))
    assert tuple(s.eval_points_area_each(dp_, df_, to_host=False, use_lists=False).shape) == (14, 18, 3)
    # the map of the affine view: its footprints are M exactly; on the device they are made there
    p = blk.warp_points(A, E)
    assert np.array_equal(map_footprints_torch(_pts(p)).cpu().numpy(), blk.map_footprints(p))
    m = s.eval_map(_pts(p), to_host=False)
    assert m.is_cuda and torch.equal(m, warp) and np.array_equal(s.eval_map(p), warp.cpu().numpy())
    assert torch.equal(s.eval_map(_pts(p), taps=None, to_host=False), s.eval_points(_pts(p), to_host=False))
    q = (p + 0.004 * (p - 20.0) ** 2).astype(np.float32)                                       # a map that is not affine
    fq = blk.map_footprints(q)
    mq = s.eval_map(_pts(q), to_host=False)
    eq = eng.sample_area_each(params, lists, _pts(q.reshape(-1, 2)), _pts(fq.reshape(-1, 2, 2)), _u8(blk.footprint_taps_each(fq.reshape(-1, 2, 2))))
    assert torch.equal(mq.reshape(-1, 3), eq) and not torch.equal(mq, s.eval_points(_pts(q), to_host=False))
    with pytest.raises(ValueError):
        s.eval_points_area_each(pts, foot, taps=(9, 8))
