"""GPU tests of the area-averaged point decoder with per-point footprints (smoe_sample_area_each through the C ABI and the
facade).  The specification is one sentence -- the result for a point is bit for bit that of smoe_sample_area called with that
one point, its footprint and its taps -- and every comparison here is bitwise, so there is no tolerance: broadcast footprints
against smoe_sample_area, three configurations mixed within every wavefront, the tilt of every case
(tests/sample_area_each_cases.py) against the composition on materialised taps (``blocks.area_taps_each``, smoe_sample_grad's
values, the ordered fp32 sum over the inside taps, one division), independence of a point from the list it comes in and from
the path its workgroup takes, void points, guarded and unaligned buffers, and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

from render_cases import _guarded, _image
from sample_area_cases import rotated_footprint
from sample_area_each_cases import each_of, mixed_configs, tilt_inputs
from sample_grad_cases import CASES, CASE_IDS, case_inputs
from steered_mixture_of_experts_amd import blocks as blk
from test_gpu_render_view import _open
from test_gpu_sample import _dev, _rotated
from test_gpu_sample_area import _area, _bits, _lattice

pytestmark = pytest.mark.gpu


def _each(eng, dp, act, grid, length, pts, foot, taps, **kw):
    """lattice values, mean, count, block (host arrays or device tensors in)"""
    dv = lambda a: a if torch.is_tensor(a) else _dev(a)
    return eng.sample_area_each(dp, act, grid, length, dv(pts), dv(foot), dv(taps), want_mean=True, want_count=True, want_block=True, **kw)


def _same(got, want, what=""):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a,
                                                  b.view(torch.uint8) if b.dtype != torch.uint8 else b), what


# ---------------------------------------------------------------------------------------------------------------
# 1. broadcast: a constant footprint and constant taps are smoe_sample_area
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_broadcast_footprints_are_sample_area(i, blended):
    c = case_inputs(i, blended)
    F, taps = rotated_footprint(i)
    eng, dp, act, grid, _ = _open(tuple(c["shape"]), c["C"], c["kpd"], c["opt"])
    pts = _dev(c["pts"])
    Fe, te = each_of(len(c["pts"]), F, taps)
    want = _area(eng, dp, act, grid, c["length"], pts, F, taps, blend=c["beta"])
    got = _each(eng, dp, act, grid, c["length"], pts, Fe, te, blend=c["beta"])
    want8 = eng.sample_area(dp, act, grid, c["length"], pts, F, taps, blend=c["beta"], dtype=torch.uint8)
    got8 = eng.sample_area_each(dp, act, grid, c["length"], pts, _dev(Fe), _dev(te), blend=c["beta"], dtype=torch.uint8)
    torch.cuda.synchronize()
    assert want[1].abs().max() > 0.05 and want[2].max() == int(np.prod(taps)) and got8.dtype == torch.uint8
    _same(got, want)
    _same([got8], [want8])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. three configurations mixed within every wavefront
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_mixed_configurations_within_a_wavefront(i, blended):
    c = case_inputs(i, blended)
    d, N = len(c["shape"]), len(c["pts"])
    cfgs = mixed_configs(i)
    foot = np.stack([cfgs[k % 3][0] for k in range(N)]).astype(np.float32)
    taps = np.array([cfgs[k % 3][1] for k in range(N)], np.uint8)
    eng, dp, act, grid, _ = _open(tuple(c["shape"]), c["C"], c["kpd"], c["opt"])
    got = _each(eng, dp, act, grid, c["length"], c["pts"], foot, taps, blend=c["beta"])
    for r, (F, tp) in enumerate(cfgs):
        want = _area(eng, dp, act, grid, c["length"], np.ascontiguousarray(c["pts"][r::3]), F, tp, blend=c["beta"])
        torch.cuda.synchronize()
        _same([g[r::3].contiguous() for g in got], want, f"configuration {r}")
        assert want[2].max() == int(np.prod(tp))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. the tilt against the composition on materialised taps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_the_tilt_is_the_ordered_mean_of_sample_grad_on_its_taps(i, blended):
    c = case_inputs(i, blended)
    t = tilt_inputs(i)
    d, N, Cn = len(c["shape"]), len(t["pts"]), c["C"]
    eng, dp, act, grid, _ = _open(tuple(c["shape"]), Cn, c["kpd"], c["opt"])
    # the composition: every slot of every point through smoe_sample_grad (a slot that holds no tap is NaN, hence outside)
    _, val, bk = eng.sample_grad(dp, act, grid, c["length"], _dev(t["tp"].reshape(-1, d)), blend=c["beta"], want_values=True, want_block=True)
    val, inside = val.reshape(N, blk.AREA_TAPS, Cn), (bk >= 0).reshape(N, blk.AREA_TAPS)
    assert np.array_equal(inside.cpu().numpy(), t["inside"])
    acc = torch.zeros((N, Cn), dtype=torch.float32, device="cuda")
    for s in range(blk.AREA_TAPS):                                             # the stated order: one fp32 add per inside tap
        acc = torch.where(inside[:, s, None], acc + val[:, s], acc)
    n_in = inside.sum(dim=1)
    want = torch.where(n_in[:, None] > 0, acc / n_in.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(acc))
    img, mean, cnt, bkc = _each(eng, dp, act, grid, c["length"], t["pts"], t["foot"], t["taps"], blend=c["beta"])
    u8 = eng.sample_area_each(dp, act, grid, c["length"], _dev(t["pts"]), _dev(t["foot"]), _dev(t["taps"]), blend=c["beta"], dtype=torch.uint8)
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), t["count"].astype(np.uint8)) and np.array_equal(n_in.cpu().numpy(), t["count"])
    assert torch.equal(mean.view(torch.int32), want.view(torch.int32)), (mean - want).abs().max().item()
    q, kq = _lattice(mean.cpu().numpy())
    assert mean.abs().max() > 0.05 and np.array_equal(_bits(img.cpu().numpy()), _bits(q)) and np.array_equal(u8.cpu().numpy(), kq)
    # one-tap points are smoe_sample_grad's values at the point itself
    one = np.flatnonzero(t["valid"] & (np.prod(t["taps"].astype(np.int64), axis=1) == 1))
    if d == 2:
        _, v1 = eng.sample_grad(dp, act, grid, c["length"], _dev(t["pts"][one]), blend=c["beta"], want_values=True)
        assert len(one) >= 100 and torch.equal(mean[_dev(one)].view(torch.int32), v1.view(torch.int32))
    # behind the horizon: 0 / 0 / 0, no block
    gone = _dev(~t["valid"])
    assert gone.any() and (img[gone] == 0).all() and (mean[gone] == 0).all() and (cnt[gone] == 0).all() and (bkc[gone] == -1).all()
    # a centre outside the image with taps inside has their mean
    assert ((bkc == -1) & (cnt > 0)).any() and (mean[(bkc == -1) & (cnt > 0)].amax(dim=1) > 0).any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. independence: a point's result does not depend on the list it comes in, nor on the path its workgroup takes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_a_point_owes_nothing_to_the_other_points_or_to_the_path(beta, monkeypatch):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    monkeypatch.delenv("SMOE_SAMPLE_RECORDS", raising=False)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    t = tilt_inputs(0)
    assert CASES[0][:3] == (shape, C_, kpd)
    length = [g * n for g, n in zip(grid, shape)]
    pts, foot, taps = t["pts"], t["foot"], t["taps"]
    with np.errstate(invalid="ignore"):
        inside, g, _u = blk.point_blocks(pts, shape, grid, length)
    own = np.where(inside, np.ravel_multi_index(tuple(g.T), grid), -1)
    order = np.argsort(own, kind="stable")                                     # sorted by the centre's block

    def run(index):
        return [r.cpu().numpy() for r in _each(eng, dp, act, grid, length, pts[index], foot[index], taps[index], blend=beta)]

    base = run(order)
    assert (base[3] == own[order]).all() and base[1].any() and np.array_equal(base[2], t["count"][order].astype(np.uint8)) and (base[2] == 1).sum() > 100

    def same(res, index, what):
        for a, b in zip(res, base):
            assert np.array_equal(_bits(a), _bits(b[index])), what

    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    allp = np.arange(len(pts))
    same(run(allp), inv, "row-major order")
    perm = np.random.default_rng(11).permutation(len(pts))
    same(run(perm), inv[perm], "a random permutation")
    same(run(allp[::3]), inv[::3], "every third point")
    for k in (17, int(np.argmax(np.abs(foot).reshape(len(pts), -1).max(axis=1))), int(np.flatnonzero(~t["valid"])[0])):
        same(run(allp[k:k + 1]), inv[k:k + 1], f"point {k} alone")
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "4")
    same(run(perm), inv[perm], "shuffled, at most 4 records staged")
    same(run(order), np.arange(len(order)), "sorted, at most 4 records staged")
    monkeypatch.setenv("SMOE_SAMPLE_RECORDS", "0")
    same(run(order), np.arange(len(order)), "sorted, nothing staged")
    same(run(allp), inv, "row-major, nothing staged")
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. void points: ordinary inputs with a defined result
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
@pytest.mark.parametrize("i", [0, 3], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_void_points(i, beta):
    c = case_inputs(i, False)
    d, N = len(c["shape"]), len(c["pts"])
    bl = None if beta is None else ((2, 2, 1) if d == 3 else 2)
    cfgs = mixed_configs(i)
    foot = np.stack([cfgs[k % 3][0] for k in range(N)]).astype(np.float32)
    taps = np.array([cfgs[k % 3][1] for k in range(N)], np.uint8)
    eng, dp, act, grid, _ = _open(tuple(c["shape"]), c["C"], c["kpd"], c["opt"])
    base = [r.cpu().numpy() for r in _each(eng, dp, act, grid, c["length"], c["pts"], foot, taps, blend=bl)]
    where = [0, 63, 64, 255, 256, N - 1] + list(range(300, 420, 7))             # the corners of wavefronts and workgroups, then interleaved
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
    got = [r.cpu().numpy() for r in _each(eng, dp, act, grid, c["length"], c["pts"], f2, t2, blend=bl)]
    u8 = eng.sample_area_each(dp, act, grid, c["length"], _dev(c["pts"]), _dev(f2), _dev(t2), blend=bl, dtype=torch.uint8).cpu().numpy()
    for a, b in zip(got[:3], base[:3]):
        assert (a[void] == 0).all() and np.array_equal(_bits(a[~void]), _bits(b[~void]))
    assert (u8[void] == 0).all() and np.array_equal(got[3], base[3]) and (base[2][void] > 0).any() and (base[3][void] >= 0).any()
    # every byte a tap count can hold, and every point void at once
    allb = np.arange(256, dtype=np.uint8)
    tb = np.ones((256, d), np.uint8)
    tb[:, d - 1] = allb
    pb, fb = np.ascontiguousarray(c["pts"][N // 2:N // 2 + 256]), np.ascontiguousarray(np.broadcast_to(cfgs[1][0], (256, d, d)))
    gb = [r.cpu().numpy() for r in _each(eng, dp, act, grid, c["length"], pb, fb, tb, blend=bl)]
    vb = blk.area_void_each(fb, tb)
    tpb, slot = blk.area_taps_each(pb, fb, tb)
    with np.errstate(invalid="ignore"):
        n_in = (blk.point_blocks(tpb, c["shape"], c["grid"], c["length"])[0] & slot).sum(axis=1)
    assert vb.sum() == 256 - 16 and (gb[2][vb] == 0).all() and (gb[1][vb] == 0).all() and np.array_equal(gb[2], n_in) and n_in.max() > 8
    t0 = np.zeros((N, d), np.uint8)
    g0 = [r.cpu().numpy() for r in _each(eng, dp, act, grid, c["length"], c["pts"], foot, t0, blend=bl)]
    assert not g0[0].any() and not g0[1].any() and not g0[2].any() and np.array_equal(g0[3], base[3])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. guarded buffers, unaligned inputs
# ---------------------------------------------------------------------------------------------------------------
SENT = -7.0


@pytest.mark.parametrize("beta", [None, 2], ids=["plain", "blend"])
def test_bounds_and_alignment(beta):
    shape, C_, kpd = (16, 16), 3, (2, 2)
    eng, dp, act, grid, _ = _open(shape, C_, kpd)
    length = [g * n for g, n in zip(grid, shape)]
    allpts = _rotated(shape, grid, (61, 83), -31.0, 0.8)                       # some of them outside
    assert not blk.point_blocks(allpts, shape, grid, length)[0].all()
    cfgs = mixed_configs(0)
    allfoot = np.stack([cfgs[k % 3][0] for k in range(len(allpts))]).astype(np.float32)
    alltaps = np.array([cfgs[k % 3][1] for k in range(len(allpts))], np.uint8)
    lib, cp = eng.lib, eng._cparams(dp)
    g3, l3 = (C.c_int32 * 3)(*(list(grid) + [1])), (C.c_int32 * 3)(*(list(length) + [1]))
    bl = None if beta is None else (C.c_float * 3)(float(beta), float(beta), 0.0)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points, n, foot, taps, values, fmt, mean, count, block):
        return lib.smoe_sample_area_each(eng._h, C.byref(cp), C.c_void_p(act.data_ptr()), g3, l3, ptr(points), n, ptr(foot), ptr(taps),
                                         bl, ptr(values), fmt, ptr(mean), ptr(count), ptr(block), None)

    from steered_mixture_of_experts_amd import _lib
    for N in (0, 1, 255, 257, 3 * 1024 + 5):
        pts, foot, taps = _dev(allpts[:N]), _dev(allfoot[:N]), _dev(alltaps[:N])
        if N:
            base = _each(eng, dp, act, grid, length, pts, foot, taps, blend=beta)
            base_u8 = eng.sample_area_each(dp, act, grid, length, pts, foot, taps, blend=beta, dtype=torch.uint8)
            # footprints one float off a 16-byte line, taps one byte off a dword: the same bits
            fbuf = torch.zeros((N * 4 + 8,), dtype=torch.float32, device="cuda")
            tbuf = torch.zeros((N * 2 + 8,), dtype=torch.uint8, device="cuda")
            for fs, ts in ((1, 1), (0, 3), (3, 0), (2, 2)):
                fv, tv = fbuf[fs:fs + N * 4].view(N, 2, 2), tbuf[ts:ts + N * 2].view(N, 2)
                fv.copy_(foot)
                tv.copy_(taps)
                assert fv.data_ptr() % 16 == 4 * fs and tv.data_ptr() % 4 == ts and foot.data_ptr() % 16 == 0 and taps.data_ptr() % 4 == 0
                _same(_each(eng, dp, act, grid, length, pts, fv, tv, blend=beta), base, (N, fs, ts))
        for shift in (0, 1, 3):
            vbuf, vview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            ubuf, uview = _guarded((N, C_), torch.uint8, 201, shift=shift)
            mbuf, mview = _guarded((N, C_), torch.float32, SENT, shift=shift)
            cbuf, cview = _guarded((N,), torch.uint8, 199, shift=shift)
            bbuf, bview = _guarded((N,), torch.int32, -9, shift=shift)
            monly, monly_view = _guarded((N, C_), torch.float32, SENT, shift=shift)
            assert call(pts, N, foot, taps, vview, _lib.SMOE_IMAGE_F32, mview, cview, bview) == 0, lib.smoe_last_error()
            assert call(pts, N, foot, taps, uview, _lib.SMOE_IMAGE_U8, None, None, None) == 0, lib.smoe_last_error()    # the extras are optional
            assert call(pts, N, foot, taps, None, _lib.SMOE_IMAGE_F32, monly_view, None, None) == 0 or N == 0, lib.smoe_last_error()   # and so is values
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
    from steered_mixture_of_experts_amd.smoe import Adam, Smoe, footprint_taps_each_torch, map_footprints_torch
    img = _image(40, 56, 3)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(4, val_iter=4)
    params, active, center = s._whole_model(False)
    E = (14, 18)
    M = np.array([[2.5, -1.0], [1.0, 2.75]])                                                    # dyadic: the map's differences are exact
    A = np.concatenate([M, (np.array([20.0, 28.0]) - M @ np.array([7.0, 9.0]))[:, None]], axis=1)
    H = np.concatenate([A, [[0.0, 0.0, 1.0]]], axis=0)
    warp = s.render_warp(A, E, taps="auto", blend=2, to_host=False)
    proj = s.render_projective(H, E, blend=2, to_host=False)
    assert proj.is_cuda and proj.dtype == torch.float32 and tuple(proj.shape) == (14, 18, 3) and torch.equal(proj, warp) and proj.max() > 0.05
    assert torch.equal(s.render_projective(H, E, taps=None, blend=2, to_host=False), s.render_warp(A, E, blend=2, to_host=False))
    assert np.array_equal(s.render_projective(H, E, blend=2), warp.cpu().numpy())                # host out
    # a tilted view: the engine call behind it, and the horizon
    Ht = H.copy()
    Ht[2, 0] = -1.0 / (0.9 * E[0])
    Ht[:2, :2] += np.outer([20.0, 28.0], Ht[2, :2])
    pts, foot, valid = blk.projective_points(Ht, E)
    taps = blk.footprint_taps_each(foot.reshape(-1, 2, 2))
    v, mean, cnt = s.render_projective(Ht, E, blend=2, to_host=False, want_mean=True, want_count=True)
    ev, em, ec = s._engine.sample_area_each(params, active, s.grid, [40, 56], _dev(pts.reshape(-1, 2)), _dev(foot.reshape(-1, 2, 2)),
                                            _dev(taps), blend=[2.0, 2.0], want_mean=True, want_count=True, center_grid=center)
    assert torch.equal(v.reshape(-1, 3), ev) and torch.equal(mean.reshape(-1, 3).view(torch.int32), em.view(torch.int32)) and torch.equal(cnt.reshape(-1), ec)
    gone = _dev(~valid)
    assert gone.sum() == 18 and (v[gone] == 0).all() and (cnt[gone] == 0).all() and cnt.max() > 16 and len(np.unique(taps, axis=0)) > 4
    dp_, df_ = _dev(pts), _dev(foot)
    assert torch.equal(footprint_taps_each_torch(df_.reshape(-1, 2, 2)).cpu(), torch.from_numpy(taps))
    assert torch.equal(s.sample_area_each(dp_, df_, blend=2, to_host=False), v)                  # device in: taps made on the device
    assert np.array_equal(s.sample_area_each(pts, foot, blend=2), v.cpu().numpy())               # host in, host out
    assert torch.equal(s.sample_area_each(dp_, df_, taps=_dev(taps.reshape(14, 18, 2)), blend=2, to_host=False), v)
    u8 = s.sample_area_each(dp_, df_, blend=2, dtype=np.uint8, to_host=False)
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.round(v * 255).to(torch.uint8))
    # the map of the affine view: its footprints are M exactly; on the device they are made there
    p = blk.warp_points(A, E)
    assert np.array_equal(map_footprints_torch(_dev(p)).cpu().numpy(), blk.map_footprints(p))
    m = s.render_map(_dev(p), blend=2, to_host=False)
    assert m.is_cuda and torch.equal(m, warp) and np.array_equal(s.render_map(p, blend=2), warp.cpu().numpy())
    q = (p + 0.004 * (p - 20.0) ** 2).astype(np.float32)                                       # a map that is not affine
    fq = blk.map_footprints(q)
    assert np.array_equal(map_footprints_torch(_dev(q)).cpu().numpy().view(np.uint32), fq.view(np.uint32))
    mq = s.render_map(_dev(q), blend=2, to_host=False)
    eq = s._engine.sample_area_each(params, active, s.grid, [40, 56], _dev(q.reshape(-1, 2)), _dev(fq.reshape(-1, 2, 2)),
                                    _dev(blk.footprint_taps_each(fq.reshape(-1, 2, 2))), blend=[2.0, 2.0], center_grid=center)
    assert torch.equal(mq.reshape(-1, 3), eq) and not torch.equal(mq, s.sample(_dev(q), blend=2, to_host=False))
    with pytest.raises(ValueError):
        s.sample_area_each(pts, foot, taps=(9, 8))
