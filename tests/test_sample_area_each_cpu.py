"""CPU tests of the host layer of the area-averaged point decoder with per-point footprints: ``blocks.area_taps_each`` /
``footprint_taps_each`` / ``projective_points`` / ``map_footprints``, the tilt cases (tests/sample_area_each_cases.py),
``Smoe.sample_area_each`` / ``render_projective`` / ``render_map`` driven through the oracle-backed stand-in engine
(tests/sample_area_each_engine.py), the CLI's ``--homography``, and what the C entry point checks without a handle."""
import os
import re

import numpy as np
import pytest
import torch

from sample_area_each_cases import each_of, mixed_configs, tilt_inputs, tilt_matrix
from sample_area_each_engine import OracleSampleAreaEachEngine
from sample_area_engine import OracleSampleAreaEngine
from sample_grad_cases import CASES, CASE_IDS, case_inputs
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd import utils
from steered_mixture_of_experts_amd.smoe import Adam, Smoe, footprint_taps_each_torch, map_footprints_torch
from test_view_render_cpu import _image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the statements of the arithmetic
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_area_taps_each_with_a_constant_footprint_is_area_taps(d):
    rng = np.random.default_rng(5)
    pts = (rng.random((300, d)) * 90 - 10).astype(np.float32)
    pts[7, 0] = np.nan
    for taps in ([(3, 2), (1, 1), (8, 8), (16, 4), (5, 1)] if d == 2 else [(2, 2, 2), (4, 4, 4), (1, 1, 1), (3, 1, 5), (16, 2, 2)]):
        F = (rng.standard_normal((d, d)) * 3).astype(np.float32)
        want = blk.area_taps(pts, F, taps)
        Fe, te = each_of(len(pts), F, taps)
        got, valid = blk.area_taps_each(pts, Fe, te)
        T = int(np.prod(taps))
        assert got.dtype == np.float32 and got.shape == (300, 64, d) and valid.shape == (300, 64) and valid.dtype == bool
        assert valid[:, :T].all() and not valid[:, T:].any() and np.isnan(got[:, T:]).all()
        assert np.array_equal(got[:, :T].view(np.uint32), want.view(np.uint32))                # bit for bit, NaN included


def test_area_taps_each_void_points_and_errors():
    pts = np.zeros((6, 2), np.float32) + 5
    F = np.tile(np.eye(2, dtype=np.float32), (6, 1, 1))
    F[4, 0, 1], F[5, 1, 0] = np.nan, np.inf
    taps = np.array([[2, 2], [0, 2], [17, 1], [16, 5], [2, 2], [2, 2]], np.uint8)
    tp, valid = blk.area_taps_each(pts, F, taps)
    assert np.array_equal(blk.area_void_each(F, taps), [False, True, True, True, True, True])
    assert valid[0, :4].all() and not valid[0, 4:].any() and not valid[1:].any() and np.isnan(tp[1:]).all()
    for bad in [dict(points=pts[0]), dict(footprints=F[:5]), dict(footprints=F[:, :1]), dict(taps=taps[:, :1]),
                dict(taps=taps.astype(np.float32))]:
        kw = dict(points=pts, footprints=F, taps=taps)
        kw.update(bad)
        with pytest.raises(ValueError):
            blk.area_taps_each(**kw)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_footprint_taps_each_is_footprint_taps_row_by_row(d):
    rng = np.random.default_rng(17 + d)
    F = (rng.standard_normal((1000, d, d)) * rng.choice([0.3, 2.0, 6.0, 20.0], size=(1000, 1, 1))).astype(np.float32)
    edge = [0.0, 0.999, 1.0, 16.5, 1e6]
    F[:len(edge)] = np.array(edge, np.float32)[:, None, None] * np.eye(d, dtype=np.float32)
    F[len(edge):2 * len(edge)] = np.array(edge, np.float32)[:, None, None]                     # every entry: the product cap bites
    got = blk.footprint_taps_each(F)
    assert got.dtype == np.uint8 and got.shape == (1000, d)
    for i in range(1000):
        assert tuple(got[i]) == blk.footprint_taps(F[i]), i
    assert (np.prod(got.astype(np.int64), axis=1) <= 64).all() and got.min() >= 1 and got.max() <= 16
    assert tuple(got[0]) == (1,) * d and tuple(got[1]) == (1,) * d and tuple(got[2]) == (1,) * d
    assert tuple(got[3]) == ((16,) if d == 1 else (8, 8) if d == 2 else (4, 4, 4)) and tuple(got[4]) == tuple(got[3])
    for v in (np.nan, np.inf, -np.inf):                                                        # not finite: taps 0, the point is void
        G = F[:3].copy()
        G[1, d - 1, 0] = v
        t = blk.footprint_taps_each(G)
        assert (t[1] == 0).all() and np.array_equal(t[[0, 2]], got[[0, 2]]) and blk.area_void_each(G, t)[1]
        with pytest.raises(ValueError):
            blk.footprint_taps(G[1])
    assert torch.equal(footprint_taps_each_torch(torch.from_numpy(F)), torch.from_numpy(got))  # the facade's device statement
    with pytest.raises(ValueError):
        blk.footprint_taps_each(F[0])


def test_projective_points_with_an_affine_matrix_are_warp_points():
    for d, size in ((2, (13, 17)), (3, (5, 6, 4)), (1, (9,))):
        rng = np.random.default_rng(d)
        A = rng.standard_normal((d, d + 1)) * 3
        H = np.concatenate([A, np.array([[0.0] * d + [1.0]])], axis=0)
        pts, foot, valid = blk.projective_points(H, size)
        assert pts.dtype == np.float32 and foot.dtype == np.float32 and valid.all()
        assert pts.shape == tuple(size) + (d,) and foot.shape == tuple(size) + (d, d)
        assert np.array_equal(pts, blk.warp_points(A, size))
        assert np.array_equal(foot, np.broadcast_to(A[:, :d].astype(np.float32), foot.shape))
    for bad in [np.eye(2), np.eye(3) * np.nan, np.full((3, 3), np.inf)]:
        with pytest.raises(ValueError):
            blk.projective_points(bad, (4, 4))
    with pytest.raises(ValueError):
        blk.projective_points(np.eye(3), (4, 0))


@pytest.mark.parametrize("i", [0, 2, 3, 4], ids=[CASE_IDS[i] for i in (0, 2, 3, 4)])
def test_the_analytic_jacobian_against_central_differences(i):
    """Along view axis m the map is x(tau) = (a + b tau) / (s + w_m tau), whose n-th derivative is n! (-w_m / s(tau))^(n - 1)
    x'(tau), and x'(tau) = x'(0) (s / s(tau))^2.  The central difference with step h differs from x'(0) by at most h^2 / 6 times
    the largest third derivative over the step, h^2 (w_m / s_lo)^2 |x'(0)| (s / s_lo)^2 with s_lo = s - |w_m| h.  On top comes the
    float64 rounding of the two positions x = N / s: with mag = |M| |c| + |t| >= |N| and smag = |w| |c| + |w0|, the numerator
    carries at most (d + 2) eps mag, the denominator (d + 2) eps smag, the quotient one more eps, so a position is off by at
    most mag / s_lo ((d + 3) eps + (d + 2) eps smag / s_lo), and the difference of two over 2 h by that over h.  Last, the one
    float32 rounding of the footprint, 2^-24 |J|.  Samples with s < 4 |w_m| h (h = 2^-10: at most the one row that falls on
    the horizon itself) are left out."""
    H, E = tilt_matrix(i)
    d = len(E)
    pts, foot, valid = blk.projective_points(H, E)
    idx = np.stack(np.meshgrid(*[np.arange(e, dtype=np.float64) + 0.5 for e in E], indexing="ij"), axis=-1)
    fmap = lambda c: (c @ H[:d, :d].T + H[:d, d]) / (c @ H[d, :d] + H[d, d])[..., None]
    s = idx @ H[d, :d] + H[d, d]
    h, eps = 2.0 ** -10, 2.0 ** -52
    mag = (np.abs(idx) + h) @ np.abs(H[:d, :d]).T + np.abs(H[:d, d])                          # |M| |c| + |t| per source axis
    smag = (np.abs(idx) + h) @ np.abs(H[d, :d]) + abs(H[d, d])
    checked = 0
    for m in range(d):
        wm = abs(H[d, m])
        ok = valid & (s >= 4 * wm * h)
        e = np.zeros(d)
        e[m] = h
        with np.errstate(invalid="ignore", divide="ignore"):
            cd = (fmap(idx + e) - fmap(idx - e)) / (2 * h)
        J = foot[..., :, m].astype(np.float64)
        s_lo = s - wm * h
        with np.errstate(invalid="ignore", divide="ignore"):
            bound = h * h * (wm / s_lo)[..., None] ** 2 * np.abs(J) * (s / s_lo)[..., None] ** 2 \
                + (mag / s_lo[..., None]) * ((d + 3) * eps + (d + 2) * eps * (smag / s_lo)[..., None]) / h + 2.0 ** -24 * np.abs(J)
        assert ok.sum() >= valid.sum() - int(np.prod(E[1:])) and (np.abs(cd - J)[ok] <= bound[ok]).all(), (np.abs(cd - J)[ok] / bound[ok]).max()
        big = ok[..., None] & (np.abs(J) > 1e-3)
        assert big.any() and np.median(bound[big] / np.abs(J)[big]) < 1e-5                     # the check is a tight one
        checked += int(ok.sum())
    assert checked >= d * 800 and (~valid).any() and np.isnan(pts[~valid]).all() and (foot[~valid] == 0).all()


def test_map_footprints():
    M = np.array([[3.0, -1.0], [0.5, 2.5]])                                                    # dyadic: every difference is exact
    A = np.concatenate([M, np.array([[4.25], [-7.5]])], axis=1)
    p = blk.warp_points(A, (9, 11))
    F = blk.map_footprints(p)
    assert F.dtype == np.float32 and F.shape == (9, 11, 2, 2) and np.array_equal(F, np.broadcast_to(M.astype(np.float32), F.shape))
    # central inside, one-sided at the ends, on a map that is not affine
    q = (p + 0.01 * p * p).astype(np.float32)
    G = blk.map_footprints(q)
    f32 = np.float32
    assert np.array_equal(G[4, 5, :, 0], ((q[5, 5] - q[3, 5]) * f32(0.5)).astype(f32)) and np.array_equal(G[4, 5, :, 1], ((q[4, 6] - q[4, 4]) * f32(0.5)).astype(f32))
    assert np.array_equal(G[0, 5, :, 0], q[1, 5] - q[0, 5]) and np.array_equal(G[8, 5, :, 0], q[8, 5] - q[7, 5])
    assert np.array_equal(G[4, 0, :, 1], q[4, 1] - q[4, 0]) and np.array_equal(G[4, 10, :, 1], q[4, 10] - q[4, 9])
    # an axis of one sample: 0; of two: the one-sided difference on both
    one = blk.map_footprints(p[:1])
    assert (one[..., 0] == 0).all() and np.array_equal(one[..., 1], np.broadcast_to(M[:, 1].astype(f32), one[..., 1].shape))
    two = blk.map_footprints(p[:2])
    assert np.array_equal(two, np.broadcast_to(M.astype(f32), two.shape))
    # a NaN neighbour: the footprints that read it are not finite, hence void; nobody else's
    r = p.copy()
    r[4, 5] = np.nan
    N = blk.map_footprints(r)
    bad = ~np.isfinite(N).all(axis=(2, 3))
    want = np.zeros((9, 11), bool)
    want[[3, 5], 5] = True
    want[4, [4, 6]] = True
    assert np.array_equal(bad, want)                                                           # (its own central differences skip it)
    assert (blk.footprint_taps_each(N.reshape(-1, 2, 2)).reshape(9, 11, 2)[want] == 0).all()
    for arr in (p, q, r, p[:1], p[:, :1], p[:2]):
        assert np.array_equal(map_footprints_torch(torch.from_numpy(arr)).numpy().view(np.uint32), blk.map_footprints(arr).view(np.uint32))
    v3 = blk.map_footprints(np.zeros((3, 4, 5, 3), np.float32))
    assert v3.shape == (3, 4, 5, 3, 3)
    for badp in (np.zeros((4, 2), np.float32), np.zeros((3, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            blk.map_footprints(badp)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_the_tilt_of_a_case_meets_its_conditions(i):
    t = tilt_inputs(i)                                                                          # asserts them
    d = t["pts"].shape[1]
    assert t["taps"].dtype == np.uint8 and t["foot"].shape == (len(t["pts"]), d, d)
    assert len(mixed_configs(i)) == 3


# ---------------------------------------------------------------------------------------------------------------
# the facade on the CPU engine
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    b = blk.synthetic_blocks(15, (16, 16), 3, 99)
    img = blk.blocks_to_image(b, (48, 80), (16, 16))[:44, :75]
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True,
             engine_factory=OracleSampleAreaEachEngine)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(3, val_iter=3)
    return s


def _affine(M, E, L):
    M = np.asarray(M, np.float64)
    return np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)


def test_facade_sample_area_each(fitted):
    s = fitted
    A = _affine([[2.5, -1.0], [1.0, 2.75]], (12, 20), (44, 75))
    pts = blk.warp_points(A, (12, 20))
    M = A[:, :2]
    foot = np.broadcast_to(M.astype(np.float32), (12, 20, 2, 2)).copy()
    want = s.sample_area(pts, M, taps=(3, 3), want_mean=True, want_count=True)
    got = s.sample_area_each(pts, foot, taps=(3, 3), want_mean=True, want_count=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and got[0].shape == (12, 20, 3) and got[2].shape == (12, 20)
    assert np.array_equal(s.sample_area_each(pts, foot), want[0]) and np.array_equal(s.sample_area_each(pts, foot, taps="auto"), want[0])
    assert np.array_equal(s.sample_area_each(pts, foot, taps=3), want[0])
    tarr = np.full((12, 20, 2), 3, np.int64)
    assert np.array_equal(s.sample_area_each(pts, foot, taps=tarr), want[0])
    assert np.array_equal(s.sample_area_each(pts, foot, taps=torch.from_numpy(tarr.astype(np.uint8))), want[0])
    u8 = s.sample_area_each(pts, foot, dtype=np.uint8, blend=2)
    assert u8.dtype == np.uint8 and np.array_equal(u8, s.sample_area(pts, M, taps=(3, 3), dtype=np.uint8, blend=2))
    dev = s.sample_area_each(torch.from_numpy(pts), torch.from_numpy(foot), to_host=False, want_mean=True)
    assert torch.is_tensor(dev[0]) and np.array_equal(dev[1].numpy(), want[1])
    assert s.sample_area_each(pts.reshape(-1, 2), foot.reshape(-1, 2, 2)).shape == (240, 3)
    assert s.sample_area_each(np.zeros((0, 2), np.float32), np.zeros((0, 2, 2), np.float32)).shape == (0, 3)
    # a tuple or a list is one configuration for all points and is checked; an array is one row per point -- told apart by type,
    # also where the shapes coincide (two points of d = 2) and for a single point
    two = s.sample_area_each(pts[0, :2], foot[0, :2], taps=[3, 2], want_count=True)
    rows = s.sample_area_each(pts[0, :2], foot[0, :2], taps=np.array([[3, 2], [3, 2]]), want_count=True)
    assert np.array_equal(two[0], rows[0]) and np.array_equal(two[1], rows[1])
    with pytest.raises(ValueError):
        s.sample_area_each(pts[0, :2], foot[0, :2], taps=np.array([3, 2]))                      # an array must be [2, 2] here
    assert np.array_equal(s.sample_area_each(pts[2, 3], foot[2, 3], taps=(3, 3)), want[0][2, 3])
    assert np.array_equal(s.sample_area_each(pts[2, 3], foot[2, 3], taps=np.array([3, 3])), want[0][2, 3])
    assert (s.sample_area_each(pts[2, 3], foot[2, 3], taps=np.array([17, 1])) == 0).all()       # a row: void, a defined result
    for bad in ((17, 1), (9, 8), [0, 1], 17):
        with pytest.raises(ValueError):
            s.sample_area_each(pts[2, 3], foot[2, 3], taps=bad)                                 # a tuple: refused
    # mixed taps per point: every point is sample_area's with its own configuration; void points give 0
    tarr[::2] = (2, 4)
    tarr[3, 5] = (0, 3)
    tarr[4, 6] = (16, 5)
    tarr[5, 7] = (300, -2)                                                                      # not a byte: void
    f2 = foot.copy()
    f2[6, 8, 1, 0] = np.nan
    v, mean, cnt = s.sample_area_each(pts, f2, taps=tarr, want_mean=True, want_count=True)
    alt = s.sample_area(pts, M, taps=(2, 4), want_mean=True, want_count=True)
    void = np.zeros((12, 20), bool)
    void[3, 5] = void[4, 6] = void[5, 7] = void[6, 8] = True
    even = np.zeros((12, 20), bool)
    even[::2] = True
    for g, a, b in zip((v, mean, cnt), alt, want):
        assert np.array_equal(g[even & ~void], a[even & ~void]) and np.array_equal(g[~even & ~void], b[~even & ~void]) and (g[void] == 0).all()
    for kw in [dict(points=pts[..., :1]), dict(footprints=foot[:5]), dict(footprints=foot[..., :1]), dict(footprints=foot.astype(np.int32) > 0),
               dict(taps=(3, 3, 3)), dict(taps=0), dict(taps=17), dict(taps=(9, 8)), dict(taps="many"), dict(taps=tarr[:5]),
               dict(taps=tarr.astype(np.float32)), dict(blend=9), dict(dtype=np.float64)]:
        args = dict(points=pts, footprints=foot, taps=(3, 3))
        args.update(kw)
        with pytest.raises(ValueError):
            s.sample_area_each(**args)


def test_render_projective_and_render_map(fitted):
    s = fitted
    E = (20, 24)
    A = _affine([[2.5, -1.0], [1.0, 2.75]], E, (44, 75))                                         # dyadic: the map's differences are exact
    H = np.concatenate([A, [[0.0, 0.0, 1.0]]], axis=0)
    warp = s.render_warp(A, E, taps="auto", blend=2)
    assert np.array_equal(s.render_projective(H, E, blend=2), warp) and warp.shape == (20, 24, 3)
    assert np.array_equal(s.render_projective(H, E, taps="auto", blend=2), warp)
    assert np.array_equal(s.render_projective(H, E, taps=(2, 2)), s.render_warp(A, E, taps=(2, 2)))
    plain = s.render_warp(A, E, blend=2)
    assert np.array_equal(s.render_projective(H, E, taps=None, blend=2), plain) and np.array_equal(s.render_projective(H, E, taps=1, blend=2), plain)
    assert np.array_equal(s.render_projective(H, E, taps=(1, 1), blend=2), plain) and not np.array_equal(plain, warp)
    # a tilted view: samples behind the horizon are 0, the others sample_area_each at projective_points
    Ht = H.copy()
    Ht[2, 0] = -1.0 / (0.9 * E[0])
    Ht[:2, :2] += np.outer([22.0, 37.5], Ht[2, :2])
    pts, foot, valid = blk.projective_points(Ht, E)
    v, cnt = s.render_projective(Ht, E, want_count=True)
    assert (~valid).sum() == 2 * 24 and (v[~valid] == 0).all() and (cnt[~valid] == 0).all() and cnt.max() > 16 and v[valid].max() > 0.05
    assert np.array_equal(v, s.sample_area_each(pts, foot)) and len(np.unique(blk.footprint_taps_each(foot.reshape(-1, 2, 2)), axis=0)) > 4
    assert (s.render_projective(Ht, E, taps=None)[~valid] == 0).all()
    assert torch.is_tensor(s.render_projective(Ht, E, to_host=False))
    # the map of the affine view: footprints are M exactly, so every sample -- the interior ones in particular -- is render_warp's
    p = blk.warp_points(A, E)
    m = s.render_map(p, blend=2)
    assert np.array_equal(m[1:-1, 1:-1], warp[1:-1, 1:-1]) and np.array_equal(m, warp)
    assert np.array_equal(s.render_map(torch.from_numpy(p), blend=2), warp)
    assert np.array_equal(s.render_map(p, taps=None, blend=2), plain) and np.array_equal(s.render_map(p, taps=(1, 1), blend=2), plain)
    assert np.array_equal(s.render_map(p, taps=(2, 2)), s.render_warp(A, E, taps=(2, 2)))
    hole = p.copy()
    hole[7, 9] = np.nan
    mh = s.render_map(hole, blend=2)
    gone = np.zeros(E, bool)
    gone[[6, 7, 8], 9] = True
    gone[7, [8, 10]] = True
    assert (mh[gone] == 0).all() and np.array_equal(mh[~gone], warp[~gone])
    for call in [lambda: s.render_projective(np.eye(2), E), lambda: s.render_projective(H * np.nan, E), lambda: s.render_projective(H, (20, 24, 3)),
                 lambda: s.render_projective(H, E, taps=(9, 8)), lambda: s.render_projective(H, E, taps="some"),
                 lambda: s.render_map(p.reshape(-1, 2)), lambda: s.render_map(p[..., :1]), lambda: s.render_map(p > 0),
                 lambda: s.render_map(p, taps=(3, 3, 3))]:
        with pytest.raises(ValueError):
            call()


def test_an_engine_without_the_method_raises():
    s = Smoe(_image(32, 48), train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True,
             engine_factory=OracleSampleAreaEngine)
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area_each()")):
        s.sample_area_each(np.zeros((1, 2), np.float32), np.eye(2, dtype=np.float32)[None])
    assert s.render_projective(np.eye(3), (4, 6), taps=1).shape == (4, 6, 1)                    # all ones: sample's path


# ---------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cli_homography(tmp_path):
    import steered_mixture_of_experts_amd.smoe as smod
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--homography"] + ["1"] * 9 + ["--size", "8", "12"])
    assert a.homography == [1.0] * 9 and a.taps is None
    img = _image(32, 48)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True,
             engine_factory=OracleSampleAreaEachEngine)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig_factory = smod._default_engine_factory
    smod._default_engine_factory = lambda cfg, device: OracleSampleAreaEachEngine(cfg, device)
    try:
        out, im = str(tmp_path / "out"), str(tmp_path / "img.npy")
        H = [3.0, 0.0, 1.0, 0.0, 3.0, 2.0, -0.05, 0.0, 1.0]
        v, _, _ = rec.main(im, out, mp, homography=H, size=[10, 15])
        assert v.shape == (10, 15, 1) and np.array_equal(v, s.render_projective(np.array(H).reshape(3, 3), (10, 15)))
        assert os.path.exists(out + "/2_reconstruction_proj10x15_tapsauto.npy")
        v, _, _ = rec.main(im, out, mp, homography=H, size=[10, 15], taps=["2"], blend=[2.0])
        assert np.array_equal(v, s.render_projective(np.array(H).reshape(3, 3), (10, 15), taps=2, blend=2))
        assert os.path.exists(out + "/2_reconstruction_proj10x15_taps2_blend2.npy")
        for kw, word in [(dict(homography=H), "--homography needs --size"), (dict(homography=H[:8], size=[10, 15]), "9 numbers"),
                         (dict(homography=H, size=[10]), "--size takes"), (dict(homography=H, size=[10, 15], scale=[2.0]), "does not go with"),
                         (dict(homography=H, size=[10, 15], affine=[1.0] * 6), "does not go with"),
                         (dict(homography=H, size=[10, 15], taps=["9", "8"]), "64")]:
            with pytest.raises(ValueError, match=word):
                rec.main(im, out, mp, **kw)
    finally:
        smod._default_engine_factory = orig_factory


def test_cli_homography_refuses_whole_image_models(tmp_path):
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    from shared_render_engine import OracleSharedRenderEngine
    from steered_mixture_of_experts_amd.smoe import SharedSmoe
    img = _image(32, 32, seed=4)
    s = SharedSmoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], engine_factory=OracleSharedRenderEngine)
    assert not hasattr(s, "sample_area_each") and not hasattr(s, "render_projective") and not hasattr(s, "render_map")
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_0.pkl")
    utils.save_model(s, mp)
    old = rec._shared_engine_factory
    rec._shared_engine_factory = OracleSharedRenderEngine
    try:
        with pytest.raises(ValueError, match="--homography needs a per-block model"):
            rec.main(str(tmp_path / "img.npy"), str(tmp_path / "out"), mp, homography=[1.0, 0, 0, 0, 1, 0, 0, 0, 1], size=[8, 8])
        with pytest.raises(ValueError, match="--taps needs a per-block model"):
            rec.main(str(tmp_path / "img.npy"), str(tmp_path / "out"), mp, homography=[1.0, 0, 0, 0, 1, 0, 0, 0, 1], size=[8, 8], taps=["auto"])
    finally:
        rec._shared_engine_factory = old


# ---------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------
def test_smoe_sample_area_each_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_sample_area_each\s*\(", src)
    assert re.search(r"const float\*\s+footprints,\s*const uint8_t\*\s+taps,\s*const float\s+blend\[3\],\s*void\*\s+values,\s*int32_t\s+image_format,"
                     r"\s*float\*\s+mean,\s*uint8_t\*\s+count,\s*int32_t\*\s+block,\s*void\*\s+stream", src)
    assert hasattr(lib, "smoe_sample_area_each") and "smoe_sample_area_each" in _lib.EXPORTS
    rc = lib.smoe_sample_area_each(None, None, None, None, None, None, 5, None, None, None, None, 0, None, None, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_sample_area_each" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
