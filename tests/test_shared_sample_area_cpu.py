"""CPU tests of the area-averaged decoder of whole-image models: the numpy restatement
(tests/shared_sample_area_engine.py) against the point restatement it is composed of, ``SharedSmoe.eval_points_area`` /
``eval_view(taps=...)`` / ``eval_warp(taps=...)`` driven through the oracle-backed stand-in engine, and what the C entry point
checks without a handle."""
import os
import re

import numpy as np
import pytest
import torch

from sample_area_engine import masked_mean
from shared_sample_area_cases import CASES, CASE_IDS, area_reference, case, loose_of, rotated_footprint
from shared_sample_area_engine import OracleSharedSampleAreaEngine, shared_sample_area_reference
from shared_sample_engine import point_mapping
from shared_sample_grad_engine import OracleSharedSampleGradEngine, shared_points_grad_reference
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
from test_shared_render_cpu import _image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 3, 4], ids=[CASE_IDS[i] for i in (0, 3, 4)])
def test_one_tap_is_the_point(i):
    c = case(i)
    d = len(c["shape"])
    F = np.random.default_rng(9).normal(size=(d, d)) * 5                       # any finite footprint: the offset is 0
    for T in (np.float32, np.float64):
        r = shared_sample_area_reference(c["p"], c["lists"], c["shape"], c["bshape"], c["pts"], F, 1, c["cfg"], T)
        ref = c["ref32"] if T is np.float32 else c["ref64"]
        assert np.array_equal(r["mean"], ref["v"]) and np.array_equal(r["batch"], c["bid"])
        assert np.array_equal(r["count"], c["inside"].astype(np.int64)) and np.array_equal(r["loose"], ref["loose"] & c["inside"])
        assert np.array_equal(r["taps"][:, 0], c["pts"])


@pytest.mark.parametrize("i", [0, 4], ids=[CASE_IDS[i] for i in (0, 4)])
def test_pixel_centre_boxes_are_the_ordered_mean_of_the_pixel_values(i):
    """F = diag(4), taps = 4 at the centres 4 (i + 0.5): the taps are pixel centres, exactly.  On the ragged 21 x 25 image
    the last cells have taps outside, and 4 does not divide the 7 x 5 batches: cells cross batch borders."""
    c = case(i)
    shape, bshape = c["shape"], c["bshape"]
    E = [-(-s // 4) for s in shape]
    cen = np.stack(np.meshgrid(*[4 * (np.arange(e, dtype=np.float32) + 0.5) for e in E], indexing="ij"), axis=-1).reshape(-1, 2)
    r = shared_sample_area_reference(c["p"], c["lists"], shape, bshape, cen, np.diag([4.0, 4.0]), 4, c["cfg"])
    pix = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) + 0.5 for s in shape], indexing="ij"), axis=-1).reshape(-1, 2)
    _, bid, u = point_mapping(pix, shape, bshape)
    v = shared_points_grad_reference(c["p"], c["lists"], u, bid, shape, c["cfg"])["v"].reshape(shape + (c["C"],))
    pad = np.zeros((4 * E[0], 4 * E[1], c["C"]), np.float32)
    ins = np.zeros((4 * E[0], 4 * E[1]), bool)
    pad[:shape[0], :shape[1]], ins[:shape[0], :shape[1]] = v, True
    box = lambda a: a.reshape((E[0], 4, E[1], 4) + a.shape[2:]).swapaxes(1, 2).reshape((E[0] * E[1], 16) + a.shape[2:])
    mean, cnt = masked_mean(box(pad), box(ins), np.float32)                    # row-major over the 4 x 4 box
    assert np.array_equal(r["mean"], mean) and np.array_equal(r["count"], cnt)
    straddle = np.array([len(np.unique(b[m])) for b, m in zip(r["tap_batch"], r["inside"])])
    if i == 4:
        assert (cnt < 16).any() and (cnt > 0).all() and straddle.max() == 4
    else:
        assert (cnt == 16).all() and straddle.max() == 1


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_loose_cap_and_float32_error_of_the_restatement(i):
    c = case(i)
    ref, ref64 = area_reference(i)
    loose = loose_of(ref, ref64)                                               # asserts the cap
    F, taps = rotated_footprint(i)
    nt = int(np.prod(taps))
    assert ref["taps"].shape == (c["pts"].shape[0], nt, len(c["shape"])) and np.array_equal(ref["count"], ref64["count"])
    part = (ref["count"] > 0) & (ref["count"] < nt)
    meets = np.array([len(np.unique(b[m])) for b, m in zip(ref["tap_batch"], ref["inside"])])
    e32 = np.abs(ref["mean"].astype(np.float64) - ref64["mean"])[~loose].max()
    print(f"{CASE_IDS[i]}: loose share {loose.mean():.2e}, cells with some taps outside {part.mean():.3f}, cells in more than "
          f"one batch {(meets > 1).mean():.3f} (up to {meets.max()}), e32 {e32:.2e}")
    assert part.any() and (meets > 1).any() and 0 < e32 < 1e-5
    out = ref["batch"] < 0
    assert out.any() and (ref["count"][out] > 0).any()                          # a centre outside with taps inside


# ---------------------------------------------------------------------------------------------------------------
# the facade through the oracle engine
# ---------------------------------------------------------------------------------------------------------------
def _make(img, bs, kpd, factory=OracleSharedSampleAreaEngine, **kw):
    s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
                   engine_factory=factory, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


@pytest.fixture(scope="module")
def fitted():
    s = _make(_image((48, 64), C=3, seed=6), (16, 16), (6, 8), use_yuv=True)
    s.train(4, val_iter=2, ukl_iter=2)
    return s


def _rotation(deg, zoom, E, L):
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    M = np.array([[c, -s], [s, c]])
    return np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)


def test_shared_smoe_has_the_method_and_no_aliases():
    assert hasattr(SharedSmoe, "eval_points_area")
    for name in ("sample_area", "sample", "render_view", "render_warp", "sample_grad", "render_warp_grad"):
        assert not hasattr(SharedSmoe, name)
    from steered_mixture_of_experts_amd.smoe import Smoe
    assert Smoe._taps_arg is SharedSmoe._taps_arg                               # one statement of the taps argument


def _engine_call(s, pts, F, taps, **kw):
    """the engine call eval_points_area makes, by hand"""
    eng = s._engine
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2)))
    return eng.sample_area(s._params, s._render_lists(False), t, F, list(taps), **kw)


def test_eval_points_area(fitted):
    s = fitted
    A = _rotation(17, 0.25, (12, 20), (48, 64))
    pts, F = blk.warp_points(A, (12, 20)), A[:, :2]
    img, mean, cnt = s.eval_points_area(pts, F, taps=(3, 3), want_mean=True, want_count=True)
    assert img.shape == (12, 20, 3) and mean.shape == (12, 20, 3) and cnt.shape == (12, 20) and cnt.dtype == np.uint8
    want = _engine_call(s, pts, F, (3, 3), want_mean=True, want_count=True)
    assert np.array_equal(img.reshape(-1, 3), want[0].numpy()) and np.array_equal(mean.reshape(-1, 3), want[1].numpy())
    assert np.array_equal(cnt.reshape(-1), want[2].numpy()) and cnt.max() == 9 and cnt.min() < 9
    assert np.array_equal(s.eval_points_area(pts, F), s.eval_points_area(pts, F, taps=blk.footprint_taps(F)))      # "auto"
    u8 = s.eval_points_area(pts, F, taps=3, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(img * 255).astype(np.uint8))
    dev = s.eval_points_area(torch.from_numpy(pts), F, taps=3, to_host=False, want_mean=True)
    assert torch.is_tensor(dev[0]) and torch.is_tensor(dev[1]) and np.array_equal(dev[1].numpy(), mean)
    assert np.array_equal(s.eval_points_area(pts, F, taps=1), s.eval_points(pts))                                 # one tap
    assert s.eval_points_area(pts, F, taps=3, use_lists=False).shape == img.shape
    assert s.eval_points_area(np.zeros((0, 2), np.float32), F, taps=2).shape == (0, 3)
    # the mean of the taps' point values, by hand: eval_points_grad's values at blocks.area_taps
    t = blk.area_taps(pts.reshape(-1, 2), F, (3, 3))
    _, V = s.eval_points_grad(t, want_values=True)
    inside = blk.point_blocks(t, (48, 64), [1, 1], (48, 64))[0]
    m, n = masked_mean(V, inside, np.float32)
    assert np.array_equal(mean.reshape(-1, 3), m) and np.array_equal(cnt.reshape(-1), n)
    out = s.eval_points_area(np.array([[-30.0, 10.0], [np.nan, 5.0]], np.float32), F, taps=3, want_mean=True, want_count=True)
    assert (out[0] == 0).all() and (out[1] == 0).all() and (out[2] == 0).all()
    for kw in [dict(points=pts[..., :1]), dict(footprint=F[:1]), dict(footprint=F * np.nan), dict(taps=(3, 3, 3)), dict(taps=0),
               dict(taps=17), dict(taps=(9, 8)), dict(taps="many"), dict(dtype=np.float64)]:
        args = dict(points=pts, footprint=F, taps=(3, 3))
        args.update(kw)
        with pytest.raises(ValueError):
            s.eval_points_area(**args)
    with pytest.raises(TypeError):
        s.eval_points_area(pts, F, taps=3, blend=2)


def test_eval_warp_and_eval_view_with_taps(fitted):
    s = fitted
    A = _rotation(-31, 0.5, (20, 24), (48, 64))
    pts = blk.warp_points(A, (20, 24))
    plain = s.eval_warp(A, (20, 24))
    assert np.array_equal(s.eval_warp(A, (20, 24), taps=None), plain) and np.array_equal(s.eval_warp(A, (20, 24), taps=1), plain)
    assert np.array_equal(s.eval_warp(A, (20, 24), taps=(1, 1)), plain) and np.array_equal(plain, s.eval_points(pts))
    pa, ia = s.eval_warp(A, (20, 24), taps=1, want_argmax=True)                # all ones: today's path, argmax and all
    assert np.array_equal(pa, plain) and ia.shape == (20, 24)
    w = s.eval_warp(A, (20, 24), taps=3)
    assert w.shape == (20, 24, 3) and not np.array_equal(w, plain)
    assert np.array_equal(w.reshape(-1, 3), _engine_call(s, pts, A[:, :2], (3, 3)).numpy())                       # the engine's bits
    assert np.array_equal(s.eval_warp(A, (20, 24), taps="auto"), s.eval_points_area(pts, A[:, :2], taps=blk.footprint_taps(A[:, :2])))
    wm = s.eval_warp(A, (20, 24), taps=2, want_mean=True, dtype=np.uint8)
    assert wm[0].dtype == np.uint8 and wm[1].shape == (20, 24, 3)
    with pytest.raises(ValueError, match="want_argmax"):
        s.eval_warp(A, (20, 24), taps=2, want_argmax=True)
    # a 1/4 view
    win, E = [(4.0, 44.0), (8.0, 64.0)], (10, 14)
    one = s.eval_view(win, size=E)
    assert np.array_equal(s.eval_view(win, size=E, taps=None), one) and np.array_equal(s.eval_view(win, size=E, taps=(1, 1)), one)
    o1, i1 = s.eval_view(win, size=E, want_argmax=True)
    o2, i2 = s.eval_view(win, size=E, taps=1, want_argmax=True)
    assert np.array_equal(o1, one) and np.array_equal(o2, one) and np.array_equal(i1, i2)
    v = s.eval_view(win, size=E, taps="auto")
    assert v.shape == (10, 14, 3) and not np.array_equal(v, one) and np.array_equal(s.eval_view(win, size=E, taps=4), v)
    centres = np.stack(np.meshgrid(blk.view_positions(4.0, 44.0, 10), blk.view_positions(8.0, 64.0, 14), indexing="ij"), axis=-1)
    assert np.array_equal(v.reshape(-1, 3), _engine_call(s, centres, np.diag([4.0, 4.0]), (4, 4)).numpy())       # the engine's bits
    rec = s.render()                                                           # the lattice image: 0.5 / 255 from the values
    box = rec[4:44, 8:64].reshape(10, 4, 14, 4, 3).mean(axis=(1, 3))
    assert np.abs(v - box).max() <= 1.0 / 255 + 1e-6
    assert np.array_equal(s.eval_view(win, size=E, taps=(4, 4), dtype=np.uint8), np.rint(v * 255).astype(np.uint8))
    assert torch.is_tensor(s.eval_view(win, size=E, taps=(4, 4), to_host=False))
    for kw in [dict(taps=(4, 4), want_argmax=True), dict(taps=(4, 4, 4)), dict(taps=(9, 8)), dict(taps="some")]:
        with pytest.raises(ValueError):
            s.eval_view(win, size=E, **kw)


def test_an_engine_without_the_method_raises():
    s = _make(_image((32, 48), seed=5), (16, 16), (3, 4), factory=OracleSharedSampleGradEngine)
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area()")):
        s.eval_points_area(np.zeros((1, 2), np.float32), np.eye(2))
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area()")):
        s.eval_view(None, size=(4, 6), taps=2)
    assert s.eval_view(None, size=(4, 6), taps=1).shape == (4, 6, 1)            # all ones: eval_view's own path


# ---------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------
def test_smoe_shared_sample_area_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_shared_sample_area\s*\(\s*smoe_shared_handle\s+h,\s*const smoe_params\*\s+p,\s*const uint32_t\*\s+lists,"
                     r"\s*const float\*\s+points,\s*int64_t\s+num_points,\s*const float\*\s+footprint,\s*const int32_t\*\s+taps,"
                     r"\s*void\*\s+values,\s*int32_t\s+image_format,\s*float\*\s+mean,\s*uint8_t\*\s+count,\s*int32_t\*\s+batch,"
                     r"\s*void\*\s+stream\s*\)", src)
    assert hasattr(lib, "smoe_shared_sample_area") and "smoe_shared_sample_area" in _lib.EXPORTS
    assert len(lib.smoe_shared_sample_area.argtypes) == 13
    F = (C.c_float * 4)(1.0, 0.0, 0.0, 1.0)
    tp = (C.c_int32 * 2)(2, 2)
    rc = lib.smoe_shared_sample_area(None, None, None, None, 5, F, tp, None, 0, None, None, None, None)
    err = lib.smoe_last_error()
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_sample_area" in err and b"handle" in err
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
