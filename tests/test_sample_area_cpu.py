"""CPU tests of the area-averaged point decoder's host layer: ``blocks.area_taps`` / ``blocks.footprint_taps``, the numpy
restatement (tests/sample_area_engine.py) and the shares of its loose set, ``Smoe.sample_area`` / ``render_warp(taps=...)`` /
``render_view(taps=...)`` driven through the oracle-backed stand-in engine, the CLI's ``--taps``, and what the C entry point
checks without a handle."""
import os
import re

import numpy as np
import pytest
import torch

from sample_area_cases import LOOSE_CAP, area_reference, loose_of, rotated_footprint
from sample_area_engine import OracleSampleAreaEngine, masked_mean, sample_area_reference
from sample_engine import OracleSampleEngine
from sample_grad_cases import CASES, CASE_IDS, case_inputs, case_reference
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd import utils
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
from test_view_render_cpu import _image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the tap positions and the automatic tap counts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_taps_of_an_integer_box_are_the_pixel_centres(s):
    """F = diag(s), taps = s, centres s (i + 0.5): tap j of cell i is the centre of pixel s i + j, exactly"""
    for d, E in ((2, (5, 7)), (3, (3, 4, 2))):
        if s ** d > 64:
            continue
        idx = np.stack(np.meshgrid(*[np.arange(e) for e in E], indexing="ij"), axis=-1).reshape(-1, d)
        pts = (s * (idx + 0.5)).astype(np.float32)
        tp = blk.area_taps(pts, np.diag([float(s)] * d), [s] * d)
        jj = np.stack(np.meshgrid(*[np.arange(s)] * d, indexing="ij"), axis=-1).reshape(-1, d)
        want = (s * idx[:, None, :] + jj[None, :, :] + 0.5).astype(np.float32)
        assert tp.dtype == np.float32 and tp.shape == (len(pts), s ** d, d) and np.array_equal(tp, want)


def test_tap_arithmetic_and_order():
    F = np.array([[1.7, -0.4], [0.3, 2.9]], np.float32)
    pts = np.array([[10.3, 20.9], [0.1, 0.2], [np.nan, 1.0]], np.float32)
    tp = blk.area_taps(pts, F, (3, 2))
    assert tp.shape == (3, 6, 2)
    f32 = np.float32
    for t, (j0, j1) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]):      # last axis fastest
        o0, o1 = f32(2 * j0 + 1 - 3) / f32(6), f32(2 * j1 + 1 - 2) / f32(4)
        for l in range(2):
            want = f32(f32(pts[0, l] + f32(F[l, 0] * o0)) + f32(F[l, 1] * o1))           # product and sum rounded apart
            assert tp[0, t, l] == want
    assert np.isnan(tp[2, :, 0]).all() and not np.isnan(tp[2, :, 1]).any()
    assert np.array_equal(blk.area_taps(pts[:2], F, (1, 1))[:, 0], pts[:2])              # one tap is the point itself
    assert np.array_equal(blk.area_taps(pts[:2], F, 1)[:, 0], pts[:2])
    for bad in [dict(footprint=F[:1]), dict(footprint=F * np.inf), dict(taps=(0, 1)), dict(taps=(17, 1)), dict(taps=(9, 8)),
                dict(taps=(1, 2, 3))]:
        kw = dict(points=pts, footprint=F, taps=(2, 2))
        kw.update(bad)
        with pytest.raises(ValueError):
            blk.area_taps(**kw)


def test_view_positions_are_view_axis_positions_rounded_once():
    from fractions import Fraction
    for lo, hi, E in [(0.0, 44.0, 11), (4.0, 44.0, 10), (0.1, 74.9, 7), (3.3, 41.7, 13), (0.0, 75.0, 1), (1e-3, 2160.0, 271)]:
        x = blk.view_positions(lo, hi, E)
        assert x.dtype == np.float32 and x.shape == (E,)
        for i in (0, E // 2, E - 1):
            exact = Fraction(lo) + (Fraction(2 * i + 1) * (Fraction(hi) - Fraction(lo))) / (2 * E)
            near = np.float32(float(exact))
            cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
            best = min(cands, key=lambda c: abs(Fraction(float(c)) - exact))
            assert abs(Fraction(float(x[i])) - exact) == abs(Fraction(float(best)) - exact)
        # the block and block-unit coordinate of view_axis at the same sample: the same position
        first, blocks, start, coords = blk.view_axis(16, 5, 75, lo, hi, E) if hi <= 75 else blk.view_axis(16, 135, 2160, lo, hi, E)
        g = first + np.searchsorted(start, np.arange(E), side="right") - 1
        assert np.abs((g * 16 + coords.astype(np.float64) * 15 + 0.5) - x).max() <= 2e-4
    assert np.array_equal(blk.view_positions(4.0, 44.0, 10), (4 + 4 * (np.arange(10) + 0.5)).astype(np.float32))
    with pytest.raises(ValueError):
        blk.view_positions(0.0, 1.0, 0)


def test_footprint_taps_and_its_caps():
    ft = blk.footprint_taps
    assert ft(np.diag([8.0, 8.0])) == (8, 8) and ft(np.diag([2.0, 2.0])) == (2, 2) and ft(np.diag([0.3, 1.0])) == (1, 1)
    assert ft(np.diag([2.5, 1.01])) == (3, 2) and ft([[0.0, -3.2], [4.0, 0.0]]) == (4, 4)
    assert ft(np.diag([40.0, 1.0])) == (16, 1) and ft(np.diag([4.0, 4.0, 4.0])) == (4, 4, 4)
    assert ft(np.diag([9.0, 9.0])) == (8, 8)                       # 81 -> 72 -> 64: the largest entry, the first of equals
    assert ft(np.diag([16.0, 5.0])) == (12, 5) and ft(np.diag([5.0, 5.0, 5.0])) == (4, 4, 4)
    c, s = 3 * np.cos(np.deg2rad(17)), 3 * np.sin(np.deg2rad(17))
    assert ft([[c, -s], [s, c]]) == (3, 3)
    for tp in (ft(np.diag([100.0, 100.0, 100.0])), ft(np.diag([16.0, 16.0]))):
        assert int(np.prod(tp)) <= 64 and max(tp) <= 16 and min(tp) >= 1
    for bad in ([[1.0, np.nan], [0.0, 1.0]], [1.0, 2.0], np.zeros((2, 3))):
        with pytest.raises(ValueError):
            ft(bad)


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", [0, 3, 4], ids=[CASE_IDS[0], CASE_IDS[3], CASE_IDS[4]])
def test_one_tap_is_the_point_value(i, blended):
    c = case_inputs(i, blended)
    F, _ = rotated_footprint(i)
    for T, ref in zip((np.float32, np.float64), case_reference(i, blended)):
        r = sample_area_reference(c["p"], c["active"], c["shape"], c["grid"], c["length"], c["pts"], F, [1] * len(c["shape"]),
                                  c["beta"], c["cfg"], T)
        assert r["mean"].dtype == T and np.array_equal(r["mean"], ref["v"]) and np.array_equal(r["block"], ref["block"])
        assert np.array_equal(r["count"], ref["inside"].astype(np.int64)) and np.array_equal(r["loose"], ref["loose"])


def test_the_mean_leaves_outside_taps_out_and_keeps_the_order():
    """a self-check of the restatement's own helper (tests/sample_area_engine.py: masked_mean), not of the product: the
    reference the other tests compare against sums in the stated order and leaves outside taps out"""
    v = np.array([[[1.0], [1e-8], [3.0], [5.0]], [[2.0], [4.0], [6.0], [8.0]], [[1.0], [1.0], [1.0], [1.0]]], np.float32)
    inside = np.array([[True, True, False, True], [True, True, True, True], [False, False, False, False]])
    mean, cnt = masked_mean(v, inside, np.float32)
    f32 = np.float32
    assert mean.dtype == np.float32 and list(cnt) == [3, 4, 0]
    assert mean[0, 0] == f32(f32(f32(f32(0) + f32(1.0)) + f32(1e-8)) + f32(5.0)) / f32(3) and mean[1, 0] == 5.0 and mean[2, 0] == 0.0


@pytest.mark.parametrize("blended", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_loose_share_of_the_rotated_footprints(i, blended):
    """the condition the GPU parity test puts on its inputs, on the restatement alone"""
    ref, ref64 = area_reference(i, blended)
    covered = ref64["count"] > 0
    partial = covered & (ref64["count"] < ref64["inside"].shape[1])
    loose = loose_of(ref, ref64)
    e32 = np.abs(ref["mean"].astype(np.float64) - ref64["mean"])[covered & ~loose].max()
    print(f"covered {covered.sum()} of {covered.size}, partially {partial.sum()}, loose share of the covered "
          f"{loose[covered].mean():.2e}, float32 vs float64 outside the loose set {e32:.2e}")
    assert np.array_equal(ref["count"], ref64["count"]) and np.array_equal(ref["block"], ref64["block"])
    assert partial.sum() >= 10 and covered.mean() > 0.5
    assert not loose[~covered].any() and loose[covered].mean() <= LOOSE_CAP
    assert 0 < e32 < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# the facade on the CPU engine
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    b = blk.synthetic_blocks(15, (16, 16), 3, 99)
    img = blk.blocks_to_image(b, (48, 80), (16, 16))[:44, :75]
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True,
             engine_factory=OracleSampleAreaEngine)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(3, val_iter=3)
    return s


def _rotation(deg, zoom, E, L):
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    M = np.array([[c, -s], [s, c]])
    return np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)


def test_facade_shapes_and_options(fitted):
    s = fitted
    A = _rotation(17, 1 / 3, (12, 20), (44, 75))
    F = A[:, :2]
    pts = blk.warp_points(A, (12, 20))
    img = s.sample_area(pts, F, taps=(3, 3))
    assert img.shape == (12, 20, 3) and img.dtype == np.float32 and img.max() > 0
    assert np.array_equal(s.sample_area(pts, F), img)                                          # auto: 3 x 3 here
    assert np.array_equal(s.sample_area(pts, F, taps="auto"), img) and np.array_equal(s.sample_area(pts, F, taps=3), img)
    assert s.sample_area(pts.reshape(-1, 2), F).shape == (240, 3) and s.sample_area(pts[2, 3], F).shape == (3,)
    assert s.sample_area(np.zeros((0, 2), np.float32), F).shape == (0, 3)
    u8 = s.sample_area(pts, F, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(img * 255).astype(np.uint8))
    v, mean, cnt = s.sample_area(pts, F, want_mean=True, want_count=True)
    assert np.array_equal(v, img) and mean.shape == (12, 20, 3) and mean.dtype == np.float32 and cnt.shape == (12, 20) and cnt.dtype == np.uint8
    assert cnt.max() == 9 and cnt.min() < 9 and np.abs(mean - v).max() <= 0.5 / 255 + 1e-6
    v2, c2 = s.sample_area(pts, F, want_count=True)
    assert np.array_equal(v2, img) and np.array_equal(c2, cnt)
    dev = s.sample_area(torch.from_numpy(pts), F, to_host=False, want_mean=True)              # tensors in, tensors out
    assert torch.is_tensor(dev[0]) and torch.is_tensor(dev[1]) and np.array_equal(dev[1].numpy(), mean)
    assert not np.array_equal(s.sample_area(pts, F, blend=2), img)
    assert not np.array_equal(s.sample_area(pts, F, taps=1), img)
    assert np.array_equal(s.sample_area(pts, F, taps=1), s.sample(pts))                        # one tap: the point
    assert np.array_equal(s.sample_area(pts, F, taps=(1, 1), blend=2), s.sample(pts, blend=2))
    # the mean of the restatement's taps, by hand
    t = blk.area_taps(pts.reshape(-1, 2), F, (3, 3))
    inside = blk.point_blocks(t, (16, 16), s.grid, (44, 75))[0]
    assert np.array_equal(inside.sum(axis=1).reshape(12, 20), cnt)
    out = s.sample_area(np.array([[-30.0, 10.0], [np.nan, 5.0]], np.float32), F, want_mean=True, want_count=True)
    assert (out[0] == 0).all() and (out[1] == 0).all() and (out[2] == 0).all()
    for kw in [dict(points=pts[..., :1]), dict(footprint=F[:1]), dict(footprint=F * np.nan), dict(taps=(3, 3, 3)), dict(taps=0),
               dict(taps=17), dict(taps=(9, 8)), dict(taps="many"), dict(blend=9), dict(dtype=np.float64)]:
        args = dict(points=pts, footprint=F, taps=(3, 3))
        args.update(kw)
        with pytest.raises(ValueError):
            s.sample_area(**args)


def test_render_warp_and_render_view_with_taps(fitted):
    s = fitted
    A = _rotation(-31, 0.5, (20, 24), (44, 75))
    pts = blk.warp_points(A, (20, 24))
    plain = s.render_warp(A, (20, 24), blend=2)
    assert np.array_equal(s.render_warp(A, (20, 24), taps=None, blend=2), plain)              # today's path
    assert np.array_equal(s.render_warp(A, (20, 24), taps=1, blend=2), plain) and np.array_equal(s.render_warp(A, (20, 24), taps=(1, 1), blend=2), plain)
    w = s.render_warp(A, (20, 24), taps=(2, 2), blend=2)
    assert w.shape == (20, 24, 3) and np.array_equal(w, s.sample_area(pts, A[:, :2], taps=(2, 2), blend=2)) and not np.array_equal(w, plain)
    assert np.array_equal(s.render_warp(A, (20, 24), taps="auto"), s.sample_area(pts, A[:, :2], taps=blk.footprint_taps(A[:, :2])))
    wm = s.render_warp(A, (20, 24), taps=2, want_mean=True, dtype=np.uint8)
    assert wm[0].dtype == np.uint8 and wm[1].shape == (20, 24, 3)
    with pytest.raises(TypeError):
        s.render_warp(A, (20, 24), taps=2, want_argmax=True)
    # a 1/4 view: the lattice of the 4 x 4 means of the pixel centres
    win, E = [(4.0, 44.0), (8.0, 72.0)], (10, 16)
    one = s.render_view(win, size=E)
    assert np.array_equal(s.render_view(win, size=E, taps=None), one) and np.array_equal(s.render_view(win, size=E, taps=(1, 1)), one)
    v = s.render_view(win, size=E, taps=(4, 4))
    assert v.shape == (10, 16, 3) and not np.array_equal(v, one)
    assert np.array_equal(s.render_view(win, size=E, taps="auto"), v) and np.array_equal(s.render_view(win, size=E, taps=4), v)
    centres = np.stack(np.meshgrid(4 + 4 * (np.arange(10) + 0.5), 8 + 4 * (np.arange(16) + 0.5), indexing="ij"), axis=-1).astype(np.float32)
    assert np.array_equal(v, s.sample_area(centres, np.diag([4.0, 4.0]), taps=(4, 4)))
    rec = s.render()                                                                           # the lattice image: 0.5 / 255 from the values
    box = rec[4:44, 8:72].reshape(10, 4, 16, 4, 3).mean(axis=(1, 3))
    assert np.abs(v - box).max() <= 1.0 / 255 + 1e-6
    assert np.array_equal(s.render_view(win, size=E, taps=(4, 4), dtype=np.uint8), np.rint(v * 255).astype(np.uint8))
    assert torch.is_tensor(s.render_view(win, size=E, taps=(4, 4), to_host=False))
    for kw in [dict(taps=(4, 4), want_argmax=True), dict(taps=(4, 4, 4)), dict(taps=(9, 8)), dict(taps="some")]:
        with pytest.raises(ValueError):
            s.render_view(win, size=E, **kw)


def test_an_engine_without_the_method_raises():
    s = Smoe(_image(32, 48), train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True,
             engine_factory=OracleSampleEngine)
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area()")):
        s.sample_area(np.zeros((1, 2), np.float32), np.eye(2))
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area()")):
        s.render_view(None, size=(4, 6), taps=2)
    assert s.render_view(None, size=(4, 6), taps=1).shape == (4, 6, 1)                          # all ones: render_view's own path


# ---------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cli_taps(tmp_path):
    import steered_mixture_of_experts_amd.smoe as smod
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--window", "0", "32", "0", "48", "--size", "8", "12", "--taps", "4", "4"])
    assert a.taps == ["4", "4"] and rec._taps_option(a.taps) == [4, 4]
    assert rec._taps_option(rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--taps", "auto"]).taps) == "auto"
    assert rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z"]).taps is None
    img = _image(32, 48)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True,
             engine_factory=OracleSampleAreaEngine)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig_factory = smod._default_engine_factory
    smod._default_engine_factory = lambda cfg, device: OracleSampleAreaEngine(cfg, device)
    try:
        out, im = str(tmp_path / "out"), str(tmp_path / "img.npy")
        v, _, _ = rec.main(im, out, mp, window=[0.0, 32.0, 0.0, 48.0], size=[8, 12], taps=["4", "4"])
        assert v.shape == (8, 12, 1) and np.array_equal(v, s.render_view(None, size=(8, 12), taps=(4, 4)))
        assert np.load(out + "/2_reconstruction_view8x12_taps4x4.npy").shape == (8, 12, 1)
        v, _, _ = rec.main(im, out, mp, size=[8, 12], taps=["auto"], blend=[2.0])
        assert np.array_equal(v, s.render_view(None, size=(8, 12), taps=(4, 4), blend=2))
        assert os.path.exists(out + "/2_reconstruction_view8x12_tapsauto_blend2.npy")
        A = [3.0, 0.0, 1.0, 0.0, 3.0, 2.0]
        v, _, _ = rec.main(im, out, mp, affine=A, size=[10, 15], taps=["3"])
        assert np.array_equal(v, s.render_warp(np.array(A).reshape(2, 3), (10, 15), taps=3))
        assert os.path.exists(out + "/2_reconstruction_warp10x15_taps3.npy")
        for kw, word in [(dict(taps=["4"]), "--affine or --window"), (dict(taps=["4"], scale=[0.5]), "--affine or --window"),
                         (dict(taps=["4"], blend=[2.0]), "--affine or --window"), (dict(taps=["four"], size=[8, 12]), "--taps takes"),
                         (dict(taps=["4", "4", "4"], size=[8, 12]), "taps"), (dict(taps=["17"], size=[8, 12]), "taps"),
                         (dict(taps=["9", "8"], size=[8, 12]), "64")]:
            with pytest.raises(ValueError, match=word):
                rec.main(im, out, mp, **kw)
    finally:
        smod._default_engine_factory = orig_factory


def test_cli_taps_refuses_whole_image_models(tmp_path):
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    from shared_render_engine import OracleSharedRenderEngine
    from steered_mixture_of_experts_amd.smoe import SharedSmoe
    img = _image(32, 32, seed=4)
    s = SharedSmoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], engine_factory=OracleSharedRenderEngine)
    assert not hasattr(s, "sample_area")
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_0.pkl")
    utils.save_model(s, mp)
    with pytest.raises(ValueError, match="--taps needs a per-block model"):
        rec.main(str(tmp_path / "img.npy"), str(tmp_path / "out"), mp, size=[8, 8], taps=["2"])


# ---------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------
def test_smoe_sample_area_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_sample_area\s*\(", src)
    assert re.search(r"const float\*\s+footprint,\s*const int32_t\*\s+taps,\s*const float\s+blend\[3\],\s*void\*\s+values,\s*int32_t\s+image_format,"
                     r"\s*float\*\s+mean,\s*uint8_t\*\s+count,\s*int32_t\*\s+block,\s*void\*\s+stream", src)
    assert hasattr(lib, "smoe_sample_area") and "smoe_sample_area" in _lib.EXPORTS
    F = (C.c_float * 4)(1.0, 0.0, 0.0, 1.0)
    tp = (C.c_int32 * 2)(2, 2)
    rc = lib.smoe_sample_area(None, None, None, None, None, None, 5, F, tp, None, None, 0, None, None, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_sample_area" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
