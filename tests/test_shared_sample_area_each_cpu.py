"""CPU tests of the area-averaged decoder of whole-image models with per-point footprints: the inputs of the GPU tests
(tests/shared_sample_area_each_cases.py), the stand-in engine (tests/shared_sample_area_each_engine.py: the restatement of
smoe_shared_sample_area per distinct (footprint, taps) pair plus the void rule), ``SharedSmoe.eval_points_area_each`` /
``eval_projective`` / ``eval_map`` driven through it, and what the C entry point checks without a handle."""
import os
import re

import numpy as np
import pytest
import torch

from sample_area_engine import masked_mean
from shared_sample_area_cases import rotated_footprint
from shared_sample_area_each_cases import CASE_IDS, SSE_POINTS, SSE_TILE, model, tilt_inputs, tilt_matrix
from shared_sample_area_each_engine import OracleSharedSampleAreaEachEngine, shared_sample_area_each_reference
from shared_sample_area_engine import OracleSharedSampleAreaEngine, shared_sample_area_reference
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe, Smoe
from test_shared_render_cpu import _image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the inputs and the stand-in
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5), ids=CASE_IDS[:5])
def test_the_tilt_meets_its_conditions(i):
    t = tilt_inputs(i)                                                          # asserts them
    d = t["pts"].shape[1]
    assert t["E"] == tuple(tilt_matrix(i)[1]) and len(t["pts"]) == int(np.prod(t["E"])) and 1900 <= len(t["pts"]) <= 4800
    meets = np.array([len(np.unique(b[b >= 0])) for b in t["tap_batch"]])
    assert meets.max() >= 2 and 0.005 < (meets >= 2).mean() < 0.2
    runs = np.concatenate([t["ntap"], np.zeros(-len(t["ntap"]) % SSE_POINTS, np.int64)]).reshape(-1, SSE_POINTS).sum(axis=1)
    assert (runs > SSE_TILE[d]).sum() >= 5 and runs.max() <= 64 * SSE_POINTS


@pytest.mark.parametrize("i", [0, 3], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_the_stand_in_is_the_area_restatement_per_point(i):
    c = model(i)
    d = len(c["shape"])
    pts = np.ascontiguousarray(c["pts"][::7][:300])
    N = len(pts)
    F, taps = rotated_footprint(i)
    cfgs = [(F, tuple(taps)), (np.diag([2.0] * d).astype(np.float32), (2,) * d), ((np.float32(0.5) * F).astype(np.float32), (1,) * d)]
    foot = np.stack([cfgs[k % 3][0] for k in range(N)]).astype(np.float32)
    tp = np.array([cfgs[k % 3][1] for k in range(N)], np.uint8)
    tp[5], tp[6, 0], foot[7, 0, 1] = 0, 17, np.nan                              # three void points
    r = shared_sample_area_each_reference(c["p"], c["lists"], c["shape"], c["bshape"], pts, foot, tp, c["cfg"])
    assert r["void"].sum() == 3 and not r["mean"][r["void"]].any() and not r["count"][r["void"]].any() and r["mean"].any()
    for k, (Fk, tk) in enumerate(cfgs):
        w = shared_sample_area_reference(c["p"], c["lists"], c["shape"], c["bshape"], pts[k::3], Fk, tk, c["cfg"])
        keep = ~r["void"][k::3]
        assert np.array_equal(r["mean"][k::3][keep], w["mean"][keep]) and np.array_equal(r["count"][k::3][keep], w["count"][keep])
        assert np.array_equal(r["batch"][k::3], w["batch"])                     # void points keep the centre's batch
    # and the composition on blocks.area_taps_each: the ordered mean of the taps' values
    t, slot = blk.area_taps_each(pts, foot, tp)
    one = shared_sample_area_reference(c["p"], c["lists"], c["shape"], c["bshape"], t.reshape(-1, d), np.eye(d), 1, c["cfg"])
    inside = (one["count"].reshape(N, -1) > 0) & slot
    m, n = masked_mean(one["mean"].reshape(N, blk.AREA_TAPS, -1), inside, np.float32)
    assert np.array_equal(m, r["mean"]) and np.array_equal(n, r["count"])


# ---------------------------------------------------------------------------------------------------------------
# the facade through the oracle engine
# ---------------------------------------------------------------------------------------------------------------
def _make(img, bs, kpd, factory=OracleSharedSampleAreaEachEngine, **kw):
    s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
                   engine_factory=factory, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


@pytest.fixture(scope="module")
def fitted():
    s = _make(_image((48, 64), C=3, seed=6), (16, 16), (6, 8), use_yuv=True)
    s.train(4, val_iter=2, ukl_iter=2)
    return s


def test_shared_smoe_has_the_methods_and_no_aliases():
    for name in ("eval_points_area_each", "eval_projective", "eval_map"):
        assert callable(getattr(SharedSmoe, name))
    for name in ("sample_area_each", "render_projective", "render_map", "sample_area", "sample", "render_view", "render_warp",
                 "sample_grad", "render_warp_grad"):
        assert not hasattr(SharedSmoe, name)
    assert Smoe._taps_each_arg is SharedSmoe._taps_each_arg and Smoe._ones_taps is SharedSmoe._ones_taps   # one statement each
    from steered_mixture_of_experts_amd.engine import SharedEngine
    assert callable(SharedEngine.sample_area_each)


def _tilt(E, L):
    M = np.array([[2.5, -1.0], [1.0, 2.75]])
    A = np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)
    H = np.concatenate([A, [[0.0, 0.0, 1.0]]], axis=0)
    Ht = H.copy()
    Ht[2, 0] = -1.0 / (0.9 * E[0])
    Ht[:2, :2] += np.outer(np.asarray(L) / 2, Ht[2, :2])
    return A, H, Ht


def test_eval_points_area_each(fitted):
    s = fitted
    E = (12, 16)
    A, H, Ht = _tilt(E, (48, 64))
    pts, foot, valid = blk.projective_points(Ht, E)
    taps = blk.footprint_taps_each(foot.reshape(-1, 2, 2))
    img, mean, cnt = s.eval_points_area_each(pts, foot, want_mean=True, want_count=True)
    assert img.shape == (12, 16, 3) and mean.shape == (12, 16, 3) and cnt.shape == (12, 16) and cnt.dtype == np.uint8
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    want = s._engine.sample_area_each(s._params, s._render_lists(False), t(pts.reshape(-1, 2)), t(foot.reshape(-1, 2, 2)), t(taps),
                                      want_mean=True, want_count=True)
    assert np.array_equal(img.reshape(-1, 3), want[0].numpy()) and np.array_equal(mean.reshape(-1, 3), want[1].numpy())
    assert np.array_equal(cnt.reshape(-1), want[2].numpy()) and cnt.max() > 9 and len(np.unique(taps, axis=0)) > 4
    assert (~valid).sum() == 16 and not img[~valid].any() and not cnt[~valid].any()
    # the taps argument: "auto", an array, one tuple, one number
    assert np.array_equal(s.eval_points_area_each(pts, foot, taps=taps.reshape(12, 16, 2)), img)
    assert np.array_equal(s.eval_points_area_each(pts, foot, taps=torch.from_numpy(taps.reshape(12, 16, 2).astype(np.int64))), img)
    fixed = s.eval_points_area_each(pts, foot, taps=(3, 2))
    assert np.array_equal(fixed, s.eval_points_area_each(pts, foot, taps=np.broadcast_to(np.array([3, 2]), (12, 16, 2))))
    assert np.array_equal(s.eval_points_area_each(pts, foot, taps=2), s.eval_points_area_each(pts, foot, taps=(2, 2)))
    assert np.array_equal(s.eval_points_area_each(pts, foot, taps=1), s.eval_points(pts))                         # one tap
    # one footprint for all: eval_points_area
    Mb = np.broadcast_to(np.float32(A[:, :2]), (12, 16, 2, 2))
    wp = blk.warp_points(A, E)
    assert np.array_equal(s.eval_points_area_each(wp, Mb, taps=(3, 3)), s.eval_points_area(wp, A[:, :2], taps=(3, 3)))
    u8 = s.eval_points_area_each(pts, foot, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(img * 255).astype(np.uint8))
    dev = s.eval_points_area_each(torch.from_numpy(pts), torch.from_numpy(foot), to_host=False, want_mean=True)
    assert torch.is_tensor(dev[0]) and torch.is_tensor(dev[1]) and np.array_equal(dev[1].numpy(), mean)
    assert s.eval_points_area_each(pts, foot, use_lists=False).shape == img.shape
    assert s.eval_points_area_each(np.zeros((0, 2), np.float32), np.zeros((0, 2, 2), np.float32)).shape == (0, 3)
    # void points through the facade: a count outside 0 .. 255 becomes 0
    tv = taps.reshape(12, 16, 2).astype(np.int64)
    tv[0, 0], tv[0, 1], tv[0, 2] = (300, 1), (-1, 1), (16, 5)
    v = s.eval_points_area_each(pts, foot, taps=tv, want_count=True)
    assert not v[0][0, :3].any() and not v[1][0, :3].any() and np.array_equal(v[0][1:], img[1:])
    for kw in [dict(points=pts[..., :1]), dict(footprints=foot[:1]), dict(footprints=foot[..., :1]), dict(footprints="no"),
               dict(taps=(3, 3, 3)), dict(taps=0), dict(taps=17), dict(taps=(9, 8)), dict(taps="many"), dict(taps=taps),
               dict(taps=taps.reshape(12, 16, 2).astype(np.float32)), dict(dtype=np.float64)]:
        args = dict(points=pts, footprints=foot)
        args.update(kw)
        with pytest.raises(ValueError):
            s.eval_points_area_each(**args)
    with pytest.raises(TypeError):
        s.eval_points_area_each(pts, foot, blend=2)


def test_eval_projective_and_eval_map(fitted):
    s = fitted
    E = (12, 16)
    A, H, Ht = _tilt(E, (48, 64))
    wp = blk.warp_points(A, E)
    # an affine H is eval_warp(taps="auto"); taps None or all ones is eval_points
    assert np.array_equal(s.eval_projective(H, E), s.eval_warp(A, E, taps="auto"))
    assert not np.array_equal(s.eval_projective(H, E), s.eval_warp(A, E))
    plain = s.eval_points(wp)
    for tp in (None, 1, (1, 1)):
        assert np.array_equal(s.eval_projective(H, E, taps=tp), plain) and np.array_equal(s.eval_map(wp, taps=tp), plain)
    pa, ia = s.eval_projective(H, E, taps=None, want_argmax=True)              # eval_points' options then
    assert np.array_equal(pa, plain) and ia.shape == E
    pts, foot, _ = blk.projective_points(Ht, E)
    assert np.array_equal(s.eval_projective(Ht, E), s.eval_points_area_each(pts, foot))
    assert np.array_equal(s.eval_projective(Ht, E, taps=(2, 3)), s.eval_points_area_each(pts, foot, taps=(2, 3)))
    pm = s.eval_projective(Ht, E, want_mean=True, dtype=np.uint8)
    assert pm[0].dtype == np.uint8 and pm[1].shape == (12, 16, 3)
    # the map of the affine view: its footprints are M exactly (dyadic entries)
    assert np.array_equal(s.eval_map(wp), s.eval_warp(A, E, taps="auto"))
    assert torch.is_tensor(s.eval_map(torch.from_numpy(wp), to_host=False))
    q = (wp + 0.004 * (wp - 20.0) ** 2).astype(np.float32)
    assert np.array_equal(s.eval_map(q), s.eval_points_area_each(q, blk.map_footprints(q)))
    assert np.array_equal(s.eval_map(torch.from_numpy(q)), s.eval_map(q)) and not np.array_equal(s.eval_map(q), s.eval_points(q))
    for bad in (np.eye(3)[:2], np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="eval_projective"):
            s.eval_projective(bad, E)
    for bad in (wp.reshape(-1, 2), wp[..., :1], wp.astype(np.int64).astype(object)):
        with pytest.raises(ValueError, match="eval_map"):
            s.eval_map(bad)
    with pytest.raises(ValueError, match="eval_map"):
        s.eval_map(torch.from_numpy(wp).to(torch.int32))


def test_an_engine_without_the_method_raises():
    s = _make(_image((32, 48), seed=5), (16, 16), (3, 4), factory=OracleSharedSampleAreaEngine)
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area_each()")):
        s.eval_points_area_each(np.zeros((1, 2), np.float32), np.eye(2, dtype=np.float32)[None])
    H = np.array([[2.0, 0, 0], [0, 2.0, 0], [0, 0, 1.0]])
    with pytest.raises(NotImplementedError, match=re.escape("this engine has no sample_area_each()")):
        s.eval_projective(H, (4, 6))
    assert s.eval_projective(H, (4, 6), taps=1).shape == (4, 6, 1)              # all ones: eval_points' own path


# ---------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------
def test_smoe_shared_sample_area_each_is_declared_exported_and_checks_its_arguments():
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_shared_sample_area_each\s*\(\s*smoe_shared_handle\s+h,\s*const smoe_params\*\s+p,\s*const uint32_t\*\s+lists,"
                     r"\s*const float\*\s+points,\s*int64_t\s+num_points,\s*const float\*\s+footprints,\s*const uint8_t\*\s+taps,"
                     r"\s*void\*\s+values,\s*int32_t\s+image_format,\s*float\*\s+mean,\s*uint8_t\*\s+count,\s*int32_t\*\s+batch,"
                     r"\s*void\*\s+stream\s*\)", src)
    assert hasattr(lib, "smoe_shared_sample_area_each") and "smoe_shared_sample_area_each" in _lib.EXPORTS
    assert len(lib.smoe_shared_sample_area_each.argtypes) == 13
    rc = lib.smoe_shared_sample_area_each(None, None, None, None, 5, None, None, None, 0, None, None, None, None)
    err = lib.smoe_last_error()
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_sample_area_each" in err and b"handle" in err
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
