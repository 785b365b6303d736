"""CPU tests of the point decoder's host layer: ``blocks.point_blocks`` / ``blocks.warp_points``, the numpy restatement
(tests/sample_engine.py), ``Smoe.sample`` / ``Smoe.render_warp`` driven through the oracle-backed stand-in engine, the CLI's
``--affine``, two gloo ranks against one, and what the C entry point checks without a handle."""
import os
import pickle
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from sample_engine import OracleSampleEngine, sample_reference
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd import utils
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
from test_view_render_cpu import _free_port, _image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(img, bs=(16, 16), kpd=(2, 2), **kw):
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
             engine_factory=OracleSampleEngine, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


def _rotation(deg, zoom, E, L):
    """[M | t] of x = R(deg) / zoom (i + 0.5 - E / 2) + L / 2"""
    c, s = np.cos(np.deg2rad(deg)) / zoom, np.sin(np.deg2rad(deg)) / zoom
    M = np.array([[c, -s], [s, c]])
    return np.concatenate([M, (np.asarray(L) / 2 - M @ (np.asarray(E) / 2))[:, None]], axis=1)


# ---------------------------------------------------------------------------------------------------------------
# blocks.point_blocks, blocks.warp_points
# ---------------------------------------------------------------------------------------------------------------
def test_pixel_centres_sit_on_the_training_lattice():
    """u of q + 0.5 is entry q of render_axis(n, n) = linspace(0, 1, n), bit for bit, in every block up to offset 200"""
    for n in range(2, 130):
        grid = 201
        q = np.arange(grid * n, dtype=np.float64)
        pts = (q + 0.5).astype(np.float32)[:, None]
        assert np.array_equal(pts[:, 0].astype(np.float64), q + 0.5)           # grid * n < 2^23: the centres are exact
        inside, g, u = blk.point_blocks(pts, [n], [grid], [grid * n])
        assert inside.all() and np.array_equal(g[:, 0], q.astype(np.int64) // n)
        assert u.dtype == np.float32
        assert np.array_equal(u[:, 0].view(np.uint32), np.tile(blk.render_axis(n, n), grid).view(np.uint32)), n
    inside, g, u = blk.point_blocks(np.array([[0.5], [3.25]], np.float32), [1], [7], [7])
    assert inside.all() and np.array_equal(g[:, 0], [0, 3]) and (u == 0).all()


@pytest.mark.parametrize("n", [5, 7])
def test_block_ownership_is_exact_at_the_borders(n):
    grid = 2 ** 24 // n
    borders = np.unique(np.concatenate([np.arange(1, 4000), np.random.default_rng(n).integers(1, grid, size=4000), [grid - 1]])) * n
    b32 = borders.astype(np.float32)
    assert np.array_equal(b32.astype(np.int64), borders)                        # the products are exact in float32
    below, above = np.nextafter(b32, np.float32(0)), np.nextafter(b32, np.float32(np.inf))
    pts = np.concatenate([below, b32, above]).astype(np.float32)
    inside, g, u = blk.point_blocks(pts[:, None], [n], [grid], [grid * n])
    want = np.array([int(Fraction(float(x)) // n) for x in pts])
    assert inside.all() and np.array_equal(g[:, 0], want)
    assert np.array_equal(g[:len(borders), 0], borders // n - 1) and np.array_equal(g[len(borders):2 * len(borders), 0], borders // n)
    # (a correctly rounded quotient happens to land on the right side of these borders; the +-1 correction against the exact
    # products is what makes ownership independent of that)
    raw = np.floor(pts / np.float32(n)).astype(np.int64)
    print(f"n = {n}: floor(x / n) in float32 alone is off by one on {(raw != want).sum()} of {len(pts)} border points")
    # t = x - g n is exact and u is its one-rounding image
    t = np.array([Fraction(float(x)) - int(gg) * n for x, gg in zip(pts, g[:, 0])])
    assert all(0 <= v < n for v in t)
    uu = ((np.array([float(v) for v in t], np.float32) - np.float32(0.5)) / np.float32(n - 1)).astype(np.float32)
    assert np.array_equal(u[:, 0], uu)


def test_points_outside():
    pts = np.array([[np.nan, 3], [3, np.nan], [-1e-6, 3], [3, -0.0], [44, 3], [43.999, 74.999], [3, 75], [0, 0], [np.inf, 1],
                    [-np.inf, 1], [47.5, 3]], np.float32)
    inside, g, u = blk.point_blocks(pts, [16, 16], [3, 5], [44, 75])
    assert inside.tolist() == [False, False, False, True, False, True, False, True, False, False, False]
    assert (g[~inside] == 0).all() and (u[~inside] == 0).all()
    assert g[5].tolist() == [2, 4] and g[3].tolist() == [0, 0]
    shaped = blk.point_blocks(pts.reshape(1, 11, 2), [16, 16], [3, 5], [44, 75])
    assert shaped[0].shape == (1, 11) and shaped[1].shape == (1, 11, 2) and shaped[2].shape == (1, 11, 2)
    for bad in [dict(points=pts[:, :1]), dict(length=[49, 75]), dict(length=[0, 75]), dict(grid=[3])]:
        kw = dict(points=pts, block_shape=[16, 16], grid=[3, 5], length=[44, 75])
        kw.update(bad)
        with pytest.raises(ValueError):
            blk.point_blocks(**kw)
    with pytest.raises(ValueError):
        blk.point_blocks(pts[:, :1], [16], [2 ** 20 + 1], [16])                  # block origins would not be exact


def test_warp_points():
    w = blk.warp_points([[1, 0, 0], [0, 1, 0]], (3, 4))
    assert w.shape == (3, 4, 2) and w.dtype == np.float32
    assert np.array_equal(w[..., 0], np.broadcast_to(np.arange(3)[:, None] + 0.5, (3, 4)))
    assert np.array_equal(w[..., 1], np.broadcast_to(np.arange(4)[None, :] + 0.5, (3, 4)))
    A = np.array([[0.5, -0.25, 3.0], [0.125, 2.0, -1.0]])
    w = blk.warp_points(A, (5, 2))
    i = np.array([3.5, 1.5])
    assert np.array_equal(w[3, 1], (A[:, :2] @ i + A[:, 2]).astype(np.float32))
    w3 = blk.warp_points(np.concatenate([np.eye(3), [[1], [2], [3]]], axis=1), (2, 3, 4))
    assert w3.shape == (2, 3, 4, 3) and np.array_equal(w3[1, 2, 3], [2.5, 4.5, 6.5])
    for bad in [([[1, 0], [0, 1]], (3, 4)), ([[1, 0, 0], [0, 1, np.nan]], (3, 4)), ([[1, 0, 0], [0, 1, 0]], (3, 0)),
                ([[1, 0, 0], [0, 1, 0]], (3, 4, 5))]:
        with pytest.raises(ValueError):
            blk.warp_points(*bad)


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_on_a_view_grid_is_the_view_restatement():
    from oracle import smoe_oracle as o
    from view_render_engine import view_reference
    b = blk.synthetic_blocks(6, (16, 16), 1, 7)
    p = o.init_params(b, [2, 2])
    cfg = o.OracleConfig(block_shape=(16, 16), channels=1, kernels=4)
    act = np.random.default_rng(2).uniform(size=(6, 4)) < 0.8
    grid = (2, 3)
    pts = blk.warp_points([[1, 0, 0], [0, 1, 0]], (32, 48))
    ax = [blk.view_axis(16, g, 16 * g, 0, 16 * g, 16 * g) for g in grid]
    for beta in (None, 2.0):
        want = view_reference(p, act, [16, 16], list(grid), [a[0] for a in ax], [a[2] for a in ax], [a[3] for a in ax], beta, cfg)
        r = sample_reference(p, act, [16, 16], list(grid), [32, 48], pts, beta, cfg)
        for k in ("recon", "v", "wt0", "block", "banded", "near_tau", "nblocks"):
            assert np.array_equal(r[k].reshape(want[k].shape), want[k]), (beta, k)
        assert r["banded"].any() == (beta is not None)


# ---------------------------------------------------------------------------------------------------------------
# Smoe.sample, Smoe.render_warp
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    s = _make(_image(44, 75, C=3, seed=3), use_yuv=True)            # ragged: 3 x 5 blocks, 4 rows and 5 columns of padding
    s.train(3, val_iter=3)
    return s


IDENT = [[1, 0, 0], [0, 1, 0]]


def test_identity_warp_is_the_reconstruction_and_a_shift_its_crop(fitted):
    s = fitted
    recon = s.get_reconstruction()
    assert recon.shape == (44, 75, 3)
    out, ids = s.render_warp(IDENT, (44, 75), want_argmax=True)
    base, bids = s.render(want_argmax=True)
    assert out.dtype == np.float32 and np.array_equal(out, recon) and np.array_equal(out, base)
    assert ids.dtype == np.int64 and ids.shape == (44, 75) and np.array_equal(ids, bids) and (ids >= 0).any()
    crop = s.render_warp([[1, 0, 7], [0, 1, 20]], (30, 41))
    assert np.array_equal(crop, recon[7:37, 20:61])
    for blend in (2.0, (1, 2)):
        assert np.array_equal(s.render_warp([[1, 0, 7], [0, 1, 20]], (30, 41), blend=blend), s.render(blend=blend)[7:37, 20:61])
    assert not np.array_equal(s.render_warp(IDENT, (44, 75), blend=2), recon)
    # 2x: the cell centres of a 2x render
    assert np.array_equal(s.render_warp([[0.5, 0, 0], [0, 0.5, 0]], (88, 150)), s.render(scale=2))


def test_the_padding_of_a_ragged_image_is_outside(fitted):
    s = fitted
    out, ids = s.render_warp(IDENT, (48, 80), want_argmax=True)
    assert np.array_equal(out[:44, :75], s.get_reconstruction())
    assert (out[44:] == 0).all() and (out[:, 75:] == 0).all() and (ids[44:] == -1).all() and (ids[:, 75:] == -1).all()
    pts = np.array([[43.99, 74.99], [44.0, 10.0], [10.0, 75.0], [-0.01, 5.0], [np.nan, 5.0]], np.float32)
    v, i = s.sample(pts, want_argmax=True)
    assert (v[1:] == 0).all() and (i[1:] == -1).all() and v[0].any()
    assert (s.sample(pts, dtype=np.uint8)[1:] == 0).all()


def test_sample_shapes_types_and_bad_arguments(fitted):
    s = fitted
    A = _rotation(17, 1.7, (31, 29), (44, 75))
    pts = blk.warp_points(A, (31, 29))
    img, ids = s.render_warp(A, (31, 29), want_argmax=True, blend=2)
    v, i = s.sample(pts, want_argmax=True, blend=2)
    assert img.shape == (31, 29, 3) and np.array_equal(v, img) and np.array_equal(i, ids)
    assert not np.array_equal(img, s.render_warp(A, (31, 29)))
    assert s.sample(pts.reshape(-1, 2)).shape == (31 * 29, 3) and s.sample(pts[3, 4]).shape == (3,)
    assert s.sample(pts.reshape(31, 1, 29, 2)).shape == (31, 1, 29, 3) and s.sample(np.zeros((0, 2), np.float32)).shape == (0, 3)
    assert np.array_equal(s.sample(pts.reshape(-1, 2)[::-1].copy())[::-1], s.sample(pts).reshape(-1, 3))
    assert np.array_equal(s.sample(pts.astype(np.float64).tolist()), s.sample(pts))         # array-like
    u8 = s.sample(pts, dtype=np.uint8, blend=2)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(img * 255).astype(np.uint8))
    import torch
    dev, did = s.sample(torch.from_numpy(pts), to_host=False, want_argmax=True, blend=2)
    assert torch.is_tensor(dev) and torch.is_tensor(did) and did.dtype == torch.int64
    assert np.array_equal(dev.numpy(), img) and np.array_equal(did.numpy(), ids)
    # global ids: block index * K + local id of the own block
    inside, g, _ = blk.point_blocks(pts, [16, 16], [3, 5], [44, 75])
    own = g[..., 0] * 5 + g[..., 1]
    has = ids >= 0
    assert inside.all() and has.any() and np.array_equal(ids[has] // s.kernels, own[has])
    for kw in [dict(points=pts[..., :1]), dict(points=np.float32(1.0)), dict(points=pts, blend=9), dict(points=pts, blend=(1, 2, 3)),
               dict(points=pts, blend=float("nan")), dict(points=pts, dtype=np.float64)]:
        with pytest.raises(ValueError):
            s.sample(**kw)
    for bad in [(IDENT, (4,)), ([[1, 0], [0, 1]], (4, 4)), (IDENT, (0, 4))]:
        with pytest.raises(ValueError):
            s.render_warp(*bad)


def test_quantized_sample_is_the_quantised_render(fitted):
    from steered_mixture_of_experts_amd.quantizer import quantize_params, rescaler
    s = fitted
    s.qparams = quantize_params(s, s.get_params())
    s.rparams = rescaler(s, s.qparams)
    assert np.array_equal(s.render_warp(IDENT, (44, 75), quantized=True), s.render(quantized=True))


# ---------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cli_affine(tmp_path):
    import steered_mixture_of_experts_amd.smoe as smod
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--affine", "1", "0", "2.5", "0", "1", "-3", "--size", "30", "40"])
    assert a.affine == [1.0, 0.0, 2.5, 0.0, 1.0, -3.0] and a.size == [30, 40]
    assert rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z"]).affine is None
    img = _image(32, 48)
    s = _make(img)
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig_factory = smod._default_engine_factory
    smod._default_engine_factory = lambda cfg, device: OracleSampleEngine(cfg, device)
    try:
        out = str(tmp_path / "out")
        im = str(tmp_path / "img.npy")
        A = _rotation(17, 1.7, (20, 36), (32, 48))
        v, _, _ = rec.main(im, out, mp, affine=[float(x) for x in A.reshape(-1)], size=[20, 36], blend=[2.0])
        assert v.shape == (20, 36, 1) and np.array_equal(v, s.render_warp(A, (20, 36), blend=2))
        assert np.load(out + "/2_reconstruction_warp20x36_blend2.npy").shape == (20, 36, 1)
        v, _, _ = rec.main(im, out, mp, affine=[1, 0, 4, 0, 1, 8], size=[10, 30])
        assert np.array_equal(v, s.get_reconstruction()[4:14, 8:38])
        assert os.path.exists(out + "/2_reconstruction_warp10x30.npy")
        # positional compatibility: affine is the last parameter
        v2, _, _ = rec.main(im, out, mp, 1, (20, 18, 6, 10, 10), False, None, None, None, None, [10, 30], [1, 0, 4, 0, 1, 8])
        assert np.array_equal(v2, v)
        for kw in [dict(affine=[1, 0, 0, 0, 1, 0]), dict(affine=[1, 0, 0, 0, 1], size=[4, 4]), dict(affine=[1, 0, 0, 0, 1, 0], size=[4]),
                   dict(affine=[1, 0, 0, 0, 1, 0], size=[4, 4], window=[0.0, 4.0, 0.0, 4.0]),
                   dict(affine=[1, 0, 0, 0, 1, 0], size=[4, 4], frames=3), dict(affine=[1, 0, 0, 0, 1, 0], size=[4, 4], scale=[2.0])]:
            with pytest.raises(ValueError):
                rec.main(im, out, mp, **kw)
    finally:
        smod._default_engine_factory = orig_factory


def test_cli_affine_refuses_whole_image_models(tmp_path):
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    from shared_render_engine import OracleSharedRenderEngine
    from steered_mixture_of_experts_amd.smoe import SharedSmoe
    img = _image(32, 32, seed=4)
    s = SharedSmoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], engine_factory=OracleSharedRenderEngine)
    assert not hasattr(s, "sample") and not hasattr(s, "render_warp")
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_0.pkl")
    utils.save_model(s, mp)
    rec._shared_engine_factory = OracleSharedRenderEngine
    try:
        with pytest.raises(ValueError, match="whole-image"):
            rec.main(str(tmp_path / "img.npy"), str(tmp_path / "out"), mp, affine=[1, 0, 0, 0, 1, 0], size=[8, 8])
    finally:
        rec._shared_engine_factory = None


# ---------------------------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
from sample_engine import OracleSampleEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
ws = int(os.environ.get("WORLD_SIZE", "1"))
if ws > 1:
    dist.init_process_group(backend="gloo")
b = blk.synthetic_blocks(15, (16, 16), 1, 99)
img = blk.blocks_to_image(b, (48, 80), (16, 16))[:44, :75]
s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, engine_factory=OracleSampleEngine)
s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
s.train(3, val_iter=3)
c, sn = np.cos(np.deg2rad(17)) / 1.3, np.sin(np.deg2rad(17)) / 1.3
M = np.array([[c, -sn], [sn, c]])
A = np.concatenate([M, (np.array([22.0, 37.5]) - M @ np.array([25.0, 40.0]))[:, None]], axis=1)
warp, ids = s.render_warp(A, (50, 80), blend=(1, 2), want_argmax=True)
pts = blk.warp_points(A, (50, 80))
out = {"warp": warp, "ids": ids, "u8": s.sample(pts, blend=1.5, dtype=np.uint8), "plain": s.sample(pts),
       "ident": s.render_warp([[1, 0, 0], [0, 1, 0]], (44, 75)), "recon": s.get_reconstruction(), "span": (s.lo, s.hi)}
if ws == 1 or dist.get_rank() == 0:
    pickle.dump(out, open(sys.argv[2], "wb"))
if ws > 1:
    dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_sample_what_one_rank_samples(tmp_path):
    w = tmp_path / "worker.py"
    w.write_text(WORKER)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    one = str(tmp_path / "one.pkl")
    subprocess.check_call([sys.executable, str(w), ROOT, one], env=env, timeout=300)
    two = str(tmp_path / "two.pkl")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(w), ROOT, two],
                          env=env, timeout=600)
    a, b = pickle.load(open(one, "rb")), pickle.load(open(two, "rb"))
    assert a["span"] == (0, 15) and b["span"] == (0, 8)
    assert a["warp"].shape == (50, 80, 1) and not np.array_equal(a["warp"], a["plain"])
    assert np.array_equal(a["ident"], a["recon"])
    assert (a["ids"] == -1).any() and (a["ids"] >= 0).any()                   # the rotated view leaves the image
    for k in ("warp", "ids", "u8", "plain", "ident"):
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------
def test_smoe_sample_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_sample\s*\(", src) and re.search(r"const\s+float\*\s+points,\s*int64_t\s+num_points", src)
    assert re.search(r"int32_t\*\s+block,\s*void\*\s+stream", src)
    assert hasattr(lib, "smoe_sample") and "smoe_sample" in _lib.EXPORTS
    bl = (C.c_float * 3)(1.0, 1.0, 0.0)
    rc = lib.smoe_sample(None, None, None, None, None, None, 5, bl, None, 0, None, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_sample" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
