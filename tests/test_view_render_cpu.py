"""CPU tests of the viewport decoder's host layer: ``blocks.view_axis``, the numpy restatement for ragged runs
(tests/view_render_engine.py), ``Smoe.render_view`` driven through the oracle-backed stand-in engine, the CLI options, two
gloo ranks against one, and what the C entry point checks without a handle."""
import os
import pickle
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd import utils
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
from view_render_engine import OracleViewEngine, view_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(h, w, C=1, seed=0):
    gh, gw = -(-h // 16), -(-w // 16)
    b = blk.synthetic_blocks(gh * gw, (16, 16), C, seed)
    return blk.blocks_to_image(b, (gh * 16, gw * 16), (16, 16))[:h, :w]


def _make(img, bs=(16, 16), kpd=(2, 2), **kw):
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
             engine_factory=OracleViewEngine, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


# ---------------------------------------------------------------------------------------------------------------
# blocks.view_axis
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 7, 16, 32, 64])
def test_view_axis_reproduces_render_axis_on_aligned_grids(n):
    """whole-axis windows with E = grid * m: np.tile(render_axis(n, m), grid) bit for bit, start = arange(grid + 1) * m"""
    for m in list(range(1, 3 * n + 1)) + [8 * n]:
        tab = blk.render_axis(n, m)
        for grid in (1, 4, 135, 240):
            first, blocks, start, coords = blk.view_axis(n, grid, grid * n, 0, grid * n, grid * m)
            assert first == 0 and blocks == grid
            assert start.dtype == np.int32 and np.array_equal(start, np.arange(grid + 1) * m)
            assert coords.dtype == np.float32
            assert np.array_equal(coords.view(np.uint32), np.tile(tab, grid).view(np.uint32)), (n, m, grid)


def test_view_axis_crops_of_an_aligned_grid_give_the_crop():
    for n, m, grid, a, b in [(16, 32, 4, 10, 70), (16, 40, 3, 1, 119), (7, 11, 5, 3, 40), (64, 65, 4, 64, 131), (5, 5, 6, 4, 9),
                             (16, 16, 4, 17, 18), (16, 8, 4, 1, 30)]:
        full = np.tile(blk.render_axis(n, m), grid)
        lo, hi = a * n / m, b * n / m                             # sample a .. b - 1 of the aligned grid
        first, blocks, start, coords = blk.view_axis(n, grid, grid * n, lo, hi, b - a)
        assert np.array_equal(coords.view(np.uint32), full[a:b].view(np.uint32)), (n, m, a, b)
        owner = np.arange(a, b) // m
        assert first == owner[0] and blocks == owner[-1] - owner[0] + 1
        assert np.array_equal(first + np.repeat(np.arange(blocks), np.diff(start)), owner)


def test_view_axis_free_windows():
    rng = np.random.default_rng(3)
    for _ in range(60):
        n = int(rng.choice([2, 3, 7, 16, 32]))
        grid = int(rng.integers(1, 9))
        length = grid * n - int(rng.integers(0, n))               # a ragged image
        lo = float(rng.uniform(0, length - 0.5))
        hi = float(rng.uniform(lo + 0.25, length))
        E = int(rng.integers(1, 200))
        first, blocks, start, coords = blk.view_axis(n, grid, length, lo, hi, E)
        assert start[0] == 0 and start[-1] == E and (np.diff(start) >= 0).all() and len(start) == blocks + 1
        assert 0 <= first and first + blocks <= grid
        x = lo + (np.arange(E) + 0.5) * (hi - lo) / E
        g = first + np.repeat(np.arange(blocks), np.diff(start))
        assert np.array_equal(g, np.minimum(np.floor(x / n).astype(int), grid - 1)) or np.abs(x / n - np.rint(x / n)).min() < 1e-9
        want = (x - g * n - 0.5) / (n - 1)
        assert np.abs(coords - want).max() < 2e-7 * max(1.0, np.abs(want).max())
        # an interior sample lies within its block's footprint
        assert (coords >= np.float32(-0.5 / (n - 1))).all() and (coords <= np.float32(1 + 0.5 / (n - 1))).all()


def test_view_axis_thumbnails_have_empty_runs_and_bad_windows_raise():
    first, blocks, start, coords = blk.view_axis(16, 4, 64, 0, 64, 3)
    assert (first, blocks) == (0, 4) and np.array_equal(start, [0, 1, 1, 2, 3])
    first, blocks, start, coords = blk.view_axis(16, 135, 2160, 0, 2160, 20)
    assert (np.diff(start) == 0).sum() == blocks - 20 and start[-1] == 20
    assert (blk.view_axis(1, 5, 5, 1, 4, 7)[3] == 0).all()
    first, blocks, start, coords = blk.view_axis(16, 3, 48, 17, 18, 1)
    assert (first, blocks) == (1, 1) and np.array_equal(start, [0, 1]) and coords[0] == np.float32(1 / 15)
    for bad in [(-1, 5), (5, 5), (6, 5), (0, 64.5), (float("nan"), 3)]:
        with pytest.raises(ValueError):
            blk.view_axis(16, 4, 64, bad[0], bad[1], 8)
    with pytest.raises(ValueError):
        blk.view_axis(16, 4, 64, 0, 64, 0)
    with pytest.raises(ValueError):
        blk.view_axis(16, 4, 60, 0, 61, 8)                        # the padding of a ragged image cannot be asked for


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_on_an_aligned_view_is_the_blend_restatement():
    from blend_render_engine import blend_reference
    from oracle import smoe_oracle as o
    from render_engine import place_blocks
    b = blk.synthetic_blocks(6, (16, 16), 1, 7)
    p = o.init_params(b, [2, 2])
    cfg = o.OracleConfig(block_shape=(16, 16), channels=1, kernels=4)
    act = np.ones((6, 4), bool)
    m, grid = (24, 20), (2, 3)
    tabs = [blk.render_axis(16, mm) for mm in m]
    ext = [g * mm for g, mm in zip(grid, m)]
    for beta in (0.0, 2.0):
        ref = blend_reference(p, act, tabs, [16, 16], list(grid), beta, cfg)
        want = place_blocks(ref["recon"], m, grid, ext, 0, np.zeros(tuple(ext) + (1,), np.float32))
        ax = [blk.view_axis(16, g, 16 * g, 0, 16 * g, e) for g, e in zip(grid, ext)]
        r = view_reference(p, act, [16, 16], list(grid), [a[0] for a in ax], [a[2] for a in ax], [a[3] for a in ax], beta, cfg)
        assert np.array_equal(r["recon"], want)
        assert r["banded"].any() == (beta > 0)
        # a crop that starts inside a block: the same samples
        ax = [blk.view_axis(16, g, 16 * g, 5 * 16 / mm, (e - 3) * 16 / mm, e - 8) for g, e, mm in zip(grid, ext, m)]
        r = view_reference(p, act, [16, 16], list(grid), [a[0] for a in ax], [a[2] for a in ax], [a[3] for a in ax], beta, cfg)
        assert np.array_equal(r["recon"], want[5:ext[0] - 3, 5:ext[1] - 3])


# ---------------------------------------------------------------------------------------------------------------
# Smoe.render_view
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    s = _make(_image(40, 52, C=3, seed=3), use_yuv=True)
    s.train(3, val_iter=3)
    return s


def test_whole_window_equals_render(fitted):
    s = fitted
    for scale in (1, 2, 1.5):
        base, ids = s.render(scale=scale, want_argmax=True)
        out, vid = s.render_view(None, scale=scale, want_argmax=True)
        assert out.shape == base.shape and out.dtype == np.float32
        assert np.array_equal(out, base) and np.array_equal(vid, ids) and vid.dtype == np.int64
    assert np.array_equal(s.render_view([None, (0, 52)]), s.render())
    assert np.array_equal(s.render_view(None, size=(80, 104)), s.render(scale=2))


def test_aligned_crop_equals_the_crop_of_render(fitted):
    s = fitted
    for blend in (0.0, 2.0, (1, 2)):
        base, ids = s.render(scale=2, blend=blend, want_argmax=True)
        out, vid = s.render_view([(2.5, 37.0), (10.0, 45.5)], scale=2, blend=blend, want_argmax=True)
        assert out.shape == (69, 71, 3)
        assert np.array_equal(out, base[5:74, 20:91]) and np.array_equal(vid, ids[5:74, 20:91])
    assert not np.array_equal(s.render_view([(2.5, 37.0), (10.0, 45.5)], scale=2, blend=2), s.render(scale=2)[5:74, 20:91])
    u8 = s.render_view([(2.5, 37.0), (10.0, 45.5)], scale=2, blend=2, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(s.render(scale=2, blend=2)[5:74, 20:91] * 255).astype(np.uint8))
    dev = s.render_view([(2.5, 37.0), (10.0, 45.5)], scale=2, to_host=False)
    assert hasattr(dev, "cpu") and np.array_equal(dev.cpu().numpy(), s.render(scale=2)[5:74, 20:91])


def test_thumbnail_free_window_and_bad_arguments(fitted):
    s = fitted
    thumb, ids = s.render_view(None, size=(2, 3), want_argmax=True)
    assert thumb.shape == (2, 3, 3) and ids.shape == (2, 3)
    free = s.render_view([(5.3, 38.7), (10.0, 50.5)], size=(37, 53))
    assert free.shape == (37, 53, 3) and np.isfinite(free).all()
    assert s.render_view([(17, 18), None], size=(1, 52)).shape == (1, 52, 3)
    for kw in [dict(window=[(0, 41), None]), dict(window=[(3, 3), None]), dict(window=[(-1, 4), None]), dict(window=[(0, 4)]),
               dict(window=None, size=(4, 4), scale=2), dict(window=None, size=(0, 4)), dict(window=None, blend=9),
               dict(window=None, dtype=np.float64)]:
        with pytest.raises(ValueError):
            s.render_view(**kw)


def test_cli_window_and_size(tmp_path):
    import steered_mixture_of_experts_amd.smoe as smod
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--window", "1", "9.5", "0", "20", "--size", "30", "40"])
    assert a.window == [1.0, 9.5, 0.0, 20.0] and a.size == [30, 40]
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z"])
    assert a.window is None and a.size is None
    img = _image(32, 48)
    s = _make(img)
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig_factory = smod._default_engine_factory
    smod._default_engine_factory = lambda cfg, device: OracleViewEngine(cfg, device)
    try:
        out = str(tmp_path / "out")
        im = str(tmp_path / "img.npy")
        v, _, _ = rec.main(im, out, mp, window=[2.5, 20.0, 4.0, 40.0], scale=[2.0], blend=[2.0])
        assert v.shape == (35, 72, 1) and np.array_equal(v, s.render(scale=2, blend=2)[5:40, 8:80])
        assert np.load(out + "/2_reconstruction_view35x72_blend2.npy").shape == (35, 72, 1)
        v, _, _ = rec.main(im, out, mp, window=[2.5, 20.0, 4.0, 40.0], size=[10, 90])
        assert v.shape == (10, 90, 1) and np.array_equal(v, s.render_view([(2.5, 20.0), (4.0, 40.0)], size=(10, 90)))
        v, _, _ = rec.main(im, out, mp, size=[4, 6])
        assert np.array_equal(v, s.render_view(None, size=(4, 6)))
        for kw in [dict(window=[1.0, 2.0, 3.0]), dict(size=[4]), dict(size=[4, 4], scale=[2.0]), dict(size=[4, 4], frames=3)]:
            with pytest.raises(ValueError):
                rec.main(im, out, mp, **kw)
    finally:
        smod._default_engine_factory = orig_factory


def test_cli_refuses_whole_image_models(tmp_path):
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    from shared_render_engine import OracleSharedRenderEngine
    from steered_mixture_of_experts_amd.smoe import SharedSmoe
    img = _image(32, 32, seed=4)
    s = SharedSmoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], engine_factory=OracleSharedRenderEngine)
    assert not hasattr(s, "render_view")
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_0.pkl")
    utils.save_model(s, mp)
    rec._shared_engine_factory = OracleSharedRenderEngine
    try:
        with pytest.raises(ValueError, match="whole-image"):
            rec.main(str(tmp_path / "img.npy"), str(tmp_path / "out"), mp, size=[8, 8])
    finally:
        rec._shared_engine_factory = None


WORKER = r'''
import os, pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
from view_render_engine import OracleViewEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
ws = int(os.environ.get("WORLD_SIZE", "1"))
if ws > 1:
    dist.init_process_group(backend="gloo")
b = blk.synthetic_blocks(15, (16, 16), 1, 99)
img = blk.blocks_to_image(b, (48, 80), (16, 16))[:44, :75]
s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, engine_factory=OracleViewEngine)
s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
s.train(3, val_iter=3)
win = [(5.3, 41.7), (10.0, 70.5)]
view, ids = s.render_view(win, size=(37, 53), blend=(1, 2), want_argmax=True)
out = {"view": view, "ids": ids, "u8": s.render_view(win, scale=1.5, blend=1.5, dtype=np.uint8), "plain": s.render_view(win, size=(37, 53)),
       "thumb": s.render_view(None, size=(2, 3)), "crop": s.render_view([(2.5, 37.0), (10.0, 45.5)], scale=2, blend=2),
       "whole": s.render(scale=2, blend=2), "span": (s.lo, s.hi)}
if ws == 1 or dist.get_rank() == 0:
    pickle.dump(out, open(sys.argv[2], "wb"))
if ws > 1:
    dist.barrier(); dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_render_the_one_rank_view(tmp_path):
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
    assert a["view"].shape == (37, 53, 1) and not np.array_equal(a["view"], a["plain"])
    assert np.array_equal(a["crop"], a["whole"][5:74, 20:91])
    for k in ("view", "ids", "u8", "plain", "thumb", "crop"):
        assert np.array_equal(a[k], b[k]), k


def test_smoe_render_view_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_render_view\s*\(", src) and re.search(r"const\s+int32_t\*\s+const\s+axis_start\[3\]", src)
    assert hasattr(lib, "smoe_render_view") and "smoe_render_view" in _lib.EXPORTS
    bl = (C.c_float * 3)(1.0, 1.0, 0.0)
    rc = lib.smoe_render_view(None, None, None, None, None, None, None, None, bl, None, 0, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_render_view" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
