"""CPU tests of the shared-mode point and viewport decoders' host layer: the mapping of smoe_shared_sample as
``blocks.point_blocks`` states it, the numpy restatement (tests/shared_sample_engine.py), ``SharedSmoe.eval_points`` /
``eval_view`` / ``eval_warp`` driven through the oracle-backed stand-in engine, two gloo ranks against one, and what the two C
entry points check without a handle."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from shared_sample_engine import OracleSharedSampleEngine, point_mapping
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
from test_shared_render_cpu import _image
from test_view_render_cpu import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(img, bs, kpd, **kw):
    s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
                   engine_factory=OracleSharedSampleEngine, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


def _fitted(C=1, shape=(48, 64), bs=(16, 16), kpd=(6, 8)):
    """a few iterations with a readmission and pruned lists"""
    s = _make(_image(shape, C=C, seed=3 + C), bs, kpd, use_yuv=(C == 3))
    s.train(4, val_iter=2, ukl_iter=2)
    return s


def _centres(shape):
    return np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) + 0.5 for s in shape], indexing="ij"), axis=-1)


# ---------------------------------------------------------------------------------------------------------------
# the mapping
# ---------------------------------------------------------------------------------------------------------------
def test_pixel_centres_and_2x_positions_sit_on_the_render_tables():
    """u of the pixel centres q + 0.5 is render_axis(S, S), u of the 2x positions (j + 0.5) / 2 is render_axis(S, 2 S), bit
    for bit, for every S in 2 .. 512"""
    for S in range(2, 513):
        c = (np.arange(S, dtype=np.float64) + 0.5).astype(np.float32)[:, None]
        inside, _, u = blk.point_blocks(c, [S], [1], [S])
        assert inside.all() and u.dtype == np.float32
        assert np.array_equal(u[:, 0].view(np.uint32), blk.render_axis(S, S).view(np.uint32)), S
        x2 = (np.arange(2 * S, dtype=np.float64) + 0.5) / 2
        c2 = x2.astype(np.float32)[:, None]
        assert np.array_equal(c2[:, 0].astype(np.float64), x2)                     # exact in float32
        inside, _, u = blk.point_blocks(c2, [S], [1], [S])
        assert inside.all()
        assert np.array_equal(u[:, 0].view(np.uint32), blk.render_axis(S, 2 * S).view(np.uint32)), S


@pytest.mark.parametrize("nb,grid", [(16, 6), (7, 3), (5, 5), (32, 120)])
def test_a_point_on_a_batch_boundary_belongs_to_the_upper_batch(nb, grid):
    S = nb * grid
    g = np.arange(1, grid)
    on = (g * nb).astype(np.float32)
    below = np.nextafter(on, np.float32(-np.inf))
    inside, bid, _ = point_mapping(np.stack([on, np.full_like(on, 0.5)], axis=-1), (S, nb), (nb, nb))
    assert inside.all() and np.array_equal(bid, g)
    inside, bid, _ = point_mapping(np.stack([below, np.full_like(on, 0.5)], axis=-1), (S, nb), (nb, nb))
    assert inside.all() and np.array_equal(bid, g - 1)
    # the second axis: the batch id is row-major over the grid
    inside, bid, _ = point_mapping(np.stack([np.full_like(on, nb + 0.5), on], axis=-1), (2 * nb, S), (nb, nb))
    assert inside.all() and np.array_equal(bid, grid + g)


def test_nan_minus_zero_and_the_far_edge():
    S = (48, 64)
    pts = np.array([[np.nan, 1.0], [1.0, np.nan], [-0.0, 3.0], [0.0, 0.0], [48.0, 1.0], [1.0, 64.0], [-1e-30, 1.0],
                    [np.nextafter(np.float32(48), np.float32(0)), np.nextafter(np.float32(64), np.float32(0))],
                    [np.inf, 1.0]], np.float32)
    inside, bid, u = point_mapping(pts, S, (16, 16))
    assert inside.tolist() == [False, False, True, True, False, False, False, True, False]
    assert bid.tolist() == [-1, -1, 0, 0, -1, -1, -1, 11, -1]
    assert (u[~inside] == 0).all()
    assert u[2, 0] == np.float32(-0.5) / np.float32(47) and u[7, 0] > 1.0


# ---------------------------------------------------------------------------------------------------------------
# the facade through the oracle engine
# ---------------------------------------------------------------------------------------------------------------
def test_shared_smoe_has_the_three_methods():
    assert hasattr(SharedSmoe, "eval_points") and hasattr(SharedSmoe, "eval_view") and hasattr(SharedSmoe, "eval_warp")
    # the names Smoe uses stay free for the change that adds them with the CLI
    assert not hasattr(SharedSmoe, "sample") and not hasattr(SharedSmoe, "render_view") and not hasattr(SharedSmoe, "render_warp")


@pytest.mark.parametrize("C", [1, 3], ids=["gray", "rgb"])
def test_points_at_the_pixel_centres_are_the_render(C):
    s = _fitted(C)
    rec = s.get_reconstruction()
    assert np.array_equal(s.render(), rec)
    lens = np.array([m.sum() for m in s.kernel_list_per_batch])
    assert lens.min() < s.kernels, "the fit did not prune any list: the test would not see the lists"
    out, ids = s.eval_points(_centres((48, 64)), want_argmax=True)
    assert out.shape == (48, 64, C) and out.dtype == np.float32 and ids.shape == (48, 64) and ids.dtype == np.int64
    assert np.array_equal(out, rec)
    _, rids = s.render(want_argmax=True)
    assert np.array_equal(ids, rids)
    assert np.array_equal(s.eval_view(None), rec)
    assert np.array_equal(s.eval_view([None, (0, 64)], scale=1), rec)
    ident, wids = s.eval_warp([[1, 0, 0], [0, 1, 0]], (48, 64), want_argmax=True)
    assert np.array_equal(ident, rec) and np.array_equal(wids, rids)
    u8 = s.eval_points(_centres((48, 64)), dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(rec * 255).astype(np.uint8))
    assert np.array_equal(s.eval_view(None, dtype=np.uint8), u8)
    t = s.eval_points(_centres((48, 64)), to_host=False)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), rec)
    # without lists: the render without lists
    assert np.array_equal(s.eval_points(_centres((48, 64)), use_lists=False), s.render(use_lists=False))
    assert np.array_equal(s.eval_view(None, use_lists=False), s.render(use_lists=False))


def test_an_aligned_window_is_the_crop_of_the_render():
    s = _fitted(1)
    big, bids = s.render(scale=2, want_argmax=True)
    out, ids = s.eval_view([(16, 40), (8, 56)], scale=2, want_argmax=True)
    assert out.shape == (48, 96, 1)
    assert np.array_equal(out, big[32:80, 16:112]) and np.array_equal(ids, bids[32:80, 16:112])
    assert np.array_equal(s.eval_view([(16, 40), (8, 56)], size=(48, 96)), out)
    # a window that starts inside a batch, off the render grid, and a thumbnail with fewer samples than batches: the points
    win, E = [(5.25, 30.5), (17.0, 49.75)], (19, 23)
    xs = [np.float32(lo) + (np.arange(e) + 0.5) * ((hi - lo) / e) for (lo, hi), e in zip(win, E)]
    pts = np.stack(np.meshgrid(*xs, indexing="ij"), axis=-1).astype(np.float32)
    a, b = s.eval_view(win, size=E), s.eval_points(pts)
    assert a.shape == (19, 23, 1) and np.abs(a - b).max() <= 1.0001 / 255 and (a != b).mean() < 0.02
    thumb = s.eval_view(None, size=(2, 3))
    assert thumb.shape == (2, 3, 1)
    assert np.array_equal(thumb, s.eval_points(np.array([[[12, 64 / 6], [12, 32], [12, 320 / 6]],
                                                          [[36, 64 / 6], [36, 32], [36, 320 / 6]]], np.float32)))


def test_video_frame_and_leading_shapes():
    vid = _image((16, 32, 8), C=1, seed=11)
    v = _make(vid, (8, 16, 4), (2, 4, 2))
    v.train(2, val_iter=2)
    rec = v.get_reconstruction()
    assert np.array_equal(v.eval_points(_centres((16, 32, 8))), rec)
    frame = v.eval_view([None, None, (2, 3)], size=(16, 32, 1))
    assert frame.shape == (16, 32, 1, 1) and np.array_equal(frame[:, :, 0], rec[:, :, 2])
    pts = _centres((16, 32, 8))
    assert v.eval_points(pts[3, 4, 5]).shape == (1,)
    assert v.eval_points(pts[3, 4]).shape == (8, 1)
    one, ids = v.eval_points(pts[None, 3:5], want_argmax=True)
    assert one.shape == (1, 2, 32, 8, 1) and ids.shape == (1, 2, 32, 8)
    assert np.array_equal(one[0], rec[3:5])
    assert v.eval_points(np.zeros((0, 3), np.float32)).shape == (0, 1)
    # outside: 0 and -1
    out, ids = v.eval_points(np.array([[-1, 1, 1], [1, 32, 1], [1, 1, np.nan], [1.5, 1.5, 1.5]], np.float32), want_argmax=True)
    assert (out[:3] == 0).all() and (ids[:3] == -1).all() and ids[3] >= 0
    warp, wid = v.eval_warp(np.concatenate([np.eye(3), [[-4], [0], [0]]], axis=1), (16, 32, 8), want_argmax=True)
    assert np.array_equal(warp[4:], rec[:12]) and (warp[:4] == 0).all() and (wid[:4] == -1).all()


def test_argument_errors():
    s = _make(_image((48, 64), seed=5), (16, 16), (3, 4))
    for bad in ([(0, 49), None], [(-1, 4), None], [(5, 5), None], [(7, 3), None], [None], [None, None, None]):
        with pytest.raises(ValueError):
            s.eval_view(bad)
    with pytest.raises(ValueError):
        s.eval_view(None, size=(8, 8), scale=2)
    with pytest.raises(ValueError):
        s.eval_view(None, size=(8, 0))
    with pytest.raises(ValueError):
        s.eval_view(None, size=(8, 8, 8))
    with pytest.raises(ValueError):
        s.eval_view(None, scale=(1, 2, 3))
    with pytest.raises(ValueError):
        s.eval_view(None, dtype=np.float64)
    with pytest.raises(ValueError):
        s.eval_points(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        s.eval_points(np.zeros((4, 2), np.float32), dtype=np.int32)
    with pytest.raises(ValueError):
        s.eval_warp(np.eye(3), (8, 8))
    with pytest.raises(TypeError):
        s.eval_points(np.zeros((4, 2), np.float32), blend=1.0)


# ---------------------------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
from shared_sample_engine import OracleSharedSampleEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
ws = int(os.environ.get("WORLD_SIZE", "1"))
if ws > 1:
    dist.init_process_group(backend="gloo")
b = blk.synthetic_blocks(15, (16, 16), 1, 99)
img = blk.blocks_to_image(b, (48, 80), (16, 16))
s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=[4, 6], batch_size=[16, 16], use_determinant=True,
               engine_factory=OracleSharedSampleEngine)
s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
s.train(4, val_iter=2, ukl_iter=2)
c, sn = np.cos(np.deg2rad(17)) / 1.3, np.sin(np.deg2rad(17)) / 1.3
M = np.array([[c, -sn], [sn, c]])
A = np.concatenate([M, (np.array([24.0, 40.0]) - M @ np.array([25.0, 40.0]))[:, None]], axis=1)
warp, ids = s.eval_warp(A, (50, 80), want_argmax=True)
out = {"warp": warp, "ids": ids, "u8": s.eval_points(blk.warp_points(A, (50, 80)), dtype=np.uint8),
       "view": s.eval_view([(5.5, 40), (16, 70)], size=(33, 41)), "ident": s.eval_view(None), "recon": s.get_reconstruction(),
       "lens": [int(m.sum()) for m in s.kernel_list_per_batch], "span": (s.lo, s.hi)}
if ws == 1 or dist.get_rank() == 0:
    pickle.dump(out, open(sys.argv[2], "wb"))
if ws > 1:
    dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_evaluate_what_one_rank_evaluates(tmp_path):
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
    assert min(a["lens"]) < 24, "no list was pruned: the gather of the lists would not show"
    assert np.array_equal(a["ident"], a["recon"])
    assert (a["ids"] == -1).any() and (a["ids"] >= 0).any()                   # the rotated view leaves the image
    for k in ("warp", "ids", "u8", "view", "ident"):
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_check_their_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_shared_sample\s*\(", src) and re.search(r"\bint\s+smoe_shared_render_view\s*\(", src)
    assert re.search(r"const\s+int32_t\*\s+const\s+axis_batch\[3\]", src)
    for name in ("smoe_shared_sample", "smoe_shared_render_view"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    rc = lib.smoe_shared_sample(None, None, None, None, 5, None, 0, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_sample" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    ext = (C.c_int32 * 3)(4, 4, 1)
    rc = lib.smoe_shared_render_view(None, None, None, ext, None, None, None, 0, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_render_view" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
