"""CPU tests of the seam-free decoder's host layer: the numpy restatement (tests/blend_render_engine.py), ``Smoe.render(blend=)``
driven through the oracle-backed stand-in engine, ``SharedSmoe``'s refusal, the CLI option, two gloo ranks against one, and
what the C entry point checks without a handle."""
import os
import pickle
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from blend_render_engine import OracleBlendEngine, axis_weights, blend_reference
from render_engine import oracle_blocks
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd import utils
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe, Smoe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(h, w, C=1, seed=0):
    gh, gw = -(-h // 16), -(-w // 16)
    b = blk.synthetic_blocks(gh * gw, (16, 16), C, seed)
    return blk.blocks_to_image(b, (gh * 16, gw * 16), (16, 16))[:h, :w]


def _make(img, bs=(16, 16), kpd=(2, 2), **kw):
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
             engine_factory=OracleBlendEngine, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


def test_axis_weights_are_a_partition_of_unity_across_the_seam():
    """Seen from both sides of a seam the two weights of a position add up to 1, are 1/2 : 1/2 on the seam, and vanish
    beyond the band."""
    n, beta = 16, 2.0
    pos = np.linspace(13.0, 18.0, 201)                        # source pixels; the seam between blocks 0 and 1 is at 15.5
    own = axis_weights(n, (pos / (n - 1)).astype(np.float32), beta, np.float64)            # block 0 towards block 1
    nbr = axis_weights(n, ((pos - n) / (n - 1)).astype(np.float32), beta, np.float64)      # block 1 towards block 0
    left, right = pos < 15.5, pos > 15.5
    assert (own[left] >= 0).all() and (own[left] <= 0.5).all() and (nbr[right] <= 0).all() and (nbr[right] >= -0.5).all()
    want = np.clip(0.5 * (1 + (pos - 15.5) / beta), 0, 1)     # weight of block 1 at every position
    assert np.abs(np.where(left, own, 1 + nbr)[left | right] - want[left | right]).max() < 1e-6
    assert (own[pos < 13.5] == 0).all() and (nbr[pos > 17.5] == 0).all()
    assert (axis_weights(1, np.zeros(5, np.float32), 0.5) == 0).all() and (axis_weights(16, np.zeros(5, np.float32), 0) == 0).all()


def test_restatement_without_neighbours_is_the_plain_restatement():
    """blend = 0, or a 1 x 1 grid: the restatement equals oracle.forward's recon."""
    b = blk.synthetic_blocks(6, (16, 16), 1, 7)
    from oracle import smoe_oracle as o
    p = o.init_params(b, [2, 2])
    cfg = o.OracleConfig(block_shape=(16, 16), channels=1, kernels=4)
    act = np.ones((6, 4), bool)
    tabs = [blk.render_axis(16, 24), blk.render_axis(16, 20)]
    plain, _ = oracle_blocks(p, act, tabs, cfg)
    r0 = blend_reference(p, act, tabs, [16, 16], [2, 3], 0.0, cfg)
    assert np.array_equal(r0["recon"], plain["recon"]) and not r0["banded"].any()
    r2 = blend_reference(p, act, tabs, [16, 16], [2, 3], 2.0, cfg)
    assert r2["banded"].any() and not r2["banded"].all()
    assert np.array_equal(r2["recon"][~r2["banded"]], plain["recon"][~r2["banded"]])
    assert (r2["nblocks"][r2["banded"]] >= 1).all() and r2["nblocks"].max() == 4
    one = {k: v[:1] for k, v in p.items()}
    r1 = blend_reference(one, act[:1], tabs, [16, 16], [1, 1], 2.0, cfg)
    assert np.array_equal(r1["recon"], plain["recon"][:1])


def test_render_blend_zero_is_render():
    img = _image(40, 52, C=3, seed=3)
    s = _make(img, use_yuv=True)
    s.train(3, val_iter=3)
    base = s.render(scale=2)
    assert np.array_equal(s.render(scale=2, blend=0), base)
    assert np.array_equal(s.render(scale=2, blend=0.0), base)
    assert np.array_equal(s.render(scale=2, blend=(0, 0)), base)
    assert np.array_equal(s.render(blend=0), s.get_reconstruction())


def test_render_blend_changes_only_the_bands_and_broadcasts():
    img = _image(40, 52, C=1, seed=5)
    s = _make(img)
    s.train(2, val_iter=2)
    base, ids0 = s.render(scale=2, want_argmax=True)
    out, ids = s.render(scale=2, blend=2, want_argmax=True)
    assert out.shape == base.shape == (80, 104, 1) and out.dtype == np.float32
    assert np.array_equal(ids, ids0)                          # the kernel map is the own block's
    changed = (out != base)[..., 0]
    assert changed.any()
    # 2x: block borders at multiples of 32 output samples, band = 2 source pixels = 4 samples on either side
    r, c = np.arange(80)[:, None], np.arange(104)[None, :]
    near = lambda x, hi: ((x % 32 < 4) & (x >= 32)) | ((x % 32 >= 28) & (x < hi))
    band = near(r, 64) | near(c, 96)
    assert not changed[~band].any()
    assert np.array_equal(s.render(scale=2, blend=(2, 2)), out)
    assert np.array_equal(s.render(scale=2, blend=[2.0]), out)
    rows = s.render(scale=2, blend=(1, 2))
    assert not np.array_equal(rows, out)
    only_rows = s.render(scale=2, blend=(1, 0))
    ch = (only_rows != base)[..., 0]
    assert ch.any() and not ch[~np.broadcast_to(near(r, 64), ch.shape)].any()
    u8 = s.render(scale=2, blend=2, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(out * 255).astype(np.uint8))
    for bad in (-1, 9, (1, 2, 3), float("nan")):
        with pytest.raises(ValueError):
            s.render(scale=2, blend=bad)


def test_render_blend_closes_the_seam_between_two_planes():
    """K = 1 per block, gate exactly 1, two different planes side by side: the blended 3x render is the window-weighted
    mean of the planes, and the step across the seam is no larger than a step inside the band."""
    img = np.full((16, 32, 1), 0.5, dtype=np.float32)
    s0 = _make(img, kpd=(1, 1))
    p = s0.get_params()
    p["nu_e"][0], p["nu_e"][1] = 0.30, 0.70
    p["gamma_e"][0, :, 0, 0], p["gamma_e"][0, :, 1, 0] = 0.10, 0.20
    p["gamma_e"][1, :, 0, 0], p["gamma_e"][1, :, 1, 0] = -0.05, 0.12
    s = Smoe(img, train_inverse_cov=False, init_params=p, batch_size=[16, 16], use_determinant=True,
             engine_factory=OracleBlendEngine)
    out = s.render(scale=3, blend=2)[..., 0]
    plain = s.render(scale=3)[..., 0]
    u = blk.render_axis(16, 48).astype(np.float64)
    P = 16 / 15
    x = np.concatenate([u, u + P])                            # image coordinate in units of block 0
    planes = [0.30 + 0.10 * u[:, None] + 0.20 * x[None, :], 0.70 - 0.05 * u[:, None] + 0.12 * (x[None, :] - P)]
    w1 = np.clip(0.5 * (1 + (x - (1 + 0.5 / 15)) / (2 / 15)), 0, 1)[None, :]
    want = (1 - w1) * planes[0] + w1 * planes[1]
    frac = (want * 255 + 0.5) % 1.0
    sure = (frac > 1e-3) & (frac < 1 - 1e-3)
    assert np.abs(out - np.rint(want * 255) / 255)[sure].max() < 1e-6 and sure.mean() > 0.98
    step = np.abs(np.diff(out, axis=1))                      # step[:, j]: between samples j and j + 1; the seam is j = 47
    assert step[:, 47].max() <= np.delete(step[:, 42:53], 5, axis=1).max() + 1 / 255 + 1e-6
    assert np.abs(np.diff(plain, axis=1))[:, 47].max() > 0.1


def test_shared_mode_refuses_blend():
    from shared_render_engine import OracleSharedRenderEngine
    img = _image(32, 32, seed=4)
    s = SharedSmoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], engine_factory=OracleSharedRenderEngine)
    with pytest.raises(ValueError, match="seams"):
        s.render(scale=2, blend=1)
    assert s.render(scale=2, blend=0).shape == (64, 64, 1)


def test_cli_blend_option(tmp_path):
    import steered_mixture_of_experts_amd.smoe as smod
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--blend", "1.5"])
    assert a.blend == [1.5] and a.scale is None
    a = rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z", "--scale", "2", "--blend", "1", "2"])
    assert a.blend == [1.0, 2.0] and a.scale == [2.0]
    assert rec._parser().parse_args(["-i", "x", "-r", "y", "-p", "z"]).blend is None
    img = _image(32, 48)
    s = _make(img)
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig_factory = smod._default_engine_factory
    smod._default_engine_factory = lambda cfg, device: OracleBlendEngine(cfg, device)
    try:
        out = str(tmp_path / "out")
        big, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp, scale=[2.0], blend=[2.0])
        assert big.shape == (64, 96, 1)
        assert np.array_equal(big, s.render(scale=2, blend=2))
        assert not np.array_equal(big, s.render(scale=2))
        assert np.load(out + "/2_reconstruction_32x32_blend2.npy").shape == (64, 96, 1)
        same, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp, blend=[1.0, 0.5])      # scale 1, blended
        assert same.shape == (32, 48, 1) and np.array_equal(same, s.render(blend=(1, 0.5)))
    finally:
        smod._default_engine_factory = orig_factory


WORKER = r'''
import os, pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
from blend_render_engine import OracleBlendEngine
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.smoe import Adam, Smoe
ws = int(os.environ.get("WORLD_SIZE", "1"))
if ws > 1:
    dist.init_process_group(backend="gloo")
b = blk.synthetic_blocks(15, (16, 16), 1, 99)
img = blk.blocks_to_image(b, (48, 80), (16, 16))[:44, :75]
s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, engine_factory=OracleBlendEngine)
s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
s.train(3, val_iter=3)
img2, ids = s.render(scale=2, blend=(1, 2), want_argmax=True)
out = {"blend": img2, "ids": ids, "u8": s.render(scale=1.5, blend=1.5, dtype=np.uint8), "plain": s.render(scale=2), "span": (s.lo, s.hi)}
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


def test_two_ranks_render_the_one_rank_image(tmp_path):
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
    assert a["blend"].shape == (88, 150, 1) and not np.array_equal(a["blend"], a["plain"])
    for k in ("blend", "ids", "u8", "plain"):
        assert np.array_equal(a[k], b[k]), k


def test_smoe_render_blend_is_declared_exported_and_checks_its_arguments():
    import ctypes as C
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_render_blend\s*\(", src) and re.search(r"const\s+float\s+blend\[3\]", src)
    assert hasattr(lib, "smoe_render_blend") and "smoe_render_blend" in _lib.EXPORTS
    bl = (C.c_float * 3)(1.0, 1.0, 0.0)
    rc = lib.smoe_render_blend(None, 0, 1, None, None, None, None, None, None, bl, None, 0, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_render_blend" in lib.smoe_last_error() and b"handle" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2 and _lib.SMOE_ABI_VERSION == 2
