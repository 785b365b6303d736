"""CPU tests of the decoder's host layer: the sample mapping (blocks.render_axis), ``Smoe.render`` driven through the
oracle-backed stand-in engine (tests/render_engine.py), the CLI options, and the C ABI's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from render_engine import OracleRenderEngine
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
             engine_factory=OracleRenderEngine, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    return s


def test_render_axis_identity_is_the_training_lattice():
    for n in range(1, 65):
        a = blk.render_axis(n, n)
        assert a.dtype == np.float32 and np.array_equal(a, np.linspace(0, 1, n).astype(np.float32)), n
    assert np.array_equal(blk.render_axis(1, 5), np.zeros(5, np.float32))


@pytest.mark.parametrize("n,m", [(16, 32), (16, 40), (16, 24), (32, 48), (4, 7), (7, 11), (5, 16), (12, 6), (10, 5), (3, 9),
                                 (16, 48), (2, 3), (64, 7)])
def test_render_axis_is_increasing_symmetric_and_centred(n, m):
    a = blk.render_axis(n, m)
    assert a.shape == (m,) and a.dtype == np.float32
    assert (np.diff(a.astype(np.float64)) > 0).all()
    s = a + a[::-1]
    assert (np.abs(s - np.float32(1)) <= np.spacing(np.float32(1))).all()
    # overhang of less than half a source pixel
    assert a[0] > -0.5 / (n - 1) and a[-1] < 1 + 0.5 / (n - 1)
    if m % n == 0:                                   # integer scale: every group of s samples is centred on its pixel
        sc = m // n
        src = np.linspace(0, 1, n)
        assert np.abs(a.astype(np.float64).reshape(n, sc).mean(axis=1) - src).max() < 1e-6


def test_render_at_scale_one_is_the_reconstruction_ragged_image():
    img = _image(40, 52, C=3, seed=3)
    s = _make(img, use_yuv=True)
    s.train(3, val_iter=3)
    rec = s.get_reconstruction()
    out = s.render(scale=1)
    assert out.shape == (40, 52, 3) and out.dtype == np.float32
    assert np.array_equal(out, rec)
    assert np.array_equal(s.render(), rec)
    u8 = s.render(scale=1, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(rec * 255).astype(np.uint8))
    out2, ids = s.render(scale=1, want_argmax=True)
    assert np.array_equal(out2, rec) and ids.shape == (40, 52) and ids.dtype == np.int64
    am = s.get_weight_matrix_argmax()
    assert ((ids == am) | (ids == -1)).all() and (ids >= 0).mean() > 0.99
    assert (ids[16:32, 16:32][ids[16:32, 16:32] >= 0] // 4 == 1 * 4 + 1).all()       # block (1, 1) of a 3 x 4 grid


def test_render_at_scale_one_is_the_reconstruction_video():
    b = blk.synthetic_blocks(4, (8, 8, 4), 1, 11)
    vid = blk.blocks_to_image(b, (16, 16, 4), (8, 8, 4))[:13]
    s = _make(vid, bs=(8, 8, 4), kpd=(2, 2, 1))
    rec = s.get_reconstruction()
    assert rec.shape == (13, 16, 4, 1)
    assert np.array_equal(s.render(scale=1), rec)
    assert s.render(samples_per_block=(8, 8, 7)).shape == (13, 16, 7, 1)
    assert s.render(scale=(1, 2, 1.5)).shape == (13, 32, 6, 1)


def test_render_shapes_and_uint8():
    img = _image(40, 52, C=1, seed=5)
    s = _make(img)
    assert s.render(scale=2).shape == (80, 104, 1)
    assert s.render(scale=(1.5, 2)).shape == (60, 104, 1)            # 24 x 32 samples per block
    assert s.render(samples_per_block=(5, 16)).shape == (12, 52, 1)  # 40 * 5 // 16
    assert s.render(samples_per_block=8).shape == (20, 26, 1)
    f = s.render(scale=2)
    u = s.render(scale=2, dtype=np.uint8)
    assert u.dtype == np.uint8 and np.array_equal(u, np.rint(f * 255).astype(np.uint8))
    with pytest.raises(ValueError):
        s.render(scale=2, samples_per_block=8)
    with pytest.raises(ValueError):
        s.render(scale=(1, 2, 3))
    with pytest.raises(ValueError):
        s.render(dtype=np.float64)


def test_render_evaluates_the_model_at_pixel_centres():
    """K = 1, y = nu + gamma * x inside (0, 1): the 3x render is the plane at render_axis' coordinates (the mapping is
    centred, not shifted by half a pixel)."""
    img = np.full((16, 32, 1), 0.5, dtype=np.float32)
    s = _make(img, kpd=(1, 1))
    p = s.get_params()
    nu, g0, g1 = 0.31, 0.23, 0.37
    p["nu_e"][:] = nu
    p["gamma_e"][:, :, 0, 0] = g0
    p["gamma_e"][:, :, 1, 0] = g1
    s2 = Smoe(img, train_inverse_cov=False, init_params=p, batch_size=[16, 16], use_determinant=True,
              engine_factory=OracleRenderEngine)
    out = s2.render(scale=3)
    u = blk.render_axis(16, 48).astype(np.float64)
    y = nu + g0 * u[:, None] + g1 * u[None, :]
    frac = (y * 255 + 0.5) % 1.0
    sure = (frac > 1e-3) & (frac < 1 - 1e-3)
    want = np.rint(255 * y) / 255
    assert out.shape == (48, 96, 1) and sure.mean() > 0.98
    for gx in range(2):
        got = out[:, gx * 48:(gx + 1) * 48, 0]
        assert np.abs(got - want)[sure].max() < 1e-6
    # a half-pixel shift of the grid would move the plane by g * 0.5 / 15 > one lattice step
    assert abs(out[0, 0, 0] - (nu + (g0 + g1) * u[0])) < 1 / 255


@pytest.mark.parametrize("precision", [6, 10])
def test_restatement_renders_on_the_lattice_of_the_precision(precision):
    """The CPU half of test_gpu_render.py's precision cases: the same model and sample tables through the restatement and
    the stand-in engine.  The image sits on the lattice of 2^p - 1 levels (at 10 bits NOT on the 255-level one), the 8-bit
    image is the lattice index, and the condition on the inputs that the GPU case asserts holds."""
    import torch
    from render_cases import _axes, _lattice, _setup
    from render_engine import oracle_blocks
    from steered_mixture_of_experts_amd.engine import EngineConfig
    shape, C_, kpd, m, B = (16, 16), 3, [2, 2], (40, 24), 37
    cfg, p, _, K = _setup(shape, C_, kpd, True, B, 100 + len(shape) + C_, precision=precision)
    active = np.random.default_rng(5).uniform(size=(B, K)) < 0.85
    levels, tau, band = _lattice(precision)
    assert (levels, tau) == (2 ** precision - 1, 0.5 / 2 ** precision) and _lattice(8) == (255, 0.5 / 256, 1e-6)
    tabs = _axes(shape, m)
    ref, _ = oracle_blocks(p, active, tabs, cfg, np.float32)
    ref64, _ = oracle_blocks(p, active, tabs, cfg, np.float64)
    frac = (np.clip(ref64["y"], 0, 1) * levels + 0.5) % 1.0
    loose = ((frac < 2e-4) | (frac > 1 - 2e-4)) | (np.abs(ref64["w"] - tau) < band).any(axis=1)[..., None]
    assert loose.mean() < 0.01
    assert (np.abs(ref["recon"] - ref64["recon"])[~np.broadcast_to(loose, frac.shape)] < 1e-7).all()
    idx = ref["recon"].astype(np.float64) * levels
    assert np.abs(idx - np.rint(idx)).max() < 1e-3 and np.rint(idx).max() <= levels and len(np.unique(np.rint(idx))) > levels // 4
    if precision > 8:
        assert np.abs(ref["recon"] * 255 - np.rint(ref["recon"] * 255)).max() > 0.25
    eng = OracleRenderEngine(EngineConfig(block_shape=shape, channels=C_, kernels=K, use_yuv=True, precision=precision))
    dp = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in p.items()}
    bits = torch.from_numpy((active.astype(np.uint32) << np.arange(K, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32).view(np.int32))
    grid, axes = (5, 8), [torch.from_numpy(np.ascontiguousarray(t)) for t in tabs]
    extent = [g * mm for g, mm in zip(grid, m)]
    img = eng.render(dp, bits, axes, grid, extent).numpy()
    assert np.array_equal(img[:m[0], :m[1]].reshape(-1, C_), ref["recon"][0].astype(np.float32))
    if precision <= 8:
        u8 = eng.render(dp, bits, axes, grid, extent, dtype=torch.uint8).numpy()
        assert np.array_equal(u8, np.rint(img * levels).astype(np.uint8)) and u8.max() <= levels


def test_quantized_render_is_the_qreconstruction():
    img = _image(32, 32, seed=2)
    s = _make(img, quantization_mode=1)
    s.train(2, val_iter=2)
    assert s.rparams is not None
    assert np.array_equal(s.render(scale=1, quantized=True), s.get_qreconstruction())


def test_shared_mode_has_no_render():
    from fake_engine import OracleSharedEngine
    img = _image(32, 32, seed=4)
    s = SharedSmoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], engine_factory=OracleSharedEngine)
    with pytest.raises(NotImplementedError):
        s.render(scale=2)


def test_cli_scale_option(tmp_path):
    import steered_mixture_of_experts_amd.smoe as smod
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    img = _image(32, 48)
    s = _make(img)
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig_factory = smod._default_engine_factory
    smod._default_engine_factory = lambda cfg, device: OracleRenderEngine(cfg, device)
    try:
        out = str(tmp_path / "out")
        base, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp)
        assert np.array_equal(base, s.get_reconstruction())                      # the defaults leave the output as it was
        assert sorted(f for f in os.listdir(out) if f.endswith(".npy")) == ["2_reconstruction.npy"]
        big, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp, scale=[2.0])
        assert big.shape == (64, 96, 1)
        assert np.array_equal(big, s.render(scale=2))
        assert np.load(out + "/2_reconstruction_32x32.npy").shape == (64, 96, 1)
        wide, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp, scale=[1.0, 2.0])
        assert wide.shape == (32, 96, 1)
        with pytest.raises(ValueError):
            rec.main(str(tmp_path / "img.npy"), out, mp, frames=7)
    finally:
        smod._default_engine_factory = orig_factory


def test_smoe_render_is_declared_exported_and_checks_its_arguments():
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_render\s*\(", src) and "SMOE_IMAGE_F32" in src and "SMOE_IMAGE_U8" in src
    assert hasattr(lib, "smoe_render") and "smoe_render" in _lib.EXPORTS
    rc = lib.smoe_render(None, 0, 1, None, None, None, None, None, None, None, 0, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_render" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2
