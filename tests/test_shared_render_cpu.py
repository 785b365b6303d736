"""CPU tests of the shared-mode decoder's host layer: ``SharedSmoe.render`` driven through the oracle-backed stand-in
engine (tests/shared_render_engine.py), the CLI on a whole-image pickle, and the C ABI's declaration / argument check."""
import os
import re

import numpy as np
import pytest
import torch

from render_engine import place_blocks
from shared_render_engine import OracleSharedRenderEngine, oracle_shared_batches
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd import utils
from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(shape, C=1, seed=0):
    d = len(shape)
    bs = (16, 16) if d == 2 else (8, 8, 4)
    g = [-(-s // b) for s, b in zip(shape, bs)]
    b = blk.synthetic_blocks(int(np.prod(g)), bs, C, seed)
    full = blk.blocks_to_image(b, tuple(gi * bi for gi, bi in zip(g, bs)), bs)
    return np.ascontiguousarray(full[tuple(slice(0, s) for s in shape)])


def _make(img, bs, kpd, lr_steer=1.0, **kw):
    s = SharedSmoe(img, train_inverse_cov=False, kernels_per_dim=list(kpd), batch_size=list(bs), use_determinant=True,
                   engine_factory=OracleSharedRenderEngine, **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(lr_steer))
    return s


def _fitted(C=1, **kw):
    """a few iterations with a readmission and pruned lists"""
    s = _make(_image((48, 64), C=C, seed=3 + C), (16, 16), (6, 8), use_yuv=(C == 3), **kw)
    s.train(4, val_iter=2, ukl_iter=2)
    return s


# 1. scale = 1 is the reconstruction
@pytest.mark.parametrize("C", [1, 3], ids=["gray", "rgb"])
def test_render_at_scale_one_is_the_reconstruction(C):
    s = _fitted(C)
    rec = s.get_reconstruction()
    lens = np.array([m.sum() for m in s.kernel_list_per_batch])
    assert lens.min() < s.kernels, "the fit did not prune any list: the test would not see the lists"
    out = s.render(scale=1)
    assert out.shape == (48, 64, C) and out.dtype == np.float32
    assert np.array_equal(out, rec)
    assert np.array_equal(s.render(), rec)
    u8 = s.render(scale=1, dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.rint(rec * 255).astype(np.uint8))
    out2, ids = s.render(scale=1, want_argmax=True)
    assert np.array_equal(out2, rec) and ids.shape == (48, 64) and ids.dtype == np.int64
    am = s.get_weight_matrix_argmax()
    assert ((ids == am) | (ids == -1)).all() and (ids >= 0).mean() > 0.99
    t = s.render(scale=1, to_host=False)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), rec)


def test_render_at_scale_one_is_the_reconstruction_video():
    vid = _image((16, 32, 8), C=1, seed=11)
    s = _make(vid, (8, 16, 4), (2, 4, 2))
    s.train(2, val_iter=2)
    rec = s.get_reconstruction()
    assert rec.shape == (16, 32, 8, 1)
    assert np.array_equal(s.render(scale=1), rec)
    assert s.render(samples_per_block=(8, 16, 7)).shape == (16, 32, 14, 1)
    assert s.render(scale=(1, 2, 1.5)).shape == (16, 64, 12, 1)


def test_quantized_render_is_the_qreconstruction():
    s = _fitted(1, quantization_mode=1)
    assert s.rparams is not None
    assert np.array_equal(s.render(scale=1, quantized=True), s.get_qreconstruction())


# 2. shapes, dtypes, argument errors
def test_render_shapes_uint8_and_argument_errors():
    s = _make(_image((48, 64), seed=5), (16, 16), (3, 4))
    assert s.render(scale=2).shape == (96, 128, 1)
    assert s.render(scale=(1.5, 2)).shape == (72, 128, 1)
    assert s.render(samples_per_block=8).shape == (24, 32, 1)
    v = _make(_image((16, 16, 8), seed=6), (16, 16, 4), (2, 2, 1))
    assert v.render(samples_per_block=(16, 16, 7)).shape == (16, 16, 14, 1)
    f = s.render(scale=2)
    u = s.render(scale=2, dtype=np.uint8)
    assert f.dtype == np.float32 and u.dtype == np.uint8 and np.array_equal(u, np.rint(f * 255).astype(np.uint8))
    with pytest.raises(ValueError):
        s.render(scale=2, samples_per_block=8)
    with pytest.raises(ValueError):
        s.render(scale=(1, 2, 3))
    with pytest.raises(ValueError):
        s.render(samples_per_block=(8, 8, 8))
    with pytest.raises(ValueError):
        s.render(samples_per_block=(8, 0))
    with pytest.raises(ValueError):
        s.render(dtype=np.float64)


# 3. position
def test_render_evaluates_the_model_at_pixel_centres():
    """K = 1, y = nu + gamma . x inside (0, 1): the 2x render is the plane at render_axis' coordinates of the IMAGE axes
    (the mapping is centred, not shifted by half a pixel, and continuous across the batches)."""
    img = np.full((16, 32, 1), 0.5, dtype=np.float32)
    p = _make(img, (16, 16), (1, 1)).get_params()
    nu, g0, g1 = 0.31, 0.23, 0.37
    p["nu_e"][:] = nu
    p["gamma_e"][:, 0, 0] = g0
    p["gamma_e"][:, 1, 0] = g1
    s = SharedSmoe(img, train_inverse_cov=False, init_params=p, batch_size=[16, 16], use_determinant=True,
                   engine_factory=OracleSharedRenderEngine)
    out = s.render(scale=2)
    u0 = blk.render_axis(16, 32).astype(np.float64)
    u1 = blk.render_axis(32, 64).astype(np.float64)
    y = nu + g0 * u0[:, None] + g1 * u1[None, :]
    frac = (y * 255 + 0.5) % 1.0
    sure = (frac > 1e-3) & (frac < 1 - 1e-3)
    want = np.rint(255 * y) / 255
    assert out.shape == (32, 64, 1) and sure.mean() > 0.98
    assert np.abs(out[..., 0] - want)[sure].max() < 1e-6
    # a half-pixel shift of the grid would move the plane by g * 0.5 / 15 > one lattice step
    assert abs(out[0, 0, 0] - (nu + g0 * u0[0] + g1 * u1[0])) < 1 / 255


# 4. use_lists=False
def test_render_without_lists():
    """``use_lists=False`` is the render with all-ones lists exactly.  Against the pruned lists it differs, within a bound:
    if r is the sum of the all-kernels gate weights of the kernels missing from a sample's list, the other weights grow
    by 1 / (1 - r), so the lattice values differ by at most (255 * r / (1 - r) + 1) * max(1, max |e|) steps."""
    s = _fitted(1)
    s.get_reconstruction()
    lists = s._lists.clone()                      # as the last evaluation pass pruned them
    free = s.render(scale=1, use_lists=False)
    eng = s._engine
    axes = [torch.from_numpy(blk.render_axis(n, n)) for n in (48, 64)]
    rec = eng.render(s._params, lists, axes, (16, 16)).numpy()
    ones = eng.render(s._params, eng.new_lists(), axes, (16, 16))
    assert np.array_equal(free, ones.numpy())
    free2 = s.render(scale=2, use_lists=False)
    axes2 = [torch.from_numpy(blk.render_axis(n, 2 * n)) for n in (48, 64)]
    assert np.array_equal(free2, eng.render(s._params, eng.new_lists(), axes2, (32, 32)).numpy())
    # the bound, per sample on the training lattice, from the restatement's gate weights with every kernel listed
    K, NB = s.kernels, s.num_batches
    grid = (3, 4)
    p = {k: v.numpy()[None] for k, v in s._params.items()}
    f = oracle_shared_batches(p, np.ones((NB, K), bool), [a.numpy() for a in axes], (16, 16), grid, 0, eng.ocfg, np.float64)
    listed = eng._mask(lists)                                                   # (NB, K)
    r = np.where(listed[:, :, None], 0.0, f["w"]).sum(axis=1)                   # (NB, M)
    assert r.max() < 0.5
    x = np.stack(np.meshgrid(*[a.numpy().astype(np.float64) for a in axes], indexing="ij"), axis=-1)
    e = p["nu_e"][0][:, None, None, :] + np.einsum("klc,hwl->khwc", p["gamma_e"][0].astype(np.float64), x)
    emax = np.maximum(1.0, np.abs(e).max(axis=(0, 3)))                          # (H, W)
    steps = 255 * r / (1 - r) + 1
    bound = place_blocks(steps[..., None], (16, 16), grid, (48, 64), 0, np.zeros((48, 64, 1)))[..., 0] * emax
    diff = np.abs(free.astype(np.float64) - rec)[..., 0] * 255
    print(f"samples that differ between use_lists=False and the pruned lists: {(diff > 0).mean():.3e}, "
          f"max {diff.max():.2f} steps, max bound {bound.max():.2f}")
    assert (diff <= bound + 1e-6).all()


# 5. CLI
def test_cli_scale_option_on_a_whole_image_pickle(tmp_path):
    import steered_mixture_of_experts_amd.smoe_reconstruction as rec
    img = _image((32, 48), seed=2)
    s = _make(img, (16, 16), (3, 4))
    s.train(2, val_iter=2)
    np.save(tmp_path / "img.npy", np.uint8(np.round(img * 255)))
    mp = str(tmp_path / "params_2.pkl")
    utils.save_model(s, mp)
    orig = rec._shared_engine_factory
    rec._shared_engine_factory = OracleSharedRenderEngine
    try:
        out = str(tmp_path / "out")
        base, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp)
        assert base.shape == (32, 48, 1)
        big, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp, scale=[2.0])
        assert big.shape == (64, 96, 1)
        # a decoded model starts from full kernel lists (smoe.py:315): the fitted model's render without lists
        assert np.array_equal(big, s.render(scale=2, use_lists=False))
        if all(m.all() for m in s.kernel_list_per_batch):
            assert np.array_equal(big, s.render(scale=2))
        assert np.load(out + "/2_reconstruction_32x32.npy").shape == (64, 96, 1)
        wide, _, _ = rec.main(str(tmp_path / "img.npy"), out, mp, scale=[1.0, 2.0])
        assert wide.shape == (32, 96, 1)
    finally:
        rec._shared_engine_factory = orig


# 6. C ABI
def test_smoe_shared_render_is_declared_exported_and_checks_its_arguments():
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smoe_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smoe_shared_render\s*\(", src)
    assert hasattr(lib, "smoe_shared_render") and "smoe_shared_render" in _lib.EXPORTS
    rc = lib.smoe_shared_render(None, 0, 1, None, None, None, None, None, 0, None, None)
    assert rc == _lib.SMOE_ERR_INVALID and b"smoe_shared_render" in lib.smoe_last_error()
    assert lib.smoe_abi_version() == 2
