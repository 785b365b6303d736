"""GPU tests of the seam-free decoder (smoe_render_blend through the C ABI and the facade): parity with the numpy restatement
(tests/blend_render_engine.py), identity with smoe_render where no neighbour has weight, the closed form of two planes,
shards / bounds, and the argument checks with a real handle.

Parity criterion = the project's existing one for ``recon`` (tests/test_gpu_render.py): with ``frac = (v64 * 255 + 0.5) mod 1``
from the float64 restatement, samples are identical (< 1e-7) where ``frac`` is farther than 2e-4 from 0 / 1 and differ by at
most one LSB elsewhere.  A sample is loose as well -- held to the one-LSB bound only -- if in any block with weight on it some
kernel's float64 gate lies within 1e-6 of the influence threshold.  Condition on the inputs: loose share < 0.01 and no
float32-vs-float64 difference of the restatement outside the loose set."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from blend_render_engine import blend_reference
from render_cases import _axes, _bits, _dev_axes, _engine, _guarded, _image, _owned, _setup, _to_dev
from render_engine import place_blocks
from steered_mixture_of_experts_amd import blocks as blk

pytestmark = pytest.mark.gpu

MODE2 = dict(quantization_mode=2, quantize_pis=True, bit_depths=(14, 12, 8, 10, 10), lower_bounds=(-60, -.3, -1, 0, -4),
             upper_bounds=(60, 1.3, 2, 2, 4))
CASES = [
    # block shape, C, kernels per dim, samples per block, blend, engine / oracle options
    ((16, 16), 1, [2, 2], (16, 16), 1.5, {}),
    ((16, 16), 3, [2, 2], (40, 24), 2, {}),
    ((32, 32), 3, [2, 4], (48, 80), 3, {}),
    ((7, 5), 1, [2, 2], (11, 16), 1, {}),
    ((16, 16, 4), 3, [2, 2, 1], (32, 32, 7), (2, 2, 1), {}),
    ((12, 10, 3), 3, [2, 2, 1], (6, 5, 9), 1, {}),
    ((16, 16), 1, [2, 2], (24, 20), 8, {}),                                  # the maximal band
    ((16, 16), 3, [2, 2], (40, 24), 2, dict(train_inverse_cov=True)),
    ((16, 16), 3, [2, 2], (40, 24), 2, MODE2),
    # 300 > 256 innermost samples: CL = 256, two passes, the second ragged
    ((7, 5), 1, [2, 2], (3, 300), 1, {}),
    # nine blocks on a grid line: the 48 KB cap on the records lowers NB from 9 to 7 (9 x (NB + 2) records of 140 floats), so a
    # workgroup boundary falls between blocks 6 and 7 and the neighbour records cross it
    ((12, 10, 3), 3, [2, 2, 1], (2, 2, 3), 1, {}, (1, 1, 9)),
]
IDS = ["x".join(map(str, c[0])) + "-c%d-to-" % c[1] + "x".join(map(str, c[3])) + "-b" + "x".join(map(str, np.atleast_1d(c[4])))
       + ("-ic" if c[5].get("train_inverse_cov") else "") + ("-mode2" if c[5].get("quantization_mode") else "") for c in CASES]


def _grid_of(case):
    """the block grid of a case: its own (seventh entry), or the suite's for its dimension"""
    return case[6] if len(case) > 6 else ((3, 4) if len(case[0]) == 2 else (2, 3, 2))


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """parameters drawn as tests/test_gpu_render.py draws them, for a FULL block grid; the restatement in both precisions"""
    shape, C_, kpd, m, beta, kw = CASES[i][:6]
    grid = _grid_of(CASES[i])
    B = int(np.prod(grid))
    cfg, p, _, K = _setup(shape, C_, kpd, C_ == 3, B, 100 + len(shape) + C_, **kw)
    active = np.random.default_rng(5).uniform(size=(B, K)) < 0.85
    p["pis"][3, 0] = 0.0
    p["pis"][4, K - 1] = -0.1
    if kw.get("train_inverse_cov"):                      # keep the matrices positive definite (tests/test_gpu_invcov.py)
        p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
        p["A_corr"] = (p["A_corr"] * 2.0).astype(np.float32)
    tabs = _axes(shape, m)
    ref = blend_reference(p, active, tabs, list(shape), list(grid), beta, cfg, np.float32)
    ref64 = blend_reference(p, active, tabs, list(shape), list(grid), beta, cfg, np.float64)
    return cfg, p, K, active, grid, tabs, ref, ref64


# ---------------------------------------------------------------------------------------------------------------
# 1. parity with the restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_parity_with_the_restatement(i):
    shape, C_, kpd, m, beta, kw = CASES[i][:6]
    cfg, p, K, active, grid, tabs, ref, ref64 = _inputs(i)
    judge_blend(shape, C_, m, beta, kw, p, K, active, grid, tabs, ref, ref64)


def judge_blend(shape, C_, m, beta, kw, p, K, active, grid, tabs, ref, ref64):
    """the criterion of the module's docstring: the condition on the inputs from the restatement (``blend_reference`` in
    float32 and float64) alone, then the kernel"""
    lsb = 1.0 / 255
    frac = (ref64["v"] * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    loose = tie | ref64["near_tau"][..., None]
    print(f"restatement: tie share {tie.mean():.2e}, loose share {loose.mean():.2e}, samples in a band {ref['banded'].mean():.2f}, "
          f"up to {ref['nblocks'].max()} blocks per sample, samples with no block left {(ref['nblocks'] == 0).sum()}")
    assert loose.mean() < 0.01
    assert (np.abs(ref["recon"] - ref64["recon"])[~loose] < 1e-7).all()

    eng = _engine(shape, C_, K, use_yuv=(C_ == 3), **kw)
    dp, act, axes = _to_dev(p), _bits(active), _dev_axes(tabs)
    extent = [g * mm for g, mm in zip(grid, m)]
    img = eng.render_blend(dp, act, axes, grid, extent, beta)
    u8 = eng.render_blend(dp, act, axes, grid, extent, beta, dtype=torch.uint8)
    torch.cuda.synchronize()
    img, u8 = img.cpu().numpy(), u8.cpu().numpy()
    want = place_blocks(ref["recon"].astype(np.float32), m, grid, extent, 0, np.zeros(tuple(extent) + (C_,), np.float32))
    lo = place_blocks(loose, m, grid, extent, 0, np.zeros(tuple(extent) + (C_,), bool))
    dd = np.abs(img - want)
    print(f"kernel: max difference outside the loose set {dd[~lo].max():.3e}, overall {dd.max():.3e}, "
          f"samples that differ {(dd > 1e-7).mean():.2e}")
    assert (dd[~lo] < 1e-7).all(), dd[~lo].max()
    assert (dd <= lsb * 1.0001).all(), dd.max()
    assert np.array_equal(u8, np.rint(img * 255).astype(np.uint8))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. identity with smoe_render
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_identity_with_render(i):
    shape, C_, kpd, m, beta, kw = CASES[i][:6]
    cfg, p, K, active, grid, tabs, ref, _ = _inputs(i)
    eng = _engine(shape, C_, K, use_yuv=(C_ == 3), **kw)
    dp, act, axes = _to_dev(p), _bits(active), _dev_axes(tabs)
    extent = [g * mm - max(1, mm // 3) for g, mm in zip(grid, m)]            # ragged: cut into the last blocks
    plain, am = eng.render(dp, act, axes, grid, extent, want_argmax=True)
    zero, am0 = eng.render_blend(dp, act, axes, grid, extent, 0.0, want_argmax=True)
    out, am1 = eng.render_blend(dp, act, axes, grid, extent, beta, want_argmax=True)
    torch.cuda.synchronize()
    assert torch.equal(zero, plain) and torch.equal(am0, am)                 # blend = 0: bit for bit
    assert torch.equal(am1, am)                                              # the kernel map is the own block's
    plain, out = plain.cpu().numpy(), out.cpu().numpy()
    banded = place_blocks(ref["banded"][..., None], m, grid, extent, 0, np.zeros(tuple(extent) + (1,), bool))[..., 0]
    assert banded.any() and not banded.all()                                 # (the maximal band leaves the block corners of the image)
    assert np.array_equal(out.view(np.uint32)[~banded], plain.view(np.uint32)[~banded])
    assert (out != plain).any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. closed form, through the facade
# ---------------------------------------------------------------------------------------------------------------
def test_two_planes_closed_form():
    """K = 1 per block, gate exactly 1, two blocks side by side with different planes inside (0, 1): the 3x render with
    blend = 2 is the window-weighted mean of the planes at render_axis' coordinates, each plane alone outside the band, and
    the step across the seam is no larger than a step inside the band plus one LSB."""
    from steered_mixture_of_experts_amd.smoe import Smoe
    img = np.full((16, 32, 1), 0.5, dtype=np.float32)
    s0 = Smoe(img, train_inverse_cov=False, kernels_per_dim=[1, 1], batch_size=[16, 16], use_determinant=True)
    p = s0.get_params()
    p["nu_e"][0], p["nu_e"][1] = 0.30, 0.70
    p["gamma_e"][0, :, 0, 0], p["gamma_e"][0, :, 1, 0] = 0.10, 0.20
    p["gamma_e"][1, :, 0, 0], p["gamma_e"][1, :, 1, 0] = -0.05, 0.12
    s = Smoe(img, train_inverse_cov=False, init_params=p, batch_size=[16, 16], use_determinant=True)
    out = s.render(scale=3, blend=2)[..., 0]
    plain = s.render(scale=3)[..., 0]
    assert out.shape == (48, 96)
    u = blk.render_axis(16, 48).astype(np.float64)
    P = 16 / 15
    x = np.concatenate([u, u + P])                                           # image coordinate in units of block 0
    planes = [0.30 + 0.10 * u[:, None] + 0.20 * x[None, :], 0.70 - 0.05 * u[:, None] + 0.12 * (x[None, :] - P)]
    w1 = np.clip(0.5 * (1 + (x - (1 + 0.5 / 15)) / (2 / 15)), 0, 1)[None, :]
    want = (1 - w1) * planes[0] + w1 * planes[1]
    frac = (want * 255 + 0.5) % 1.0
    sure = (frac > 1e-3) & (frac < 1 - 1e-3)
    assert sure.mean() > 0.98
    assert np.abs(out - np.rint(want * 255) / 255)[sure].max() < 1e-6
    outside = (w1[0] == 0) | (w1[0] == 1)                                    # 2 source pixels = 6 samples on either side
    assert outside.sum() == 96 - 12
    assert np.array_equal(out[:, outside].view(np.uint32), plain[:, outside].view(np.uint32))
    for g in range(2):
        cols = outside & ((np.arange(96) // 48) == g)
        fr = (planes[g] * 255 + 0.5) % 1.0
        ok = ((fr > 1e-3) & (fr < 1 - 1e-3))[:, cols]
        assert np.abs(out[:, cols] - np.rint(planes[g][:, cols] * 255) / 255)[ok].max() < 1e-6
    step = np.abs(np.diff(out, axis=1))                                      # step[:, j]: between samples j and j + 1
    seam, inside = step[:, 47].max(), step[:, 42:53].max()
    jump = np.abs(np.diff(plain, axis=1))[:, 47].max()
    print(f"largest step across the seam: blend = 2 {seam:.5f} (largest inside the band {inside:.5f}); blend = 0 {jump:.5f}")
    assert seam <= np.delete(step[:, 42:53], 5, axis=1).max() + 1 / 255 + 1e-6
    assert jump > 0.1


# ---------------------------------------------------------------------------------------------------------------
# 4. shards and bounds, argument checks with a handle
# ---------------------------------------------------------------------------------------------------------------
SENT = -7.0


@pytest.mark.parametrize("i", [1, 4, 6], ids=[IDS[i] for i in [1, 4, 6]])
def test_shards_and_bounds(i):
    from steered_mixture_of_experts_amd import _lib
    shape, C_, kpd, m, beta, kw = CASES[i][:6]
    cfg, p, K, active, grid, tabs, ref, _ = _inputs(i)
    B = int(np.prod(grid))
    eng = _engine(shape, C_, K, use_yuv=(C_ == 3), **kw)
    dp, act, axes = _to_dev(p), _bits(active), _dev_axes(tabs)
    extent = [g * mm - max(1, mm // 3) for g, mm in zip(grid, m)]            # a ragged extent is cropped
    ishape = tuple(extent) + (C_,)
    buf, view = _guarded(ishape, torch.float32, SENT)
    eng.render_blend(dp, act, axes, grid, extent, beta, out=view)
    torch.cuda.synchronize()
    whole = view.cpu().numpy().copy()
    flat = buf.cpu().numpy()
    assert (flat[:64] == SENT).all() and (flat[64 + whole.size:] == SENT).all() and (whole != SENT).all()
    # several ranges into one (misaligned) buffer == one call; each call writes exactly its blocks' positions
    buf2, view2 = _guarded(ishape, torch.float32, SENT, shift=1)
    written = np.zeros(tuple(extent), bool)
    for first, count in [(0, 5), (5, 1), (6, B - 6)]:
        eng.render_blend(dp, act, axes, grid, extent, beta, first_block=first, num_blocks=count, out=view2)
        torch.cuda.synchronize()
        written |= _owned(m, grid, extent, first, count)
        part = view2.cpu().numpy()
        assert (part[written] != SENT).all() and (part[~written] == SENT).all(), (first, count)
    assert np.array_equal(view2.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    f2 = buf2.cpu().numpy()
    assert (f2[:65] == SENT).all() and (f2[65 + whole.size:] == SENT).all()
    # uint8 and the argmax plane through the C entry, guarded and misaligned
    lib = _lib.load()
    cp = eng._cparams(dp)
    d = len(shape)
    t3 = (C.c_void_p * 3)(*([t.data_ptr() for t in axes] + [None] * (3 - d)))
    m3 = (C.c_int32 * 3)(*(list(m) + [1] * (3 - d)))
    g3 = (C.c_int32 * 3)(*(list(grid) + [1] * (3 - d)))
    e3 = (C.c_int64 * 3)(*(list(extent) + [1] * (3 - d)))
    bl = [float(v) for v in np.atleast_1d(beta)]
    b3 = (C.c_float * 3)(*((bl * d if len(bl) == 1 else bl) + [0.0] * (3 - d)))
    bufu, viewu = _guarded(ishape, torch.uint8, 201, shift=3)
    abuf, aview = _guarded(tuple(extent), torch.uint8, 77, shift=5)

    def call(first=0, count=B, params=cp, blend=b3, image=viewu, e_=e3, fmt=1):
        return lib.smoe_render_blend(eng._h, first, count, None if params is None else C.byref(params), C.c_void_p(act.data_ptr()),
                                     t3, m3, g3, e_, blend, None if image is None else C.c_void_p(image.data_ptr()), fmt,
                                     C.c_void_p(aview.data_ptr()), None)

    assert call(0, 7) == 0 and call(7, B - 7) == 0, lib.smoe_last_error()
    torch.cuda.synchronize()
    fu, fa = bufu.cpu().numpy(), abuf.cpu().numpy()
    assert (fu[:67] == 201).all() and (fu[67 + whole.size:] == 201).all()
    assert np.array_equal(viewu.cpu().numpy(), np.rint(whole * 255).astype(np.uint8))
    assert (fa[:69] == 77).all() and (fa[69 + aview.numel():] == 77).all()
    _, am = eng.render(dp, act, axes, grid, extent, want_argmax=True)
    assert torch.equal(aview, am)
    # invalid arguments with a real handle: SMOE_ERR_INVALID, the argument named, nothing written
    viewu.fill_(201)
    aview.fill_(77)
    nan3 = (C.c_float * 3)(float("nan"), 0.0, 0.0)
    neg3 = (C.c_float * 3)(1.0, -0.5, 0.0)
    big3 = (C.c_float * 3)(1.0, shape[1] / 2 + 0.01, 0.0)
    zero_e = (C.c_int64 * 3)(*([0] + list(extent[1:]) + [1] * (3 - d)))
    for kwargs, word in [(dict(blend=None), b"blend"), (dict(blend=nan3), b"blend[0]"), (dict(blend=neg3), b"blend[1]"),
                         (dict(blend=big3), b"blend[1]"), (dict(params=None), b"p "), (dict(image=None), b"image"),
                         (dict(first=1), b"first_block"), (dict(e_=zero_e), b"extent"), (dict(fmt=7), b"image_format")]:
        assert call(**kwargs) == _lib.SMOE_ERR_INVALID, kwargs
        assert word in lib.smoe_last_error(), (kwargs, lib.smoe_last_error())
    torch.cuda.synchronize()
    assert (bufu == 201).all() and (abuf == 77).all()
    assert lib.smoe_abi_version() == 2
    eng.close()


def test_facade_blend_on_the_device():
    """Smoe.render(blend=) on the device equals the engine's render_blend, leaves blend = 0 as it was, and changes only
    samples within the band."""
    from steered_mixture_of_experts_amd.smoe import Adam, Smoe
    img = _image(40, 52, C_=3, seed=3)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(4, val_iter=4)
    s.get_reconstruction()
    base = s.render(scale=2, to_host=False)
    assert torch.equal(s.render(scale=2, blend=0, to_host=False), base)
    out, ids = s.render(scale=2, blend=(1, 2), to_host=False, want_argmax=True)
    axes = _dev_axes(_axes((16, 16), (32, 32)))
    direct = s._engine.render_blend(s._params, s._render_lists(False), axes, s.grid, (80, 104), (1, 2))
    torch.cuda.synchronize()
    assert torch.equal(out, direct) and not torch.equal(out, base)
    assert torch.equal(ids, s.render(scale=2, to_host=False, want_argmax=True)[1])
    u8 = s.render(scale=2, blend=(1, 2), dtype=np.uint8)
    assert np.array_equal(u8, np.rint(out.cpu().numpy() * 255).astype(np.uint8))
