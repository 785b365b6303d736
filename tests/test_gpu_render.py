"""GPU tests of the decoder (smoe_render through the C ABI): bit-identity with smoe_forward on the training lattice,
parity with the CPU restatement on resampled grids, uint8 output, shards / bounds / argument checks, and the facade.

Criterion on resampled grids = the project's existing one for ``recon`` (tests/test_gpu_parity.py): with
``frac = (clip(y64, 0, 1) * 255 + 0.5) mod 1`` from the float64 restatement, values are identical (< 1e-7) where ``frac`` is
farther than 2e-4 from 0 / 1, differ by at most one LSB elsewhere, and the tie share stays below 0.01.  A sample on which
some kernel's float64 gate lies within 1e-6 of the influence threshold may have that kernel masked differently: judged by
the one-LSB bound only, counted towards the same cap."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import smoe_oracle as o
from render_cases import _axes, _bits, _dev_axes, _engine, _guarded, _image, _lattice, _owned, _setup, _to_dev
from render_engine import oracle_blocks, place_blocks
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks

pytestmark = pytest.mark.gpu

SHAPES = [
    # block_shape, C, kernels_per_dim, use_yuv  (the list of tests/test_gpu_parity.py)
    ((16, 16), 1, [2, 2], False),
    ((16, 16), 3, [2, 2], True),
    ((32, 32), 3, [2, 4], True),
    ((16, 16, 4), 3, [2, 2, 1], True),
    ((16, 16), 1, [2, 4], False),
    ((7, 5), 1, [2, 2], False),
    ((12, 10, 3), 3, [2, 2, 1], True),
]
B37 = 37


def _ids(cases):
    return ["x".join(map(str, c[0])) + f"-c{c[1]}" + "".join(f"-{x}" for x in c[4:] if isinstance(x, str)) for c in cases]


def _parity_inputs(shape, C_, kpd, yuv, **cfgkw):
    cfg, p, tgt, K = _setup(shape, C_, kpd, yuv, B37, 100 + len(shape) + C_, **cfgkw)
    active = np.random.default_rng(5).uniform(size=(B37, K)) < 0.85
    p["pis"][3, 0] = 0.0
    p["pis"][4, K - 1] = -0.1
    return cfg, p, tgt, K, active


def _grid_of(shape):
    return (5, 8) if len(shape) == 2 else (5, 4, 2)


# ---------------------------------------------------------------------------------------------------------------
# 4. identity with smoe_forward on the training lattice
# ---------------------------------------------------------------------------------------------------------------
OPTIONS = [
    ("train_inverse_cov", dict(train_inverse_cov=True)),
    ("radial_as", dict(radial_as=True)),
    ("no_determinant", dict(use_determinant=False)),
    ("only_y_gamma", dict(only_y_gamma=True)),
    ("quantize_pis", dict(quantize_pis=True)),
    ("mode2", dict(quantization_mode=2, quantize_pis=True, bit_depths=(14, 12, 8, 10, 10), lower_bounds=(-60, -.3, -1, 0, -4),
                   upper_bounds=(60, 1.3, 2, 2, 4))),
    ("mode3", dict(quantization_mode=3, quantize_pis=True, bit_depths=(14, 12, 8, 10, 10), lower_bounds=(-60, -.3, -1, 0, -4),
                   upper_bounds=(60, 1.3, 2, 2, 4))),
    ("mode2_centre_grid", dict(quantization_mode=2, quantize_pis=True, bit_depths=(14, 10, 8, 10, 10),
                               lower_bounds=(-60, -.06, -1, 0, -4), upper_bounds=(60, .08, 2, 2, 4))),
]
IDENTITY = [s + ("plain", {}) for s in SHAPES] + [SHAPES[1] + (name, kw) for name, kw in OPTIONS]


@pytest.mark.parametrize("case", IDENTITY, ids=_ids(IDENTITY))
def test_identity_with_forward(case):
    shape, C_, kpd, yuv, name, kw = case
    d = len(shape)
    cfg, p, tgt, K, active = _parity_inputs(shape, C_, kpd, yuv)
    if kw.get("train_inverse_cov"):                      # keep the matrices positive definite (tests/test_gpu_invcov.py)
        p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
        p["A_corr"] = (p["A_corr"] * 2.0).astype(np.float32)
    if kw.get("quantization_mode", 0) == 3:              # mode 3 assumes A_corr zero on and above the diagonal
        p["A_corr"] = p["A_corr"] * np.tril(np.ones((d, d), np.float32), -1)
    eng = _engine(shape, C_, K, use_yuv=yuv, **kw)
    gdev = None
    if name == "mode2_centre_grid":
        grid_mu = o.init_params(tgt.reshape((B37,) + tuple(shape) + (C_,)), kpd)["musX"].astype(np.float32)
        off = np.random.default_rng(4).uniform(-0.05, 0.05, size=grid_mu.shape).astype(np.float32)
        p["musX"] = (grid_mu + off).astype(np.float32)
        gdev = torch.from_numpy(grid_mu).cuda()
        eng.set_center_grid(gdev)
    dp = _to_dev(p)
    act = _bits(active)
    T = torch.from_numpy(np.ascontiguousarray(np.transpose(tgt, (0, 2, 1)))).cuda()
    fw = eng.forward(T, dp, act, want_recon=True, want_argmax=True, update_active=False)
    grid = _grid_of(shape)
    extent = [g * n - max(1, n // 3) for g, n in zip(grid, shape)]       # cuts into the last block row / column
    img, am = eng.render(dp, act, _dev_axes(_axes(shape, shape)), grid, extent, want_argmax=True)
    torch.cuda.synchronize()
    img, am = img.cpu().numpy(), am.cpu().numpy()
    recon = blk.from_planar(fw["recon"].cpu().numpy(), shape).reshape(B37, -1, C_)
    want = place_blocks(recon, shape, grid, extent, 0, np.zeros(tuple(extent) + (C_,), np.float32))
    want_am = place_blocks(fw["argmax"].cpu().numpy().reshape(B37, -1, 1), shape, grid, extent, 0,
                           np.full(tuple(extent) + (1,), 255, np.uint8))[..., 0]
    own = _owned(shape, grid, extent, 0, B37)
    assert own.any() and not own.all()
    assert np.array_equal(img.view(np.uint32)[own], want.view(np.uint32)[own])          # bit for bit
    assert not (am[own] == 255).any()
    assert np.array_equal(am[own], want_am[own])
    assert (img[~own] == 0).all() and (am[~own] == 255).all()                           # absent blocks: untouched
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. + 6. parity with the restatement on resampled grids, uint8 output
# ---------------------------------------------------------------------------------------------------------------
RESAMPLED = [
    ((16, 16), 1, [2, 2], False, (32, 32), {}),
    ((16, 16), 3, [2, 2], True, (40, 24), {}),
    ((32, 32), 3, [2, 4], True, (48, 80), {}),
    ((16, 16, 4), 3, [2, 2, 1], True, (32, 32, 7), {}),
    ((7, 5), 1, [2, 2], False, (11, 16), {}),
    ((12, 10, 3), 3, [2, 2, 1], True, (6, 5, 9), {}),
    ((16, 16), 3, [2, 2], True, (40, 24), dict(train_inverse_cov=True)),
    ((7, 5), 1, [2, 2], False, (3, 300), {}),    # 300 > 256 innermost samples: CL = 256, two passes, the second ragged
    # off the 8-bit lattice (nudged_max, inv_scale and the influence threshold follow the precision): 1 023 and 63 levels
    ((16, 16), 3, [2, 2], True, (40, 24), dict(precision=10)),
    ((16, 16), 3, [2, 2], True, (40, 24), dict(precision=6)),
]


def _tag(kw):
    return "".join("-ic" if k == "train_inverse_cov" else f"-p{v}" for k, v in kw.items())


@pytest.mark.parametrize("case", RESAMPLED, ids=["x".join(map(str, c[0])) + "-c%d-to-" % c[1] + "x".join(map(str, c[4]))
                                                 + _tag(c[5]) for c in RESAMPLED])
def test_parity_on_resampled_grids(case):
    shape, C_, kpd, yuv, m, kw = case
    cfg, p, tgt, K, active = _parity_inputs(shape, C_, kpd, yuv, **kw)
    if kw.get("train_inverse_cov"):
        p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
        p["A_corr"] = (p["A_corr"] * 2.0).astype(np.float32)
    judge_resampled(shape, C_, yuv, m, kw, cfg, p, K, active, _grid_of(shape))


def judge_resampled(shape, C_, yuv, m, kw, cfg, p, K, active, grid):
    """the criterion of the module's docstring for the first ``len(active)`` blocks of ``grid`` rendered at ``m`` samples per
    block: the condition on the inputs from the restatement alone, then the kernel"""
    B = len(active)
    tabs = _axes(shape, m)
    ref, _ = oracle_blocks(p, active, tabs, cfg, np.float32)
    ref64, _ = oracle_blocks(p, active, tabs, cfg, np.float64)
    levels, tau, band = _lattice(cfg.precision)
    lsb = 1.0 / levels
    frac = (np.clip(ref64["y"], 0, 1) * levels + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    near_tau = (np.abs(ref64["w"] - tau) < band).any(axis=1)[..., None]                 # (B, M, 1)
    loose = tie | near_tau
    # condition on the inputs: the restatement itself has few ties and no fp32-vs-fp64 difference outside them
    print(f"oracle: tie share {tie.mean():.2e}, near-threshold gate entries {(np.abs(ref64['w'] - tau) < band).mean():.2e}, "
          f"loose share {loose.mean():.2e}")
    assert loose.mean() < 0.01
    assert (np.abs(ref["recon"] - ref64["recon"])[~np.broadcast_to(loose, tie.shape)] < 1e-7).all()

    eng = _engine(shape, C_, K, use_yuv=yuv, **kw)
    dp = _to_dev(p)
    act = _bits(active)
    extent = [g * mm for g, mm in zip(grid, m)]
    axes = _dev_axes(tabs)
    img = eng.render(dp, act, axes, grid, extent)
    u8 = eng.render(dp, act, axes, grid, extent, dtype=torch.uint8) if cfg.precision <= 8 else None     # (refused above 8 bits)
    torch.cuda.synchronize()
    img = img.cpu().numpy()
    own = _owned(m, grid, extent, 0, B)
    want = place_blocks(ref["recon"].astype(np.float32), m, grid, extent, 0, np.zeros(tuple(extent) + (C_,), np.float32))
    loose_img = place_blocks(np.broadcast_to(loose, tie.shape), m, grid, extent, 0, np.zeros(tuple(extent) + (C_,), bool))
    dd = np.abs(img - want)[own]
    lo = loose_img[own]
    print(f"kernel: max difference outside ties {dd[~lo].max():.3e}, overall {dd.max():.3e}, "
          f"samples that differ {(dd > 1e-7).mean():.2e}")
    assert (dd[~lo] < 1e-7).all(), dd[~lo].max()
    assert (dd <= lsb * 1.0001).all(), dd.max()
    # 6. uint8 = the lattice index of the fp32 image
    if u8 is not None:
        assert np.array_equal(u8.cpu().numpy(), np.rint(img * levels).astype(np.uint8))
    assert np.abs(img * levels - np.rint(img * levels)).max() < 1e-3                   # on the lattice of this precision
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. shards and bounds
# ---------------------------------------------------------------------------------------------------------------
SENT = -7.0


@pytest.mark.parametrize("shape,C_,kpd,yuv,m", [((16, 16), 3, [2, 2], True, (16, 16)), ((16, 16), 1, [2, 2], False, (24, 20)),
                                               ((16, 16, 4), 3, [2, 2, 1], True, (16, 16, 7))],
                         ids=["16x16-c3", "16x16-c1-to-24x20", "16x16x4-c3-to-16x16x7"])
def test_shards_and_bounds(shape, C_, kpd, yuv, m):
    cfg, p, tgt, K, active = _parity_inputs(shape, C_, kpd, yuv)
    active[7] = False                                        # a block with no live kernel
    eng = _engine(shape, C_, K, use_yuv=yuv)
    dp = _to_dev(p)
    act = _bits(active)
    grid = _grid_of(shape)
    extent = [g * mm - max(1, mm // 3) for g, mm in zip(grid, m)]
    axes = _dev_axes(_axes(shape, m))
    ishape = tuple(extent) + (C_,)
    own = _owned(m, grid, extent, 0, B37)

    def run(first, count, shift=0, with_act=True, dtype=torch.float32):
        sub = {k: v[first:first + count].contiguous() for k, v in dp.items()}
        fill = SENT if dtype == torch.float32 else 201
        buf, view = _guarded(ishape, dtype, fill, shift=shift)
        abuf, aview = _guarded(tuple(extent), torch.uint8, 77, shift=shift)
        return buf, view, abuf, aview, sub, (act[first:first + count].contiguous() if with_act else None)

    buf, view, abuf, aview, sub, a = run(0, B37)
    eng.render(sub, a, axes, grid, extent, out=view, want_argmax=False)
    # the engine allocates the argmax plane itself: drive the C entry for a guarded one below; here the image
    torch.cuda.synchronize()
    whole = view.cpu().numpy().copy()
    flat = buf.cpu().numpy()
    assert (flat[:64] == SENT).all() and (flat[64 + whole.size:] == SENT).all()         # guard band
    assert (whole[own] != SENT).all() and (whole[~own] == SENT).all()                    # exactly the owned positions
    # two shards == one call, bit for bit; an unaligned image takes the element-wise path to the same result
    h = 19
    buf2, view2, _, _, sub_a, a_a = run(0, h, shift=1)
    eng.render(sub_a, a_a, axes, grid, extent, first_block=0, out=view2)
    _, _, _, _, sub_b, a_b = run(h, B37 - h)
    eng.render(sub_b, a_b, axes, grid, extent, first_block=h, out=view2)
    torch.cuda.synchronize()
    assert np.array_equal(view2.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    f2 = buf2.cpu().numpy()
    assert (f2[:65] == SENT).all() and (f2[65 + whole.size:] == SENT).all()
    # uint8 with guard band
    bufu, viewu, _, _, sub, a = run(0, B37, dtype=torch.uint8)
    eng.render(sub, a, axes, grid, extent, out=viewu, dtype=torch.uint8)
    torch.cuda.synchronize()
    u = viewu.cpu().numpy()
    fu = bufu.cpu().numpy()
    assert (fu[:64] == 201).all() and (fu[64 + u.size:] == 201).all()
    assert np.array_equal(u[own], np.rint(whole[own] * 255).astype(np.uint8)) and (u[~own] == 201).all()
    # argmax plane through the C entry with a guarded buffer
    from steered_mixture_of_experts_amd import _lib
    lib = _lib.load()
    cp = eng._cparams(sub)
    tabs = (C.c_void_p * 3)(*([t.data_ptr() for t in axes] + [None] * (3 - len(shape))))
    m3 = (C.c_int32 * 3)(*(list(m) + [1] * (3 - len(shape))))
    g3 = (C.c_int32 * 3)(*(list(grid) + [1] * (3 - len(shape))))
    e3 = (C.c_int64 * 3)(*(list(extent) + [1] * (3 - len(shape))))
    buf3, view3, abuf, aview, _, _ = run(0, B37)

    def call(first=0, count=B37, params=cp, tabs_=tabs, m_=m3, g_=g3, e_=e3, image=view3, fmt=0):
        return lib.smoe_render(eng._h, first, count, None if params is None else C.byref(params), C.c_void_p(a.data_ptr()),
                               tabs_, m_, g_, e_, None if image is None else C.c_void_p(image.data_ptr()), fmt,
                               C.c_void_p(aview.data_ptr()), None)

    assert call() == 0, lib.smoe_last_error()
    torch.cuda.synchronize()
    am = aview.cpu().numpy()
    fa = abuf.cpu().numpy()
    assert (fa[:64] == 77).all() and (fa[64 + am.size:] == 77).all() and (am[~own] == 77).all()
    assert np.array_equal(view3.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    dead = _owned(m, grid, extent, 7, 1)
    assert (am[dead] == 255).all() and (whole[dead] == 0).all()                          # no live kernel: 0, marker 255
    assert (am[own & ~dead] < K).mean() > 0.99
    # active = NULL equals an all-ones mask
    ones = torch.full((B37,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    r1 = eng.render(sub, ones, axes, grid, extent)
    r0 = eng.render(sub, None, axes, grid, extent)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1)
    # invalid arguments: SMOE_ERR_INVALID, the message names the argument, nothing is written
    view3.fill_(SENT)
    aview.fill_(77)
    bad_tabs = (C.c_void_p * 3)(*([axes[0].data_ptr()] + [None] * 2))
    bad_m = (C.c_int32 * 3)(*([m[0], 0] + [1] * 1))
    big_e = (C.c_int64 * 3)(*([extent[0], grid[1] * m[1] + 1] + list(extent[2:]) + [1] * (3 - len(shape))))
    zero_e = (C.c_int64 * 3)(*([0] + list(extent[1:]) + [1] * (3 - len(shape))))
    total = int(np.prod(grid))
    for kwargs, word in [(dict(params=None), b"p "), (dict(image=None), b"image"), (dict(tabs_=bad_tabs), b"axis_coords"),
                         (dict(m_=bad_m), b"samples"), (dict(first=total - B37 + 1), b"first_block"),
                         (dict(e_=big_e), b"extent"), (dict(e_=zero_e), b"extent"), (dict(fmt=7), b"image_format")]:
        assert call(**kwargs) == _lib.SMOE_ERR_INVALID, kwargs
        assert word in lib.smoe_last_error(), (kwargs, lib.smoe_last_error())
    torch.cuda.synchronize()
    assert (buf3 == SENT).all() and (abuf == 77).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. the facade on the device
# ---------------------------------------------------------------------------------------------------------------
def test_facade_render_on_the_device():
    from steered_mixture_of_experts_amd.smoe import Adam, Smoe
    img = _image(40, 52, C_=3, seed=3)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, use_yuv=True,
             quantization_mode=1)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(4, val_iter=4)
    rec = s.get_reconstruction()
    assert np.array_equal(s.render(scale=1).view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(s.render(scale=1, dtype=np.uint8), np.rint(rec * 255).astype(np.uint8))
    for scale, m, ext in [(2, (32, 32), (80, 104)), ((1.5, 2), (24, 32), (60, 104))]:
        out = s.render(scale=scale, to_host=False)
        assert tuple(out.shape) == ext + (3,) and out.is_cuda
        axes = _dev_axes(_axes((16, 16), m))
        direct = s._engine.render(s._params, s._recon_active, axes, s.grid, ext)
        torch.cuda.synchronize()
        assert torch.equal(out, direct)
    _, ids = s.render(scale=1, want_argmax=True)
    am = s.get_weight_matrix_argmax()
    assert ((ids == am) | (ids == -1)).all() and (ids >= 0).mean() > 0.99
    if s.rparams is None:
        s._quantize()
    s.run_batched(train=False, update_reconstruction=True, with_quantized_params=True)
    assert np.array_equal(s.render(scale=1, quantized=True).view(np.uint32), s.get_qreconstruction().view(np.uint32))
    # video
    b = synthetic_blocks(8, (16, 16, 4), 3, 11)
    vid = blk.blocks_to_image(b, (32, 32, 8), (16, 16, 4))[:27, :, :7]
    v = Smoe(vid, train_inverse_cov=False, kernels_per_dim=[2, 2, 1], batch_size=[16, 16, 4], use_determinant=True)
    assert np.array_equal(v.render(scale=1).view(np.uint32), v.get_reconstruction().view(np.uint32))
    assert v.render(samples_per_block=(16, 16, 7)).shape == (27, 32, 12, 3)


def test_facade_render_is_centred():
    """K = 1 per block, y = nu + gamma . x inside (0, 1) and gate exactly 1: the 3x render is the plane at render_axis'
    coordinates, away from rounding ties."""
    from steered_mixture_of_experts_amd.smoe import Smoe
    img = np.full((16, 32, 1), 0.5, dtype=np.float32)
    s0 = Smoe(img, train_inverse_cov=False, kernels_per_dim=[1, 1], batch_size=[16, 16], use_determinant=True)
    p = s0.get_params()
    nu, g0, g1 = 0.31, 0.23, 0.37
    p["nu_e"][:] = nu
    p["gamma_e"][:, :, 0, 0] = g0
    p["gamma_e"][:, :, 1, 0] = g1
    s = Smoe(img, train_inverse_cov=False, init_params=p, batch_size=[16, 16], use_determinant=True)
    out = s.render(scale=3)
    u = blk.render_axis(16, 48).astype(np.float64)
    y = nu + g0 * u[:, None] + g1 * u[None, :]
    frac = (y * 255 + 0.5) % 1.0
    sure = (frac > 1e-3) & (frac < 1 - 1e-3)
    want = np.rint(255 * y) / 255
    assert out.shape == (48, 96, 1) and sure.mean() > 0.98
    for gx in range(2):
        assert np.abs(out[:, gx * 48:(gx + 1) * 48, 0] - want)[sure].max() < 1e-6
