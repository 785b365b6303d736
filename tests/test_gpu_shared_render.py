"""GPU tests of the shared-mode decoder (smoe_shared_render through the C ABI): bit-identity with smoe_shared_forward on the
training lattice, parity with the CPU restatement on resampled grids, uint8 output, shards / bounds / workgroup split,
batches larger than smoe_shared_forward can take, and the facade.

Criterion on resampled grids = tests/test_gpu_render.py's: with ``frac = (clip(y64, 0, 1) * 255 + 0.5) mod 1`` from the
float64 restatement, values are identical (< 1e-7) where ``frac`` is farther than 2e-4 from 0 / 1 and no float64 gate lies
within 1e-6 of the influence threshold; at most one LSB elsewhere; the share of such loose samples is capped at 0.01 -- a
condition on the inputs that the restatement alone has to meet first."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import smoe_oracle as o
from render_cases import _bits, _dev_axes, _guarded, _owned
from render_engine import place_blocks
from shared_render_engine import OracleSharedRenderEngine, ids_of, oracle_shared_batches
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks

pytestmark = pytest.mark.gpu

IMAGES = [
    # image shape, batch shape, C, kernels per dim
    ((64, 96), (16, 16), 1, [6, 8]),
    ((64, 96), (32, 32), 3, [6, 8]),
    ((48, 64), (16, 32), 3, [12, 12]),           # K = 144 > SH_KC: several staging chunks, five list words
    ((32, 48, 8), (16, 16, 4), 3, [4, 4, 2]),
    ((21, 25), (7, 5), 1, [3, 3]),               # ragged tiles
]
QKW = dict(quantize_pis=True, bit_depths=(14, 12, 8, 10, 10), lower_bounds=(-60, -.3, -1, 0, -4), upper_bounds=(60, 1.3, 2, 2, 4))
OPTIONS = [
    ("train_inverse_cov", dict(train_inverse_cov=True)),
    ("radial_as", dict(radial_as=True)),
    ("no_determinant", dict(use_determinant=False)),
    ("only_y_gamma", dict(only_y_gamma=True)),
    ("quantize_pis", dict(quantize_pis=True)),
    ("mode2", dict(quantization_mode=2, **QKW)),
    ("mode3", dict(quantization_mode=3, **QKW)),
    ("mode2_centre_grid", dict(quantization_mode=2, quantize_pis=True, bit_depths=(14, 10, 8, 10, 10),
                               lower_bounds=(-60, -.06, -1, 0, -4), upper_bounds=(60, .08, 2, 2, 4))),
]
EMPTY = 2                                        # the batch whose list is empty


def _name(c):
    return "x".join(map(str, c[0])) + f"-c{c[2]}-b" + "x".join(map(str, c[1]))


def _grid(shape, bshape):
    return [s // b for s, b in zip(shape, bshape)]


def _setup(shape, bshape, C_, kpd, name="plain", **kw):
    """perturbed initialisation as tests/test_gpu_render.py::_setup draws it, on the global kernel set"""
    d = len(shape)
    seed = 300 + d + C_
    img = synthetic_blocks(1, shape, C_, seed)[0]
    p = o.shared_init_params(img, kpd)
    K = p["pis"].shape[1]
    rng = np.random.default_rng(seed + 1)
    p["A_corr"] = (rng.normal(size=p["A_corr"].shape) * 1.5).astype(np.float32)
    p["A_diagonal"] = (p["A_diagonal"] + rng.normal(size=p["A_diagonal"].shape)).astype(np.float32)
    p["gamma_e"] = (rng.normal(size=p["gamma_e"].shape) * 0.1).astype(np.float32)
    grid_mu = p["musX"].copy()
    p["musX"] = (p["musX"] + rng.normal(size=p["musX"].shape) * 0.02).astype(np.float32)
    p["pis"] = (p["pis"] * rng.uniform(0.5, 1.5, size=p["pis"].shape)).astype(np.float32)
    p["pis"][0, 0] = 0.0
    p["pis"][0, K - 1] = -0.1
    if kw.get("train_inverse_cov"):                      # keep the matrices positive definite
        p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
    if kw.get("quantization_mode", 0) == 3:              # mode 3 assumes A_corr zero on and above the diagonal
        p["A_corr"] = p["A_corr"] * np.tril(np.ones((d, d), np.float32), -1)
    if kw.get("radial_as"):                              # one steering value per kernel
        p["A_diagonal"] = np.ascontiguousarray(p["A_diagonal"][:, :, :1, :1] * np.eye(d, dtype=np.float32))
    cfg = o.OracleConfig(block_shape=bshape, channels=C_, kernels=K, use_yuv=(C_ == 3), **kw)
    mus_grid = None
    if name == "mode2_centre_grid":
        off = np.random.default_rng(4).uniform(-0.05, 0.05, size=grid_mu.shape).astype(np.float32)
        p["musX"] = (grid_mu + off).astype(np.float32)
        mus_grid = np.ascontiguousarray(grid_mu[0])
        cfg.mus_grid = grid_mu
    NB = int(np.prod(_grid(shape, bshape)))
    lists = np.random.default_rng(5).uniform(size=(NB, K)) < 0.85
    lists[EMPTY] = False
    return img, p, cfg, K, NB, lists, mus_grid


def _engine(shape, bshape, C_, K, mus_grid=None, **kw):
    from steered_mixture_of_experts_amd.engine import SharedConfig, SharedEngine
    eng = SharedEngine(SharedConfig(image_shape=shape, batch_shape=bshape, channels=C_, kernels=K, use_yuv=(C_ == 3), **kw))
    if mus_grid is not None:
        eng._test_grid = torch.from_numpy(mus_grid).cuda()
        eng.set_center_grid(eng._test_grid)
    return eng


def _dev(p):
    return {k: torch.from_numpy(np.ascontiguousarray(v[0])).cuda() for k, v in p.items()}


def _dev_lists(mask):
    return _bits(mask, words=True)


def _tables(shape, extent):
    return [blk.render_axis(n, e) for n, e in zip(shape, extent)]


# ---------------------------------------------------------------------------------------------------------------
# 7. identity with smoe_shared_forward on the training lattice
# ---------------------------------------------------------------------------------------------------------------
IDENTITY = [c + ("plain", {}) for c in IMAGES] + [IMAGES[1] + (n, kw) for n, kw in OPTIONS]


@pytest.mark.parametrize("case", IDENTITY, ids=[_name(c) + "-" + c[4] for c in IDENTITY])
def test_identity_with_shared_forward(case):
    shape, bshape, C_, kpd, name, kw = case
    img, p, cfg, K, NB, lists, mus_grid = _setup(shape, bshape, C_, kpd, name, **kw)
    eng = _engine(shape, bshape, C_, K, mus_grid, **kw)
    dp, dl = _dev(p), _dev_lists(lists)
    tb, _ = blk.image_to_blocks(img, bshape)
    T = torch.from_numpy(blk.to_planar(tb)).cuda()
    fw = eng.forward(T, dp, dl, want_recon=True, want_argmax=True, update_lists=False)
    out, ids = eng.render(dp, dl, _dev_axes(_tables(shape, shape)), bshape, want_argmax=True)
    torch.cuda.synchronize()
    out, ids = out.cpu().numpy(), ids.cpu().numpy()
    want = blk.blocks_to_image(blk.from_planar(fw["recon"].cpu().numpy(), bshape), shape, bshape)
    am = fw["argmax"].cpu().numpy().reshape((NB,) + tuple(bshape) + (1,))
    want_ids = blk.blocks_to_image(am, shape, bshape)[..., 0]
    assert out.shape == want.shape and out.dtype == np.float32
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))                     # bit for bit
    have = ids >= 0
    assert np.array_equal(ids[have], want_ids[have])
    dead = _owned(bshape, _grid(shape, bshape), shape, EMPTY, 1)
    assert (ids[dead] == -1).all() and (out[dead] == 0).all()                            # the empty list: 0, marker -1
    assert have[~dead].mean() > 0.99
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. parity with the restatement on resampled grids, uint8 output
# ---------------------------------------------------------------------------------------------------------------
RESAMPLED = [
    (IMAGES[0], (32, 32), {}, True),
    (IMAGES[1], (80, 48), {}, True),
    (IMAGES[2], (24, 40), {}, True),
    (IMAGES[3], (32, 32, 7), {}, True),
    (IMAGES[4], (11, 16), {}, True),
    (IMAGES[1], (80, 48), dict(train_inverse_cov=True), True),
    (IMAGES[0], (32, 32), {}, False),                                  # use_lists=False: no lists at all
]
TAU = 0.5 / 256


def _reference(image, m, kw, use_lists, first=0, count=None):
    """the float32 / float64 restatement of the batches [first, first + count) and the loose set; asserts the conditions
    the inputs have to meet by themselves"""
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, mus_grid = _setup(shape, bshape, C_, kpd, **kw)
    grid = _grid(shape, bshape)
    count = NB - first if count is None else count
    mask = (lists if use_lists else np.ones_like(lists))[first:first + count]
    tabs = _tables(shape, [g * v for g, v in zip(grid, m)])
    ref = oracle_shared_batches(p, mask, tabs, m, grid, first, cfg, np.float32)
    ref64 = oracle_shared_batches(p, mask, tabs, m, grid, first, cfg, np.float64)
    frac = (np.clip(ref64["y"], 0, 1) * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    near_tau = (np.abs(ref64["w"] - TAU) < 1e-6).any(axis=1)[..., None]                  # (nb, M, 1)
    loose = np.broadcast_to(tie | near_tau, tie.shape)
    none = ~(ref64["wt"] > 0).any(axis=1)                                                # (nb, M): samples without any influence
    live = [b for b in range(count) if mask[b].any()]
    d32 = np.abs(ref["recon"] - ref64["recon"])[~loose]
    print(f"oracle: tie share {tie.mean():.2e}, loose share {loose.mean():.2e}, fp32 vs fp64 outside the loose set "
          f"{d32.max():.2e}, samples without influence in batches with a list {none[live].mean() if live else 0.0:.2e}")
    assert loose.mean() < 0.01
    assert (d32 < 1e-7).all()
    return dict(p=p, cfg=cfg, K=K, NB=NB, lists=lists, grid=grid, tabs=tabs, ref=ref, ref64=ref64, loose=loose)


def _assert_parity(got, R, m, first, count, C_):
    """criterion 8 on the positions of the batches [first, first + count)"""
    grid = R["grid"]
    extent = [g * v for g, v in zip(grid, m)]
    own = _owned(m, grid, extent, first, count)
    want = place_blocks(R["ref"]["recon"].astype(np.float32), m, grid, extent, first, np.zeros(tuple(extent) + (C_,), np.float32))
    loose_img = place_blocks(R["loose"], m, grid, extent, first, np.zeros(tuple(extent) + (C_,), bool))
    dd = np.abs(got - want)[own]
    lo = loose_img[own]
    print(f"kernel: max difference outside the loose set {dd[~lo].max():.3e}, overall {dd.max():.3e}, "
          f"samples that differ {(dd > 1e-7).mean():.2e}")
    assert (dd[~lo] < 1e-7).all(), dd[~lo].max()
    assert (dd <= 1.0001 / 255).all(), dd.max()


@pytest.mark.parametrize("case", RESAMPLED, ids=[_name(c[0]) + "-to-" + "x".join(map(str, c[1])) + ("-ic" if c[2] else "")
                                                 + ("" if c[3] else "-nolists") for c in RESAMPLED])
def test_parity_on_resampled_grids(case):
    image, m, kw, use_lists = case
    shape, bshape, C_, kpd = image
    R = _reference(image, m, kw, use_lists)
    eng = _engine(shape, bshape, C_, R["K"], **kw)
    dp = _dev(R["p"])
    dl = _dev_lists(R["lists"]) if use_lists else None
    axes = _dev_axes(R["tabs"])
    out, ids = eng.render(dp, dl, axes, m, want_argmax=True)
    u8 = eng.render(dp, dl, axes, m, dtype=torch.uint8)
    torch.cuda.synchronize()
    out, ids, u8 = out.cpu().numpy(), ids.cpu().numpy(), u8.cpu().numpy()
    _assert_parity(out, R, m, 0, R["NB"], C_)
    assert np.array_equal(u8, np.rint(out * 255).astype(np.uint8))                       # the lattice index of the fp32 image
    # ids: the restatement's first maximum, away from near-equal top weights and the influence threshold
    extent = [g * v for g, v in zip(R["grid"], m)]
    want_ids = place_blocks(ids_of(R["ref"]["wt"])[..., None], m, R["grid"], extent, 0, np.full(tuple(extent) + (1,), -1, np.int32))[..., 0]
    srt = np.sort(R["ref64"]["wt"], axis=1)
    shaky = ((srt[:, -1, :] - srt[:, -2, :]) < 1e-6) | (np.abs(R["ref64"]["w"] - TAU) < 1e-6).any(axis=1)
    shaky = place_blocks(shaky[..., None], m, R["grid"], extent, 0, np.zeros(tuple(extent) + (1,), bool))[..., 0]
    assert ((ids == want_ids) | shaky).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. shards, bounds, workgroup split
# ---------------------------------------------------------------------------------------------------------------
SENT = -7.0


SHARDS = [(IMAGES[0], (48, 40)), (IMAGES[1], (32, 32)), (IMAGES[3], (16, 16, 7))]      # 2 tiles / 1 tile / 2 tiles per batch


@pytest.mark.parametrize("image,m", SHARDS, ids=[_name(c[0]) + "-to-" + "x".join(map(str, c[1])) for c in SHARDS])
def test_shards_bounds_and_split(image, m, monkeypatch):
    from steered_mixture_of_experts_amd import _lib
    shape, bshape, C_, kpd = image
    d = len(shape)
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    grid = _grid(shape, bshape)
    extent = [g * v for g, v in zip(grid, m)]
    eng = _engine(shape, bshape, C_, K)
    lib = _lib.load()
    dp, dl = _dev(p), _dev_lists(lists)
    axes = _dev_axes(_tables(shape, extent))
    ishape = tuple(extent) + (C_,)
    cp = eng._cparams(dp)
    tabs = (C.c_void_p * 3)(*([t.data_ptr() for t in axes] + [None] * (3 - d)))
    m3 = (C.c_int32 * 3)(*(list(m) + [1] * (3 - d)))

    def call(first, count, image_t, arg_t, fmt=0, params=cp, lists_t=dl, tabs_=tabs, m_=m3, h=None):
        lp = None if lists_t is None else C.c_void_p(lists_t[first:].data_ptr())
        return lib.smoe_shared_render(eng._h if h is None else h, first, count, None if params is None else C.byref(params), lp,
                                      tabs_, m_, None if image_t is None else C.c_void_p(image_t.data_ptr()), fmt,
                                      None if arg_t is None else C.c_void_p(arg_t.data_ptr()), None)

    # one call, guard bands
    buf, view = _guarded(ishape, torch.float32, SENT)
    abuf, aview = _guarded(tuple(extent), torch.int32, 77)
    assert call(0, NB, view, aview) == 0, lib.smoe_last_error()
    torch.cuda.synchronize()
    whole, whole_ids = view.cpu().numpy().copy(), aview.cpu().numpy().copy()
    flat, fa = buf.cpu().numpy(), abuf.cpu().numpy()
    assert (flat[:64] == SENT).all() and (flat[64 + whole.size:] == SENT).all()
    assert (fa[:64] == 77).all() and (fa[64 + whole_ids.size:] == 77).all()
    assert (whole != SENT).all() and (whole_ids != 77).all()
    # three shards into one buffer whose base is offset by 4 bytes (no 16-byte alignment) == one call, bit for bit
    a_, b_ = max(1, NB // 4), max(2, (2 * NB) // 3)
    buf2, view2 = _guarded(ishape, torch.float32, SENT, shift=1)
    abuf2, aview2 = _guarded(tuple(extent), torch.int32, 77, shift=1)
    for first, count in ((0, a_), (a_, b_ - a_), (b_, NB - b_)):
        assert call(first, count, view2, aview2) == 0, lib.smoe_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(view2.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(aview2.cpu().numpy(), whole_ids)
    f2, fa2 = buf2.cpu().numpy(), abuf2.cpu().numpy()
    assert (f2[:65] == SENT).all() and (f2[65 + whole.size:] == SENT).all()
    assert (fa2[:65] == 77).all() and (fa2[65 + whole_ids.size:] == 77).all()
    # a shard alone: the positions of the batches not rendered keep the sentinel
    buf3, view3 = _guarded(ishape, torch.float32, SENT)
    abuf3, aview3 = _guarded(tuple(extent), torch.int32, 77)
    assert call(a_, b_ - a_, view3, aview3) == 0
    torch.cuda.synchronize()
    own = _owned(m, grid, extent, a_, b_ - a_)
    part, part_ids = view3.cpu().numpy(), aview3.cpu().numpy()
    assert np.array_equal(part[own].view(np.uint32), whole[own].view(np.uint32)) and (part[~own] == SENT).all()
    assert np.array_equal(part_ids[own], whole_ids[own]) and (part_ids[~own] == 77).all()
    # uint8 with guard band, aligned and offset by one byte
    for shift in (0, 1):
        bufu, viewu = _guarded(ishape, torch.uint8, 201, shift=shift)
        assert call(0, NB, viewu, None, fmt=1) == 0
        torch.cuda.synchronize()
        fu = bufu.cpu().numpy()
        assert (fu[:64 + shift] == 201).all() and (fu[64 + shift + whole.size:] == 201).all()
        assert np.array_equal(viewu.cpu().numpy(), np.rint(whole * 255).astype(np.uint8))
    # the split of a batch over workgroups does not change a bit
    for split in ("1", "2", "3", "64"):
        monkeypatch.setenv("SMOE_SHARED_RENDER_SPLIT", split)
        buf4, view4 = _guarded(ishape, torch.float32, SENT)
        abuf4, aview4 = _guarded(tuple(extent), torch.int32, 77)
        assert call(0, NB, view4, aview4) == 0
        torch.cuda.synchronize()
        assert np.array_equal(buf4.cpu().numpy().view(np.uint32), flat.view(np.uint32)), split
        assert np.array_equal(abuf4.cpu().numpy(), fa), split
    monkeypatch.delenv("SMOE_SHARED_RENDER_SPLIT")
    # lists = NULL equals all-ones lists
    r1 = eng.render(dp, eng.new_lists(), axes, m)
    r0 = eng.render(dp, None, axes, m)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1)
    # invalid arguments: SMOE_ERR_INVALID, the message names the call, nothing is written
    view.fill_(SENT)
    aview.fill_(77)
    bad_tabs = (C.c_void_p * 3)(*([axes[0].data_ptr()] + [None] * 2))
    bad_m = (C.c_int32 * 3)(*([m[0], 0] + [1]))
    for kwargs, word in [(dict(params=None), b"p "), (dict(image_t=None), b"image"), (dict(tabs_=bad_tabs), b"axis_coords"),
                         (dict(tabs_=None), b"axis_coords"), (dict(m_=bad_m), b"samples"), (dict(first=1, count=NB), b"range"),
                         (dict(first=-1, count=1), b"range"), (dict(fmt=7), b"image_format"), (dict(h=C.c_void_p(None)), b"handle")]:
        args = dict(first=0, count=NB, image_t=view, arg_t=aview)
        args.update(kwargs)
        assert call(**args) == _lib.SMOE_ERR_INVALID, kwargs
        err = lib.smoe_last_error()
        assert b"smoe_shared_render" in err and word in err, (kwargs, err)
    eng10 = _engine(shape, bshape, C_, K, precision=10)
    assert call(0, NB, view, aview, fmt=1, h=eng10._h) == _lib.SMOE_ERR_INVALID and b"precision" in lib.smoe_last_error()
    eng10.close()
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (abuf == 77).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 10. batches larger than smoe_shared_forward can hold
# ---------------------------------------------------------------------------------------------------------------
LARGE = [(IMAGES[1], (128, 128), [0, EMPTY, 5]), (IMAGES[3], (48, 48, 12), [1, 7, 11])]


@pytest.mark.parametrize("image,m,probe", LARGE, ids=[_name(c[0]) + "-to-" + "x".join(map(str, c[1])) for c in LARGE])
def test_large_batches(image, m, probe):
    shape, bshape, C_, kpd = image
    img, p, cfg, K, NB, lists, _ = _setup(shape, bshape, C_, kpd)
    eng = _engine(shape, bshape, C_, K)
    grid = _grid(shape, bshape)
    extent = [g * v for g, v in zip(grid, m)]
    axes = _dev_axes(_tables(shape, extent))
    out = eng.render(_dev(p), _dev_lists(lists), axes, m)
    u8 = eng.render(_dev(p), _dev_lists(lists), axes, m, dtype=torch.uint8)
    torch.cuda.synchronize()
    out, u8 = out.cpu().numpy(), u8.cpu().numpy()
    assert out.shape == tuple(extent) + (C_,)
    assert np.array_equal(u8, np.rint(out * 255).astype(np.uint8))
    for b in probe:
        R = _reference(image, m, {}, True, first=b, count=1)
        _assert_parity(out, R, m, b, 1, C_)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 11. the facade on the device
# ---------------------------------------------------------------------------------------------------------------
def test_facade_render_on_the_device():
    from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
    shape, bshape, C_ = (64, 96), (32, 32), 3
    g = [4, 6]
    b = synthetic_blocks(int(np.prod(g)), (16, 16), C_, 3)
    img = blk.blocks_to_image(b, shape, (16, 16))
    kw = dict(train_inverse_cov=False, batch_size=list(bshape), use_determinant=True, use_yuv=True)
    s = SharedSmoe(img, kernels_per_dim=[6, 8], **kw)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(0.01))
    s.train(6, val_iter=3, ukl_iter=3)
    rec = s.get_reconstruction()
    lens = np.array([m_.sum() for m_ in s.kernel_list_per_batch])
    print(f"list lengths after the fit: mean {lens.mean():.1f} of {s.kernels}")
    out = s.render(scale=1, to_host=False)
    assert out.is_cuda and np.array_equal(out.cpu().numpy().view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(s.render(scale=1, dtype=np.uint8), np.rint(rec * 255).astype(np.uint8))
    _, ids = s.render(scale=1, want_argmax=True)
    am = s.get_weight_matrix_argmax()
    assert ((ids == am) | (ids == -1)).all() and (ids >= 0).mean() > 0.99
    # 2x: the facade on the restatement with the same parameters and lists
    big = s.render(scale=2)
    assert big.shape == (128, 192, 3)
    t = SharedSmoe(img, init_params=s.get_params(), engine_factory=OracleSharedRenderEngine, **kw)
    t._lists = s._recon_lists.cpu().clone()
    ref_img = t.render(scale=2)
    m, grid = (64, 64), [2, 3]
    p = {k: v[None] for k, v in s.get_params().items()}
    tabs = _tables(shape, (128, 192))
    mask = t._engine._mask(t._lists)
    ref64 = oracle_shared_batches(p, mask, tabs, m, grid, 0, t._engine.ocfg, np.float64)
    frac = (np.clip(ref64["y"], 0, 1) * 255 + 0.5) % 1.0
    loose = np.broadcast_to(((frac < 2e-4) | (frac > 1 - 2e-4)) | (np.abs(ref64["w"] - TAU) < 1e-6).any(axis=1)[..., None], frac.shape)
    assert loose.mean() < 0.01
    loose_img = place_blocks(loose, m, grid, (128, 192), 0, np.zeros((128, 192, 3), bool))
    dd = np.abs(big - ref_img)
    print(f"facade 2x: max difference outside the loose set {dd[~loose_img].max():.3e}, overall {dd.max():.3e}")
    assert (dd[~loose_img] < 1e-7).all() and (dd <= 1.0001 / 255).all()
    # use_lists=False is the render with full lists
    free = s.render(scale=2, use_lists=False, to_host=False)
    axes = _dev_axes(tabs)
    direct = s._engine.render(s._params, s._engine.new_lists(), axes, m)
    torch.cuda.synchronize()
    assert torch.equal(free, direct)
    # video, and batches of 16 384 samples through the facade
    vb = synthetic_blocks(4, (16, 16, 4), 3, 11)
    vid = blk.blocks_to_image(vb, (32, 32, 4), (16, 16, 4))
    v = SharedSmoe(vid, kernels_per_dim=[4, 4, 2], train_inverse_cov=False, batch_size=[16, 16, 4], use_determinant=True)
    assert np.array_equal(v.render(scale=1).view(np.uint32), v.get_reconstruction().view(np.uint32))
    assert v.render(samples_per_block=(16, 16, 7)).shape == (32, 32, 7, 3)
    assert s.render(scale=4).shape == (256, 384, 3)
