"""GPU parity of train_inverse_cov (the reference CONSTRUCTOR default; smoe.py:734-735,791-793): A symmetric
(diag + A_corr + A_corr^T), maha = r^T A r, determinant factor prod(diag A) -- against the CPU restatement
(checked against torch.autograd in tests/test_oracle.py)."""
import numpy as np
import pytest
import torch

from oracle import smoe_oracle as o
from test_gpu_parity import LATE_SHAPES, SHAPES, _bits_to_mask, _close, _engine, _mask_to_bits, _planar, _setup, _to_dev, _to_host

pytestmark = pytest.mark.gpu


def _ic_setup(shape, C, kpd, yuv, B, seed, **kw):
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, seed, train_inverse_cov=True, **kw)
    # generate_kernel_grid squares A_init for this form (smoe.py:2162); keep the matrices positive definite
    p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
    p["A_corr"] = (p["A_corr"] * 2.0).astype(np.float32)
    return cfg, p, coords, tgt, K


# the FULL triples and the odd block shapes, then the triples no other deterministic case runs with train_inverse_cov (the basic
# set of a triple that is not FULL holds the +ic kernels as well)
IC_SHAPES = SHAPES + LATE_SHAPES


@pytest.mark.parametrize("shape,C,kpd,yuv", IC_SHAPES)
@pytest.mark.parametrize("tiling", [16, 64])
def test_invcov_forward(shape, C, kpd, yuv, tiling):
    B = 29
    cfg, p, coords, tgt, K = _ic_setup(shape, C, kpd, yuv, B, 500 + C, pis_l1=0.2, u_l1=0.003)
    active = np.random.default_rng(3).uniform(size=(B, K)) < 0.9
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float32)
    ref64 = o.forward(p, tgt, coords, active, cfg, None, np.float64)
    eng = _engine(shape, C, K, use_yuv=yuv, pis_l1=0.2, u_l1=0.003, train_inverse_cov=True)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    out = eng.forward(_planar(tgt), dp, act, want_recon=True, want_gate=True)
    torch.cuda.synchronize()
    gate = out["gate_w"].cpu().numpy()
    near_tau = np.abs(ref64["w"] - 0.5 / 256) < 1e-6
    assert (_close(gate, ref["wt"], rtol=2e-5) | near_tau).all(), np.abs(gate - ref["wt"]).max()
    recon = np.transpose(out["recon"].cpu().numpy(), (0, 2, 1))
    frac = (np.clip(ref64["y"], 0, 1) * 255 + 0.5) % 1.0
    tie = (frac < 3e-4) | (frac > 1 - 3e-4)
    assert (np.abs(recon - ref["recon"])[~tie] < 1e-7).all()
    refq = o.forward(p, tgt, coords, active, cfg, None, np.float32, q_override=recon)
    assert _close(out["loss"].cpu().numpy(), refq["loss"], rtol=3e-5).all()
    new_act = _bits_to_mask(act.cpu().numpy().view(np.uint32), K)
    assert (new_act == ref["active_new"])[~near_tau.any(axis=2)].all()
    # it really is the other form
    std = o.forward(p, tgt, coords, active, o.OracleConfig(**{**cfg.__dict__, "train_inverse_cov": False}), None, np.float32)
    assert np.abs(std["wt"] - ref["wt"]).max() > 1e-2
    eng.close()


@pytest.mark.parametrize("shape,C,kpd,yuv", IC_SHAPES)
@pytest.mark.parametrize("tiling", [16, 64])
def test_invcov_one_step_gradients(shape, C, kpd, yuv, tiling):
    B = 21
    cfg, p, coords, tgt, K = _ic_setup(shape, C, kpd, yuv, B, 700 + C, pis_l1=0.05, u_l1=0.001)
    active = np.ones((B, K), dtype=bool)
    eng = _engine(shape, C, K, use_yuv=yuv, pis_l1=0.05, u_l1=0.001, train_inverse_cov=True)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    fw = eng.forward(T, dp, act, want_recon=True, update_active=False)
    recon = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref64 = o.forward(p, tgt, coords, active, cfg, None, np.float64, want_grads=True, q_override=recon)
    state = eng.new_adam_state(dp)
    loss = torch.zeros(B, device="cuda")
    eng.fit(T, dp, state, act, 1, loss_out=loss)
    torch.cuda.synchronize()
    tie = (np.abs(ref64["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
    edge = ((np.abs(ref64["y"]) < 1e-6) | (np.abs(ref64["y"] - 1) < 1e-6)).any(axis=(1, 2))
    clean = ~(tie | edge)
    assert clean.sum() >= B // 2
    assert _close(loss.cpu().numpy()[clean], ref64["loss"][clean], rtol=3e-5).all()
    m = _to_host(state.m)
    for name in o.PARAM_NAMES:
        g_ref = ref64["grads"][name][clean]
        scale = np.abs(g_ref).max() + 1e-30
        err = np.abs(m[name][clean] / 0.1 - g_ref).max() / scale
        assert err < 3e-5, (name, err)
    eng.close()


def test_invcov_gentle_fit_and_readmission():
    shape, C, kpd = (16, 16), 1, [2, 2]
    B = 64
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 991, perturb=False, lr_steer=0.05, train_inverse_cov=True)
    p["A_diagonal"] = p["A_diagonal"] ** 2
    n = 40
    p32, _, i32 = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float32)
    p64, _, _ = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float64)
    eng = _engine(shape, C, K, lr_steer=0.05, train_inverse_cov=True)
    dp = _to_dev(p)
    state = eng.new_adam_state(dp)
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    T = _planar(tgt)
    l0 = eng.forward(T, dp, act, want_recon=False)["loss"].cpu().numpy()
    eng.fit(T, dp, state, act, n)
    l1 = eng.forward(T, dp, act, want_recon=False, update_active=False)["loss"].cpu().numpy()
    torch.cuda.synchronize()
    assert np.median(l1) < 0.7 * np.median(l0)
    got = _to_host(dp)
    for name in o.PARAM_NAMES:
        dev = np.abs(got[name] - p32[name])
        floor = np.abs(p32[name] - p64[name])
        assert np.median(dev) <= 3 * np.median(floor) + 1e-5, (name, np.median(dev), np.median(floor))
    pp = {k: v.copy() for k, v in got.items()}
    pp["A_diagonal"][5] *= 900.0
    want = o.readmit(pp, np.zeros((B, K), bool), cfg, np.float32)
    empty = torch.zeros_like(act)
    eng.update_kernel_list(_to_dev(pp), empty)
    torch.cuda.synchronize()
    assert np.array_equal(_bits_to_mask(empty.cpu().numpy().view(np.uint32), K), want) and not want[5].all()
    eng.close()


def test_invcov_facade_and_refused_combinations():
    from fake_engine import OracleEngine
    from steered_mixture_of_experts_amd import _lib
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    from steered_mixture_of_experts_amd.smoe import Adam, Smoe
    b = blk.synthetic_blocks(16, (16, 16), 1, 9)
    img = blk.blocks_to_image(b, (64, 64), (16, 16))
    runs = []
    for factory in (None, OracleEngine):
        s = Smoe(img, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True, train_inverse_cov=True,
                 **({} if factory is None else {"engine_factory": factory}))
        s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(0.05))
        s.train(20, val_iter=10)
        runs.append([v for _, v in s.get_losses()])
    assert abs(runs[0][0] - runs[1][0]) < 1e-6 * runs[1][0] + 1e-9 and np.allclose(runs[0], runs[1], rtol=2e-2)
    assert runs[0][-1] < runs[0][0]
    # the form composes with the SSIM loss and the fake-quantised graph: one-step gradients against the oracle
    for kw in ({"ssim_opt": True}, {"quantization_mode": 3, "quantize_pis": True, "bit_depths": (14, 12, 8, 10, 10)},
               {"quantization_mode": 2, "quantize_pis": True, "bit_depths": (16, 12, 8, 10, 10),
                "lower_bounds": (-200, -.3, -1, 0, -4), "upper_bounds": (200, 1.3, 2, 2, 4)}):
        B = 17
        cfg, p, coords, tgt, K = _ic_setup((16, 16), 1, [2, 2], False, B, 41, **kw)
        d = 2
        p["A_corr"] = p["A_corr"] * np.tril(np.ones((d, d), np.float32), -1)
        active = np.ones((B, K), bool)
        eng = _engine((16, 16), 1, K, train_inverse_cov=True, **kw)
        dp = _to_dev(p)
        act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
        T = _planar(tgt)
        recon = np.transpose(eng.forward(T, dp, act, want_recon=True, update_active=False)["recon"].cpu().numpy(), (0, 2, 1))
        ref = o.forward(p, tgt, coords, active, cfg, None, np.float32, want_grads=True, q_override=recon)
        st = eng.new_adam_state(dp)
        eng.fit(T, dp, st, act, 1)
        torch.cuda.synchronize()
        tie = (np.abs(ref["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
        edge = ((np.abs(ref["y"]) < 1e-6) | (np.abs(ref["y"] - 1) < 1e-6)).any(axis=(1, 2))
        clean = ~(tie | edge)
        m = _to_host(st.m)
        for name in o.PARAM_NAMES:
            g_ref = ref["grads"][name][clean]
            err = np.abs(m[name][clean] / 0.1 - g_ref).max() / (np.abs(g_ref).max() + 1e-30)
            assert err < 1e-4, (kw, name, err)
        eng.close()


@pytest.mark.parametrize("ic", [False, True])
@pytest.mark.parametrize("shape,C,kpd,yuv,tiling", [((16, 16), 1, [2, 2], False, 16), ((16, 16), 3, [2, 2], True, 64),
                                                     ((16, 16, 4), 3, [2, 2, 1], True, 64), ((7, 5), 1, [2, 2], False, 16)])
def test_radial_steering(shape, C, kpd, yuv, tiling, ic):
    """radial_as (smoe.py:714-719): equal steering diagonals, their gradient is the trace of dL/dA, A_corr is not
    trained, the u_l1 term counts d times."""
    B, d = 19, len(shape)
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, 900 + C, pis_l1=0.05, u_l1=0.002, radial_as=True,
                                    train_inverse_cov=ic)
    a = np.abs(p["A_diagonal"][:, :, 0, 0]) ** (2 if ic else 1)
    p["A_diagonal"] = (a[..., None, None] * np.eye(d)).astype(np.float32)
    p["A_corr"] = np.zeros_like(p["A_corr"])
    active = np.ones((B, K), bool)
    eng = _engine(shape, C, K, use_yuv=yuv, pis_l1=0.05, u_l1=0.002, radial_as=True, train_inverse_cov=ic)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    recon = np.transpose(eng.forward(T, dp, act, want_recon=True, update_active=False)["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float64, want_grads=True, q_override=recon)
    st = eng.new_adam_state(dp)
    eng.fit(T, dp, st, act, 3)
    torch.cuda.synchronize()
    got = _to_host(dp)
    dg = np.diagonal(got["A_diagonal"], axis1=-2, axis2=-1)
    assert np.all(dg == dg[..., :1]) and not got["A_corr"].any()          # tied, A_corr untouched
    assert np.abs(dg - np.diagonal(p["A_diagonal"], axis1=-2, axis2=-1)).max() > 0.5        # and really trained (lr 1.0)
    # first-step gradient through a fresh one-step run
    dp1 = _to_dev(p)
    st1 = eng.new_adam_state(dp1)
    eng.fit(T, dp1, st1, act, 1)
    torch.cuda.synchronize()
    tie = (np.abs(ref["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
    edge = ((np.abs(ref["y"]) < 1e-6) | (np.abs(ref["y"] - 1) < 1e-6)).any(axis=(1, 2))
    clean = ~(tie | edge)
    m = _to_host(st1.m)
    for name in ("A_diagonal", "musX", "nu_e", "pis"):
        g_ref = ref["grads"][name][clean]
        err = np.abs(m[name][clean] / 0.1 - g_ref).max() / (np.abs(g_ref).max() + 1e-30)
        assert err < 5e-5, (name, err)
    assert not m["A_corr"].any()
    eng.close()


QKW = dict(bit_depths=(14, 12, 8, 10, 10), lower_bounds=(-60, -.3, -1, 0, -4), upper_bounds=(60, 1.3, 2, 2, 4))


@pytest.mark.parametrize("tiling", [16, 64])
def test_radial_steering_with_fixed_range_quantisation(tiling):
    """radial_as together with quantization_mode 2 (smoe.py:481-484: the (K,) variable through a fixed-range fake quant):
    the d tied copies quantise alike, their mask is the variable's mask, the gradient stays the trace."""
    shape, C, kpd, yuv = (16, 16), 1, [2, 2], False
    B, d = 19, 2
    kw = dict(pis_l1=0.05, u_l1=0.002, radial_as=True, quantization_mode=2, quantize_pis=True, **QKW)
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, 950, **kw)
    a = np.abs(p["A_diagonal"][:, :, 0, 0])
    a[3, 1] = 75.0                                     # outside the fixed range: clamped, no gradient
    p["A_diagonal"] = (a[..., None, None] * np.eye(d)).astype(np.float32)
    p["A_corr"] = np.zeros_like(p["A_corr"])
    active = np.ones((B, K), bool)
    eng = _engine(shape, C, K, use_yuv=yuv, **kw)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    recon = np.transpose(eng.forward(T, dp, act, want_recon=True, update_active=False)["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float32, want_grads=True, q_override=recon)
    st = eng.new_adam_state(dp)
    eng.fit(T, dp, st, act, 1)
    torch.cuda.synchronize()
    tie = (np.abs(ref["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
    edge = ((np.abs(ref["y"]) < 1e-6) | (np.abs(ref["y"] - 1) < 1e-6)).any(axis=(1, 2))
    clean = ~(tie | edge)
    m = _to_host(st.m)
    for name in ("A_diagonal", "musX", "nu_e", "pis", "gamma_e"):
        g_ref = ref["grads"][name][clean]
        err = np.abs(m[name][clean] / 0.1 - g_ref).max() / (np.abs(g_ref).max() + 1e-30)
        assert err < 5e-5, (name, err)
    assert not m["A_corr"].any() and not m["A_diagonal"][3, 1].any()
    dg = np.diagonal(_to_host(dp)["A_diagonal"], axis1=-2, axis2=-1)
    assert np.all(dg == dg[..., :1])
    eng.close()


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("shape,C,kpd,yuv,tiling", [((16, 16), 1, [2, 2], False, 16), ((16, 16), 1, [2, 2], False, 64),
                                                     ((16, 16, 4), 3, [2, 2, 1], True, 64)])
def test_radial_steering_with_ranges_from_the_data(shape, C, kpd, yuv, tiling, tied):
    """radial_as together with quantization_mode 3 (smoe.py:498-504): fake_quant(a, 0, max - min) + min on the (K,)
    variable -- the reference does not shift the input by the minimum, restated as is (oracle pinned against autograd in
    tests/test_oracle.py).  ``tied``: equal steering values except one (tied minima share the routed gradient)."""
    B, d = 19, len(shape)
    kw = dict(pis_l1=0.05, u_l1=0.002, radial_as=True, quantization_mode=3, quantize_pis=True,
              bit_depths=(12, 10, 6, 10, 8))
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, 960 + C, **kw)
    a = np.abs(p["A_diagonal"][:, :, 0, 0])
    if tied:
        a[:] = a[:, :1]
        a[1::2, 1] *= 1.5
    p["A_diagonal"] = (a[..., None, None] * np.eye(d)).astype(np.float32)
    p["A_corr"] = np.zeros_like(p["A_corr"])
    p["pis"][2, 1] = 0.0004                            # qpis = 0: outside the mask of the ranges
    active = np.ones((B, K), bool)
    eng = _engine(shape, C, K, use_yuv=yuv, **kw)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    fw = eng.forward(T, dp, act, want_recon=True, update_active=False)
    recon = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float32, want_grads=True, q_override=recon)
    assert np.abs(fw["loss"].cpu().numpy() - ref["loss"]).max() < 2e-5
    st = eng.new_adam_state(dp)
    eng.fit(T, dp, st, act, 1)
    torch.cuda.synchronize()
    tie = (np.abs(ref["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
    edge = ((np.abs(ref["y"]) < 1e-6) | (np.abs(ref["y"] - 1) < 1e-6)).any(axis=(1, 2))
    clean = ~(tie | edge)
    assert clean.sum() >= B // 2
    m = _to_host(st.m)
    for name in ("A_diagonal", "musX", "nu_e", "pis", "gamma_e"):
        g_ref = ref["grads"][name][clean]
        err = np.abs(m[name][clean] / 0.1 - g_ref).max() / (np.abs(g_ref).max() + 1e-30)
        assert err < 3e-4, (name, err)      # fp32 sums over up to 1 024 pixels against the fp32 restatement (other order)
    assert not m["A_corr"].any()
    dg = np.diagonal(_to_host(dp)["A_diagonal"], axis1=-2, axis2=-1)
    assert np.all(dg == dg[..., :1])
    eng.close()
