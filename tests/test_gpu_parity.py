"""GPU parity: libsmoe_hip.so (through the C ABI) vs the CPU restatement in oracle/.

Tolerances: single-pass quantities <= 1e-5 relative (<= 1e-6 absolute near
0); quantised reconstruction identical except <= 1 LSB where y*255 sits within 1e-4 of a
half-integer; one Adam step <= 1e-5; trajectories are judged against the fp32-vs-fp64
sensitivity floor of the restatement itself (the reference's default hyper-parameters make
the 200-step trajectory chaotic, see DESIGN.md "Parity").
"""
import numpy as np
import pytest
import torch

from oracle import smoe_oracle as o
from steered_mixture_of_experts_amd.blocks import synthetic_blocks

pytestmark = pytest.mark.gpu

SHAPES = [
    # block_shape, C, kernels_per_dim, use_yuv
    ((16, 16), 1, [2, 2], False),
    ((16, 16), 3, [2, 2], True),
    ((32, 32), 3, [2, 4], True),
    ((16, 16, 4), 3, [2, 2, 1], True),
    ((16, 16), 1, [2, 4], False),
    # odd shapes: the generic kernels (XL=false: G is not a multiple of the last axis) and ragged pixel counts
    ((7, 5), 1, [2, 2], False),
    ((12, 10, 3), 3, [2, 2, 1], True),
]
# kernel grids / channel counts outside the BASELINE shapes (csrc/smoe_variants.def, basic instantiations):
# the reference takes any grid (smoe.py:2146-2163)
EXTRA_SHAPES = [
    ((16, 16), 1, [3, 3], False),
    ((16, 16), 3, [3, 3], True),
    ((16, 16), 1, [1, 1], False),
    ((16, 16), 3, [1, 2], True),
    ((16, 16), 3, [3, 1], False),
    ((16, 16), 1, [2, 3], False),
    ((16, 16), 1, [3, 4], False),
    ((16, 16), 1, [4, 4], False),
    ((16, 16), 3, [2, 3], True),
    ((8, 8, 4), 1, [2, 2, 1], False),        # grayscale video
    ((8, 8, 8), 1, [2, 2, 2], False),
    ((8, 8, 4), 1, [1, 3, 1], False),
    ((12, 12, 4), 3, [1, 3, 2], True),
    ((8, 8, 8), 3, [2, 2, 2], True),
    ((16, 16, 4), 3, [1, 1, 1], True),
]
# the triples of csrc/smoe_variants.def the lists above leave out: appended at the end, so that the slices below ([::3], [:6])
# keep the entries they had (tests/test_triple_cases_cpu.py: SHAPES + EXTRA_SHAPES name every triple of the build)
LATE_SHAPES = [
    ((16, 16), 1, [1, 2], False),
    ((16, 16), 1, [3, 1], False),
    ((16, 16), 3, [1, 1], True),
    ((8, 8, 4), 1, [1, 1, 1], False),
    ((8, 8, 4), 1, [2, 1, 1], False),
    ((8, 8, 4), 1, [3, 2, 1], False),
    ((8, 8, 4), 3, [1, 2, 1], True),
    ((8, 8, 4), 3, [3, 1, 1], True),
]
EXTRA_SHAPES = EXTRA_SHAPES + LATE_SHAPES
ALL_SHAPES = [(s, 16) for s in SHAPES] + [(s, 64) for s in SHAPES] + [(s, 32) for s in SHAPES[:5]] \
    + [(s, 16) for s in EXTRA_SHAPES] + [(s, 64) for s in EXTRA_SHAPES]
# 128 = one block on both wavefronts of a workgroup (smoe_fit only: the evaluation has no such mode)
# 216 / 416 / 816 = team tiling of smoe_fit (csrc/smoe_team.hip.h): four blocks per workgroup of 2 / 4 / 8 wavefronts on the
# 16-lane layout; block shapes whose last axis divides 16
TEAM_OK = [s for s in SHAPES + EXTRA_SHAPES if 16 % s[0][-1] == 0]
# 264 = duo tiling of smoe_fit (csrc/smoe_duo.hip.h): one block on two symmetric wavefronts; triples with at most 128 slots


def _duo_rows(s):
    """rows of the joint scratch the first wavefront sums: the slots of half the kernels + the loss + their influence counters"""
    d, C, K = len(s[0]), s[1], int(np.prod(s[2]))
    kh = (K + 1) // 2
    return kh * (1 + d + d * (d + 1) // 2 + C + d * C) + 1 + kh


DUO_OK = [s for s in SHAPES + EXTRA_SHAPES if _duo_rows(s) <= 64]
FIT_SHAPES = ALL_SHAPES + [(s, 128) for s in SHAPES] + [(s, 128) for s in EXTRA_SHAPES[::3]] \
    + [(s, 816) for s in TEAM_OK] + [(s, 416) for s in TEAM_OK[:6]] + [(s, 216) for s in TEAM_OK[:6]] + [(s, 264) for s in DUO_OK]


def _ids(cases):
    return ["x".join(map(str, s[0])) + f"-c{s[1]}-k" + "x".join(map(str, s[2])) + f"-g{t}" for s, t in cases]


ALL_IDS = _ids(ALL_SHAPES)


def _engine(shape, C, K, **kw):
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    cfg = EngineConfig(block_shape=shape, channels=C, kernels=K, **kw)
    return BlockEngine(cfg)


def _to_dev(p):
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in p.items()}


def _to_host(p):
    return {k: v.detach().cpu().numpy() for k, v in p.items()}


def _mask_to_bits(active):
    K = active.shape[1]
    return (active.astype(np.uint32) << np.arange(K, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)


def _bits_to_mask(bits, K):
    return ((bits[:, None] >> np.arange(K, dtype=np.uint32)[None, :]) & 1).astype(bool)


def _setup(shape, C, kpd, yuv, B, seed, perturb=True, **cfgkw):
    K = int(np.prod(kpd))
    blk = synthetic_blocks(B, shape, C, seed)
    p = o.init_params(blk, kpd)
    rng = np.random.default_rng(seed + 1)
    if perturb:
        p["A_corr"] = (rng.normal(size=p["A_corr"].shape) * 1.5).astype(np.float32)
        p["A_diagonal"] = (p["A_diagonal"] + rng.normal(size=p["A_diagonal"].shape)).astype(np.float32)
        p["gamma_e"] = (rng.normal(size=p["gamma_e"].shape) * 0.1).astype(np.float32)
        p["musX"] = (p["musX"] + rng.normal(size=p["musX"].shape) * 0.05).astype(np.float32)
        p["pis"] = (p["pis"] * rng.uniform(0.5, 1.5, size=p["pis"].shape)).astype(np.float32)
    cfg = o.OracleConfig(block_shape=shape, channels=C, kernels=K, use_yuv=yuv, **cfgkw)
    coords = o.block_coords(shape)
    tgt = blk.reshape(B, -1, C)
    return cfg, p, coords, tgt, K


def _planar(tgt):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(tgt, (0, 2, 1)))).cuda()


def _close(a, b, rtol=1e-5, atol=1e-6):
    return np.abs(a - b) <= atol + rtol * np.abs(b)


def test_coords_match_numpy_linspace():
    for shape in [(16, 16), (32, 32), (16, 16, 4), (7, 5), (1, 9)]:
        C, K = 1, 4
        if len(shape) == 3:
            C = 3
        eng = _engine(shape, C, K)
        got = eng.coords().numpy()
        want = o.block_coords(shape).T
        assert np.array_equal(got, want), shape
        eng.close()


@pytest.mark.parametrize("case,tiling", ALL_SHAPES, ids=ALL_IDS)
def test_forward_parity(case, tiling):
    shape, C, kpd, yuv = case
    B = 37      # ragged: not a multiple of the blocks per workgroup
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, 100 + len(shape) + C, pis_l1=0.2, u_l1=0.003)
    rng = np.random.default_rng(5)
    active = rng.uniform(size=(B, K)) < 0.85
    p["pis"][3, 0] = 0.0            # pis <= 0 kernels are absent (smoe.py:480)
    p["pis"][4, K - 1] = -0.1
    lw = rng.uniform(0.0, 1.0, size=(B, tgt.shape[1])).astype(np.float32)
    ref = o.forward(p, tgt, coords, active, cfg, lw, np.float32)
    ref64 = o.forward(p, tgt, coords, active, cfg, lw, np.float64)
    eng = _engine(shape, C, K, use_yuv=yuv, pis_l1=0.2, u_l1=0.003)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    out = eng.forward(_planar(tgt), dp, act, loss_w=torch.from_numpy(lw).cuda(), want_recon=True,
                      want_argmax=True, want_gate=True)
    torch.cuda.synchronize()
    loss = out["loss"].cpu().numpy()
    sse = out["sse"].cpu().numpy()
    recon = np.transpose(out["recon"].cpu().numpy(), (0, 2, 1))
    gate = out["gate_w"].cpu().numpy()
    # gate weights: 1e-5 relative, except entries that sit on the influence threshold
    tau = 0.5 / 256
    near_tau = np.abs(ref64["w"] - tau) < 1e-6
    ok = _close(gate, ref["wt"]) | near_tau
    assert ok.all(), np.abs(gate - ref["wt"]).max()
    # quantised reconstruction: identical except <= 1 LSB where y*255 is within 2e-4 of a tie
    lsb = 1.0 / 255
    d = np.abs(recon - ref["recon"])
    frac = (np.clip(ref64["y"], 0, 1) * 255 + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    assert (d[~tie] < 1e-7).all(), d[~tie].max()
    assert (d <= lsb * 1.0001).all()
    assert tie.mean() < 0.01
    # loss / sse given the implementation's own lattice values (the quantiser makes them
    # discontinuous at ties): tight for every block
    refq = o.forward(p, tgt, coords, active, cfg, lw, np.float32, q_override=recon)
    assert _close(loss, refq["loss"], rtol=2e-5).all(), np.abs(loss - refq["loss"]).max()
    assert _close(sse, refq["sse"], rtol=2e-5).all()
    # new active mask and argmax
    new_act = _bits_to_mask(act.cpu().numpy().view(np.uint32), K)
    unstable = near_tau.any(axis=2)
    assert (new_act == ref["active_new"])[~unstable].all()
    am = out["argmax"].cpu().numpy().astype(np.int64)
    # ties between two kernels' gate values within rounding are allowed to differ
    srt = np.sort(np.concatenate([ref64["wt"], np.zeros_like(ref64["wt"][:, :1])], axis=1), axis=1)   # (K = 1: vs zero)
    close_top = (srt[:, -1, :] - srt[:, -2, :]) < 1e-6
    assert (am == ref["argmax"])[~close_top & ~unstable.any(axis=1)[:, None]].all()
    eng.close()


@pytest.mark.parametrize("case,tiling", FIT_SHAPES, ids=_ids(FIT_SHAPES))
def test_one_step_parity(case, tiling):
    """One train iteration: gradients enter Adam's first step as sign-like updates, so
    parity is checked on m (= 0.1*g, exposes the gradient itself), v and the parameters."""
    shape, C, kpd, yuv = case
    B = 21
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, 300 + len(shape) + C)
    active = np.ones((B, K), dtype=bool)
    eng = _engine(shape, C, K, use_yuv=yuv)
    eng.set_tiling(tiling)
    assert ("team16w%d" % (tiling // 100) in eng.fit_variant(B)) == (tiling in (216, 416, 816))
    assert ("duo64w2" in eng.fit_variant(B)) == (tiling == 264)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    # the implementation's own lattice values at these parameters (forward kernel)
    fw = eng.forward(T, dp, act, want_recon=True, update_active=False)
    recon = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float32, want_grads=True, q_override=recon)
    ref64 = o.forward(p, tgt, coords, active, cfg, None, np.float64, want_grads=True, q_override=recon)
    st = o.new_adam_state(p)
    p_ref = o.adam_step({k: v.copy() for k, v in p.items()}, ref["grads"], st, cfg, np.float32)
    state = eng.new_adam_state(dp)
    loss = torch.zeros(B, device="cuda")
    sse = torch.zeros(B, device="cuda")
    eng.fit(T, dp, state, act, 1, loss_out=loss, sse_out=sse)
    torch.cuda.synchronize()
    assert state.step == 1
    # exclude blocks with a gate value on the influence threshold or a blend on the clip
    # edge (discontinuous gradient there); ties of the quantiser are handled by q_override
    tie = (np.abs(ref64["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
    edge = ((np.abs(ref64["y"]) < 1e-6) | (np.abs(ref64["y"] - 1) < 1e-6)).any(axis=(1, 2))
    clean = ~(tie | edge)
    assert clean.sum() >= (3 * B) // 4
    # `recon` came from the evaluation kernel.  That it IS the fit kernel's own lattice is checked, not assumed: a fit launch
    # with every learning rate 0 (no update) reports the loss / SSE of its own pass over the same parameters, and a single
    # pixel one LSB apart would move a block's SSE by >= 1e-4 relative.  With the lattices equal, EVERY tie-free block has to
    # meet the single-pass tolerance (was 85 % of them).
    eng0 = _engine(shape, C, K, use_yuv=yuv, lr_expert=0.0, lr_pis=0.0, lr_steer=0.0)
    eng0.set_tiling(tiling)
    dp0 = _to_dev(p)
    st0 = eng0.new_adam_state(dp0)
    act0 = act.clone()
    l_fit0, s_fit0 = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    eng0.fit(T, dp0, st0, act0, 1, loss_out=l_fit0, sse_out=s_fit0)
    torch.cuda.synchronize()
    for k in dp0:
        assert np.array_equal(dp0[k].cpu().numpy(), np.ascontiguousarray(p[k], dtype=np.float32)), k     # zero learning rates: nothing moved
    eng0.close()
    same_lattice = _close(s_fit0.cpu().numpy(), fw["sse"].cpu().numpy(), rtol=2e-6, atol=1e-9)
    assert same_lattice.all(), np.flatnonzero(~same_lattice)
    assert _close(l_fit0.cpu().numpy(), fw["loss"].cpu().numpy(), rtol=2e-6, atol=1e-12).all()
    lc, sc = _close(loss.cpu().numpy()[clean], ref["loss"][clean], rtol=2e-5), _close(sse.cpu().numpy()[clean], ref["sse"][clean], rtol=2e-5)
    assert lc.all() and sc.all(), (np.flatnonzero(~lc), np.flatnonzero(~sc))
    m = _to_host(state.m)
    got = _to_host(dp)
    for name in o.PARAM_NAMES:
        g_ref = ref["grads"][name][clean]
        # (one kernel per block: w = 1, the gradients of pis / musX / A vanish identically and only rounding residue of the
        # hardware reciprocal is left -- measured against the scale of the expert gradients then)
        scale = max(np.abs(ref64["grads"][name][clean]).max(), (1.0 if K == 1 else 0.0) * np.abs(ref64["grads"]["nu_e"][clean]).max()) + 1e-30
        g_got = m[name][clean] / 0.1
        err = np.abs(g_got - g_ref).max() / scale
        assert err < 2e-5, (name, err)
        if K == 1 and name in ("pis", "musX", "A_diagonal", "A_corr"):
            # one kernel per block: w = 1, these gradients vanish identically.  The kernel returns exact zeros (not the
            # rounding residue of its hardware reciprocal, which Adam would normalise into a step of the size of the learning
            # rate): slots and parameters stay where they were  
            assert not m[name][clean].any(), name
            assert np.array_equal(got[name][clean], p[name][clean]), name
            continue
        perr = np.abs(got[name][clean] - p_ref[name][clean])
        # first TF1-Adam step: delta = lr*g/(|g| + eps*sqrt(1-b1)... ) = lr*g/(|g| + 3.16e-7):
        # an element's sensitivity to gradient noise dg is lr*e/(|g|+e)^2 with e = 1e-8/sqrt(1e-3)
        lr = {"pis": cfg.lr_pis, "A_diagonal": cfg.lr_steer, "A_corr": cfg.lr_steer}.get(name, cfg.lr_expert)
        e = 1e-8 / np.sqrt(1e-3)
        gabs = np.abs(ref64["grads"][name][clean])
        tol = 1e-6 * (np.abs(p_ref[name][clean]) + 1.0) + 2e-5 * lr + lr * (4e-6 * scale) * e / (gabs + e) ** 2
        assert (perr <= tol).all(), (name, (perr / tol).max())
    eng.close()


def test_cfg1_single_block_forward_and_200_iterations():
    """BASELINE configs[0] on the HIP path: ONE 16x16 grayscale block, K = 4, 200 Adam iterations (B = 1: one workgroup,
    the block on both of its wavefronts (duo tiling), 255 idle CUs; the tail-block path of every loader).  Six different blocks, each
    run alone.  Evaluation pass against the restatement; the 200-iteration fit at the CLI defaults judged by how long the GPU
    follows the fp32 restatement (against how long the fp64 restatement does) and by the restatement's own reproducibility band;
    with a well-conditioned steering step (lr_mult 10) within 0.05 dB and parameter-close."""
    shape, C, kpd, K, N = (16, 16), 1, [2, 2], 4, 256
    coords = o.block_coords(shape)
    ps = lambda sse: float(-10 * np.log10(max(float(sse), 1e-12) / (N * C)))
    d_gpu, d_floor, gentle, follow = [], [], [], []
    for seed in range(6):
        b = synthetic_blocks(1, shape, C, 20260500 + seed)
        tgt = b.reshape(1, -1, C)
        p = o.init_params(b, kpd)
        T = _planar(tgt)
        cfg = o.OracleConfig(block_shape=shape, channels=C, kernels=K, quantize_pis=True)
        eng = _engine(shape, C, K, quantize_pis=True)
        assert eng.fit_variant(1).endswith("_duo64w2")        # one block: the two-wavefront (duo) tiling
        # evaluation of the single block
        dp = _to_dev(p)
        act = torch.full((1,), 15, dtype=torch.int32, device="cuda")
        out = eng.forward(T, dp, act, want_recon=True, want_argmax=True, want_gate=True)
        ref = o.forward(p, tgt, coords, np.ones((1, K), bool), cfg, None, np.float32)
        ref64 = o.forward(p, tgt, coords, np.ones((1, K), bool), cfg, None, np.float64)
        recon = np.transpose(out["recon"].cpu().numpy(), (0, 2, 1))
        frac = (np.clip(ref64["y"], 0, 1) * 255 + 0.5) % 1.0
        tie = (frac < 2e-4) | (frac > 1 - 2e-4)
        assert (np.abs(recon - ref["recon"])[~tie] < 1e-7).all() and (np.abs(recon - ref["recon"]) <= 1.0001 / 255).all()
        refq = o.forward(p, tgt, coords, np.ones((1, K), bool), cfg, None, np.float32, q_override=recon)
        assert _close(out["loss"].cpu().numpy(), refq["loss"], rtol=2e-5).all() and _close(out["sse"].cpu().numpy(), refq["sse"], rtol=2e-5).all()
        assert _close(out["gate_w"].cpu().numpy(), ref["wt"]).all() or (np.abs(ref64["w"] - 0.5 / 256) < 1e-6).any()
        assert np.array_equal(_bits_to_mask(act.cpu().numpy().view(np.uint32), K), ref["active_new"]) or (np.abs(ref64["w"] - 0.5 / 256) < 1e-6).any()
        # the whole fit, CLI defaults (lr_steer = 1.0): 200 iterations in two launches with the readmission in between
        st = eng.new_adam_state(dp)
        f0 = eng.forward(T, dp, act, want_recon=False)
        for _ in range(2):
            eng.fit(T, dp, st, act, 100, loss0=f0["loss"])
            eng.update_kernel_list(dp, act)
        g = eng.forward(T, dp, act, want_recon=False)
        torch.cuda.synchronize()
        assert st.step == 200 and np.isfinite(g["sse"].cpu().numpy()).all()
        p32, _, i32 = o.fit(p, tgt, coords, cfg, 200, val_iter=100, dtype=np.float32, record_every=1)
        p64, _, i64 = o.fit(p, tgt, coords, cfg, 200, val_iter=100, dtype=np.float64, record_every=1)
        a = ps(o.forward(p32, tgt, coords, i32["active"], cfg, None, np.float32)["sse"][0])
        c = ps(o.forward(p64, tgt, coords, i64["active"], cfg, None, np.float64)["sse"][0])
        d_gpu.append(abs(ps(g["sse"][0].item()) - a))
        # the restatement's own reproducibility band for this block: fp64, and fp32 reruns from parameters perturbed by 1e-7
        band = [abs(a - c)]
        rng = np.random.default_rng(seed)
        for _ in range(4):
            pp = {k: (v * (1 + 1e-7 * rng.standard_normal(v.shape))).astype(v.dtype) for k, v in p.items()}
            q, _, j = o.fit(pp, tgt, coords, cfg, 200, val_iter=100, dtype=np.float32)
            band.append(abs(ps(o.forward(q, tgt, coords, j["active"], cfg, None, np.float32)["sse"][0]) - a))
        d_floor.append(max(band))
        # ... and HOW LONG the GPU follows the fp32 restatement, iteration by iteration (one iteration per launch; the loss a
        # launch reports is the one of the pass before its Adam step, like the restatement's trace): at least half as long as
        # the fp64 restatement does -- the chaos-proof form of "inside the fp32-vs-fp64 floor"
        dp = _to_dev(p)
        act = torch.full((1,), 15, dtype=torch.int32, device="cuda")
        st = eng.new_adam_state(dp)
        lo = torch.zeros(1, device="cuda")
        lg = []
        for _ in range(100):
            eng.fit(T, dp, st, act, 1, loss0=f0["loss"], loss_out=lo)
            lg.append(float(lo.item()))
        l32 = np.array([t[1][0] for t in i32["trace"]][:100], np.float64)
        l64 = np.array([t[1][0] for t in i64["trace"]][:100], np.float64)
        first = lambda x: int(np.argmax(np.abs(x - l32) > 1e-2 * np.abs(l32))) if (np.abs(x - l32) > 1e-2 * np.abs(l32)).any() else 100
        follow.append((first(np.array(lg)), first(l64)))
        eng.close()
        # well-conditioned steering step: the regime in which a trajectory is reproducible
        cfg_g = o.OracleConfig(block_shape=shape, channels=C, kernels=K, quantize_pis=True, lr_steer=1e-2)
        eng = _engine(shape, C, K, quantize_pis=True, lr_steer=1e-2)
        dp = _to_dev(p)
        act = torch.full((1,), 15, dtype=torch.int32, device="cuda")
        st = eng.new_adam_state(dp)
        f0 = eng.forward(T, dp, act, want_recon=False)
        for _ in range(2):
            eng.fit(T, dp, st, act, 100, loss0=f0["loss"])
            eng.update_kernel_list(dp, act)
        g = eng.forward(T, dp, act, want_recon=False)
        q32, _, j32 = o.fit(p, tgt, coords, cfg_g, 200, val_iter=100, dtype=np.float32)
        q64, _, j64 = o.fit(p, tgt, coords, cfg_g, 200, val_iter=100, dtype=np.float64)
        a = ps(o.forward(q32, tgt, coords, j32["active"], cfg_g, None, np.float32)["sse"][0])
        c = ps(o.forward(q64, tgt, coords, j64["active"], cfg_g, None, np.float64)["sse"][0])
        gentle.append((abs(ps(g["sse"][0].item()) - a), abs(a - c)))
        got = _to_host(dp)
        for name in ("nu_e", "musX", "pis"):
            assert np.abs(got[name] - q32[name]).max() <= 3 * np.abs(q32[name] - q64[name]).max() + 1e-3 * (np.abs(q32[name]).max() + 1), (seed, name)
        eng.close()
    # CLI defaults: chaotic (A steps by ~1 per iteration through an 8-bit quantiser).  Two criteria that do
    # not depend on which way a chaotic block happens to fall: (i) the GPU follows the fp32 restatement at least half as many
    # iterations (loss within 1 %) as the fp64 restatement does, block by block; (ii) over the six blocks the final PSNR
    # deviates from the fp32 restatement's by no more than the restatement's own band (fp64 and four fp32 reruns from
    # parameters perturbed by 1e-7) allows: the medians within a factor of two.
    for tg, t64 in follow:
        assert tg >= 0.5 * t64, follow
    assert np.median([tg for tg, _ in follow]) >= 0.8 * np.median([t64 for _, t64 in follow]), follow
    assert np.median(d_gpu) <= 2.0 * np.median(d_floor) + 0.25, (d_gpu, d_floor)
    # gentle steering step: the contract's 0.05 dB per block (or inside the restatement's own spread where that is larger)
    for dg, df in gentle:
        assert dg <= max(0.05, 2 * df), gentle


def test_short_trajectory_vs_sensitivity_floor():
    """20 iterations at the reference's default learning rates (A trained with lr 1.0 through
    an 8-bit quantiser: rounding differences are amplified, DESIGN.md "Parity").  The GPU's
    deviation from the fp32 restatement must not exceed the restatement's own fp32-vs-fp64
    deviation, and the median block PSNR must agree within 0.05 dB."""
    shape, C, kpd = (16, 16), 1, [2, 2]
    B = 1024
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 777, perturb=False)
    n = 20
    p32, _, i32 = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float32)
    p64, _, i64 = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float64)
    eng = _engine(shape, C, K)
    dp = _to_dev(p)
    state = eng.new_adam_state(dp)
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    T = _planar(tgt)
    eng.forward(T, dp, act, want_recon=False)          # iteration-0 eval pass prunes
    eng.fit(T, dp, state, act, n)
    out = eng.forward(T, dp, act, want_recon=False, update_active=False)
    torch.cuda.synchronize()
    got = _to_host(dp)
    f32 = o.forward(p32, tgt, coords, i32["active"], cfg, None, np.float32)
    f64 = o.forward(p64, tgt, coords, i64["active"], cfg, None, np.float64)
    ps = lambda sse: -10 * np.log10(np.maximum(sse, 1e-12) / (tgt.shape[1] * C))
    g, a, b = ps(out["sse"].cpu().numpy()), ps(f32["sse"]), ps(f64["sse"])
    d_gpu = np.median(np.abs(g - a))
    d_floor = np.median(np.abs(a - b))
    assert d_gpu <= 1.5 * d_floor + 0.005, (d_gpu, d_floor)
    assert abs(np.median(g) - np.median(a)) < 0.05, (np.median(g), np.median(a))
    for name in ("nu_e", "musX", "gamma_e", "pis", "A_diagonal", "A_corr"):
        dev = np.median(np.abs(got[name] - p32[name]))
        floor = np.median(np.abs(p32[name] - p64[name]))
        assert dev <= 2 * floor + 1e-6, (name, dev, floor)
    eng.close()


@pytest.mark.parametrize("tiling,B", [(816, 1024), (416, 37), (216, 150), (264, 1024), (264, 5)])
def test_team_tiling_follows_the_restatement_over_a_trajectory(tiling, B):
    """The team kernel (four blocks per workgroup, the wavefronts split the pixel rows; double-buffered parameters, derived
    constants published by the slot owners) over 40 iterations incl. the kernel-list pruning and a batch that does not fill
    the last workgroup: parameters, kernel lists and losses follow the fp32 restatement inside its own fp32-vs-fp64 floor;
    two runs are bit-identical; with quantize_pis (the CLI default)."""
    shape, C, kpd = (16, 16), 1, [2, 2]
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 1234, perturb=False, lr_steer=1e-2, quantize_pis=True)
    n = 40
    p32, _, i32 = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float32)
    p64, _, i64 = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float64)
    T = _planar(tgt)
    runs = []
    for _ in range(2):
        eng = _engine(shape, C, K, lr_steer=1e-2, quantize_pis=True)
        eng.set_tiling(tiling)
        assert ("duo64w2" if tiling == 264 else "team16w%d" % (tiling // 100)) in eng.fit_variant(B)
        dp = _to_dev(p)
        state = eng.new_adam_state(dp)
        act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
        f0 = eng.forward(T, dp, act, want_recon=False)
        loss = torch.zeros(B, device="cuda")
        eng.fit(T, dp, state, act, n // 2, loss0=f0["loss"])
        eng.fit(T, dp, state, act, n - n // 2, loss0=f0["loss"], loss_out=loss)          # state carried across launches
        torch.cuda.synchronize()
        runs.append((_to_host(dp), _to_host(state.m), act.cpu().numpy().copy(), loss.cpu().numpy().copy()))
        eng.close()
    for name in o.PARAM_NAMES:
        assert np.array_equal(runs[0][0][name], runs[1][0][name]) and np.array_equal(runs[0][1][name], runs[1][1][name]), name
    assert np.array_equal(runs[0][2], runs[1][2])
    got = runs[0][0]
    for name in o.PARAM_NAMES:
        dev = np.abs(got[name] - p32[name])
        floor = np.abs(p32[name] - p64[name])
        assert np.median(dev) <= 3 * np.median(floor) + 1e-5, (name, np.median(dev), np.median(floor))
        assert np.isfinite(got[name]).all()
    same_lists = (_bits_to_mask(runs[0][2].view(np.uint32), K) == i32["active"]).all(axis=1)
    assert same_lists.mean() > 0.97


def test_gentle_lr_trajectory_tight():
    """With a small steering learning rate the dynamics are well conditioned and the GPU
    follows the restatement closely over 50 steps."""
    shape, C, kpd = (16, 16), 1, [2, 2]
    B = 64
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 991, perturb=False, lr_steer=1e-2)
    n = 50
    p32, st32, i32 = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float32)
    p64, _, _ = o.fit(p, tgt, coords, cfg, n, val_iter=10 ** 9, dtype=np.float64)
    eng = _engine(shape, C, K, lr_steer=1e-2)
    dp = _to_dev(p)
    state = eng.new_adam_state(dp)
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    T = _planar(tgt)
    eng.forward(T, dp, act, want_recon=False)
    eng.fit(T, dp, state, act, n)
    torch.cuda.synchronize()
    got = _to_host(dp)
    for name in o.PARAM_NAMES:
        dev = np.abs(got[name] - p32[name])
        floor = np.abs(p32[name] - p64[name])
        assert np.median(dev) <= 3 * np.median(floor) + 1e-5, (name, np.median(dev), np.median(floor))
    eng.close()


@pytest.mark.parametrize("tiling", [0, 416, 816, 264])
def test_frozen_blocks_and_divergence_flag(tiling):
    shape, C, kpd = (16, 16), 1, [2, 2]
    B = 8
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 4242, perturb=False)
    eng = _engine(shape, C, K)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    before = _to_host(dp)
    state = eng.new_adam_state(dp)
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    div = torch.zeros(B, dtype=torch.int32, device="cuda")
    div[2] = 1
    loss0 = torch.full((B,), 1.0, device="cuda")
    loss0[5] = -100.0 + 1e-4     # loss + 1 > (loss0 + 100) * 10 trips immediately
    eng.fit(_planar(tgt), dp, state, act, 5, diverged=div, loss0=loss0)
    torch.cuda.synchronize()
    after = _to_host(dp)
    d = div.cpu().numpy()
    assert d[2] == 1 and d[5] == 1 and d[[0, 1, 3, 4, 6, 7]].sum() == 0
    for name in o.PARAM_NAMES:
        assert np.array_equal(after[name][2], before[name][2])
    # block 5 took exactly one step (the diverging iteration's update is kept, smoe.py:1527-1570)
    st = o.new_adam_state(p)
    f = o.forward(p, tgt, coords, np.ones((B, K), bool), cfg, None, np.float32, want_grads=True)
    p1 = o.adam_step({k: v.copy() for k, v in p.items()}, f["grads"], st, cfg, np.float32)
    assert np.allclose(after["nu_e"][5], p1["nu_e"][5], atol=2e-6)
    assert not np.allclose(after["nu_e"][0], p1["nu_e"][0], atol=1e-4)
    eng.close()


def test_update_kernel_list_and_best_and_reduce():
    shape, C, kpd = (16, 16), 1, [2, 2]
    B = 50
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 31337)
    p["A_diagonal"][7] *= 40.0          # far kernels: maha at every probe >= 800 for some
    p["pis"][9, 2] = 0.0
    active = np.zeros((B, K), dtype=bool)
    active[::2, 0] = True
    want = o.readmit(p, active, cfg, np.float32)
    eng = _engine(shape, C, K)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    eng.update_kernel_list(dp, act)
    torch.cuda.synchronize()
    got = _bits_to_mask(act.cpu().numpy().view(np.uint32), K)
    assert np.array_equal(got, want)
    assert not want[7].all() and not want[9, 2]
    # best snapshot
    loss = torch.rand(B, device="cuda")
    best_loss = torch.full((B,), 0.5, device="cuda")
    best = {k: torch.zeros_like(v) for k, v in dp.items()}
    eng.checkpoint_best(loss, best_loss, dp, best)
    torch.cuda.synchronize()
    better = (loss < 0.5).cpu().numpy()
    for name in o.PARAM_NAMES:
        b = best[name].cpu().numpy()
        assert np.array_equal(b[better], p[name][better].astype(np.float32))
        assert not b[~better].any()
    assert np.array_equal(best_loss.cpu().numpy(), np.where(better, loss.cpu().numpy(), 0.5).astype(np.float32))
    # scalar reduction
    sse = torch.rand(B, device="cuda")
    r = eng.reduce_scalars(loss, sse, act).cpu().numpy()
    assert abs(r[0] - float(loss.double().sum()) * 256) < 1e-6
    assert abs(r[1] - float(sse.double().sum())) < 1e-9
    assert r[2] == got.sum()
    eng.close()


def test_error_paths():
    from steered_mixture_of_experts_amd import _lib
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    with pytest.raises(_lib.SmoeError) as e:
        BlockEngine(EngineConfig(block_shape=(16, 16), channels=2, kernels=5))
    assert e.value.code == _lib.SMOE_ERR_UNSUPPORTED
    eng = _engine((16, 16), 1, 4)
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(3, 1, 100, device="cuda"), eng.new_params(3), torch.zeros(3, dtype=torch.int32, device="cuda"))
    eng.close()


@pytest.mark.parametrize("tiling", [16, 64, 128, 216, 816, 264])
def test_fit_with_loss_weights_regularisers_and_clipping(tiling):
    """The fit kernel's per-pixel loss-weight path (padding / loss masks, smoe.py:550,932), the l1
    regularisers (smoe.py:1027,1044) and gradient clipping (smoe.py:1152-1153) against the oracle."""
    shape, C, kpd, yuv = (16, 16), 3, [2, 2], True
    B = 19
    kw = dict(pis_l1=0.3, u_l1=0.002, grad_clip=2e-4)
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, yuv, B, 4711, **kw)
    rng = np.random.default_rng(3)
    lw = (rng.uniform(size=(B, tgt.shape[1])) < 0.7).astype(np.float32)       # 0/1 mask like the padding mask
    lw[5] = 0.0                                                                 # a fully masked block
    active = np.ones((B, K), dtype=bool)
    active[2, 1] = False
    eng = _engine(shape, C, K, use_yuv=yuv, **kw)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T, LW = _planar(tgt), torch.from_numpy(lw).cuda()
    fw = eng.forward(T, dp, act, loss_w=LW, want_recon=True, update_active=False)
    recon = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, lw, np.float32, want_grads=True, q_override=recon)
    ref64 = o.forward(p, tgt, coords, active, cfg, lw, np.float64, want_grads=True, q_override=recon)
    st = o.new_adam_state(p)
    p_ref = o.adam_step({k: v.copy() for k, v in p.items()}, ref["grads"], st, cfg, np.float32)
    state = eng.new_adam_state(dp)
    loss = torch.zeros(B, device="cuda")
    eng.fit(T, dp, state, act, 1, loss_w=LW, loss_out=loss)
    torch.cuda.synchronize()
    assert np.allclose(loss.cpu().numpy(), ref["loss"], rtol=3e-5, atol=1e-9)
    clip = kw["grad_clip"]
    m = _to_host(state.m)
    for name in o.PARAM_NAMES:
        g_clip = np.clip(ref64["grads"][name], -clip, clip)
        scale = max(clip, float(np.abs(ref64["grads"][name]).max()))
        assert np.abs(m[name] / 0.1 - g_clip).max() < 3e-5 * scale + 1e-9, name
        assert (np.abs(m[name] / 0.1) <= clip * 1.00001).all()
    assert (np.abs(ref64["grads"]["nu_e"]) > clip).any()                        # the clip actually bites
    got = _to_host(dp)
    # block 5 (all weights 0): only the regulariser gradients move pis / A_diagonal
    assert np.array_equal(got["nu_e"][5], p["nu_e"][5]) and np.array_equal(got["musX"][5], p["musX"][5])
    assert not np.array_equal(got["pis"][5], p["pis"][5])
    for name in ("nu_e", "musX", "gamma_e"):
        assert np.abs(got[name] - p_ref[name]).max() < 2e-5, name
    eng.close()


@pytest.mark.parametrize("tiling", [16, 64, 128, 416, 264])
def test_only_y_gamma(tiling):
    """gamma_mask (smoe.py:725-729): slopes act and train only for channel 0."""
    shape, C, kpd = (16, 16), 3, [2, 2]
    B = 11
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, True, B, 99, only_y_gamma=True)
    active = np.ones((B, K), dtype=bool)
    eng = _engine(shape, C, K, use_yuv=True, only_y_gamma=True)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    fw = eng.forward(T, dp, act, want_recon=True, update_active=False)
    recon = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float64, want_grads=True, q_override=recon)
    plain = o.forward(p, tgt, coords, active, o.OracleConfig(block_shape=shape, channels=C, kernels=K, use_yuv=True),
                      None, np.float64)
    assert np.abs(plain["y"] - ref["y"]).max() > 1e-3                 # the mask changes the blend
    assert np.allclose(fw["loss"].cpu().numpy(), ref["loss"], rtol=3e-5)
    st = eng.new_adam_state(dp)
    before = dp["gamma_e"].cpu().numpy().copy()
    eng.fit(T, dp, st, act, 1)
    torch.cuda.synchronize()
    m = _to_host(st.m)
    for name in o.PARAM_NAMES:
        scale = np.abs(ref["grads"][name]).max() + 1e-30
        assert np.abs(m[name] / 0.1 - ref["grads"][name]).max() / scale < 3e-5, name
    after = dp["gamma_e"].cpu().numpy()
    assert np.array_equal(after[..., 1:], before[..., 1:]) and not np.array_equal(after[..., 0], before[..., 0])
    eng.close()


@pytest.mark.parametrize("tiling", [0, 816, 264])
@pytest.mark.parametrize("qpis", [False, True])
def test_kernel_count_as_norm_l1(qpis, tiling):
    """kernel_count_as_norm_l1 (smoe.py:1022-1027): the pis l1 term is normalised by the number of kernels with
    (q)pis > 0 -- independent of the kernel list -- instead of start_pis."""
    shape, C, kpd = (16, 16), 1, [2, 4]
    B = 24
    cfg, p, coords, tgt, K = _setup(shape, C, kpd, False, B, 55, pis_l1=0.3, u_l1=0.002, kernel_count_as_norm_l1=True,
                                    quantize_pis=qpis)
    p["pis"][0, 1] = 0.0
    p["pis"][0, 5] = -0.2
    p["pis"][1, 2] = 0.0006 if qpis else 0.0           # rounds to 0 on the pis lattice
    active = np.ones((B, K), bool)
    active[0, 0] = False
    eng = _engine(shape, C, K, pis_l1=0.3, u_l1=0.002, kernel_count_as_norm_l1=True, quantize_pis=qpis)
    eng.set_tiling(tiling)
    dp = _to_dev(p)
    act = torch.from_numpy(_mask_to_bits(active).view(np.int32)).cuda()
    T = _planar(tgt)
    fw = eng.forward(T, dp, act, want_recon=True, update_active=False)
    recon = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref = o.forward(p, tgt, coords, active, cfg, None, np.float32, want_grads=True, q_override=recon)
    plain = o.forward(p, tgt, coords, active, o.OracleConfig(**{**cfg.__dict__, "kernel_count_as_norm_l1": False}), None,
                      np.float32, q_override=recon)
    assert _close(fw["loss"].cpu().numpy(), ref["loss"], rtol=2e-5).all()
    assert np.abs(ref["loss"] - plain["loss"])[:2].min() > 1e-3          # blocks 0 and 1 lost kernels: different norm
    st = eng.new_adam_state(dp)
    eng.fit(T, dp, st, act, 1)
    torch.cuda.synchronize()
    g = st.m["pis"].cpu().numpy() / 0.1
    assert np.abs(g - ref["grads"]["pis"]).max() < 2e-5 * np.abs(ref["grads"]["pis"]).max()
    eng.close()
