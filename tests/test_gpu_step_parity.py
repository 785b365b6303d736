"""GPU matrix of the teacher-forced step (tests/step_parity.py) and launch-split invariance of smoe_fit.

(a) ONE Adam step from a state with non-trivial slots, beta powers and a partial kernel list, element by element against
    the restatement: every shape of test_gpu_parity.SHAPES x every fit tiling x loss-weight kinds (padding mask, fractional,
    pixel sub-sample, none) x two states (t = 7, beta powers of step 150), the option legs (l1 + clip, quantize_pis,
    train_inverse_cov, quantization_mode 2 / 3; the switches off their defaults: use_determinant, each train_*, precision
    6 / 10, margin, start_pis) with a padding mask, precision 10 and use_determinant=False without weights too (the
    unweighted kernels are instantiations of their own), and the SSIM graph with weights passed.
(b) Six iterations as one launch of 6, as 2 + 4 and as 6 x 1 give bit-identical parameters, slots, lists, flags and losses:
    inside a launch the kernel advances the beta powers and refreshes its derived LDS state itself, at a launch boundary
    it rebuilds them from global memory and from the host's running products.
(c) Every case asserts on smoe_last_fit_variant which kernel produced its numbers.
"""
import dataclasses

import numpy as np
import pytest
import torch

import step_parity as sp
from oracle import smoe_oracle as o
from test_gpu_parity import DUO_OK, SHAPES, TEAM_OK, _bits_to_mask, _engine

pytestmark = pytest.mark.gpu

# tilings of smoe_fit (include/smoe_hip.h: smoe_set_tiling)
# (128 = one block on both wavefronts: two rows of 64 pixels, so not the 35-pixel blocks of (7, 5) -- there smoe_fit runs the
# plain 64-lane kernel, which the 64 column covers)
TILINGS = [(s, 16) for s in SHAPES] + [(s, 64) for s in SHAPES] + [(s, 32) for s in SHAPES[:5]] \
    + [(s, 128) for s in SHAPES if int(np.prod(s[0])) >= 128] \
    + [(s, 264) for s in SHAPES if s in DUO_OK] + [(s, 816) for s in SHAPES if s in TEAM_OK]
KIND_STATES = [("pad", False), ("frac", False), ("sample", False), ("none", True), ("pad", True)]
LEG_SHAPES = [SHAPES[1], SHAPES[2], SHAPES[3]]          # (16,16)/3, (32,32)/3, (16,16,4)/3
# train_inverse_cov has its own instantiation on the 16-, 32- and 64-lane tilings (the basic set), quantization_mode 2 / 3
# and SSIM on the 16- and 64-lane tilings only; the pair, duo and team tilings carry the plain margin-loss graph
_ALL, _BASIC = (16, 64, 32, 128, 264, 816), (16, 64, 32)
LEG_TILINGS = {"l1clip": _ALL, "qpis": _ALL, "ic": _BASIC, "q2": (16, 64), "q3": (16, 64),
               "nodet": _ALL, "nodet_ic": _BASIC, "fz_pis": _ALL, "fz_mus": _ALL, "fz_gam": _ALL, "p10": _ALL, "p6": _ALL, "margin": _ALL,
               "startpis": _ALL}
# ... and blocks of 1 024 pixels with loss weights do not fit the 16-lane quantised kernels' LDS (four blocks per wavefront,
# each with its pixel rows, its weights and the quantised parameter image): the library refuses them, see
# test_weighted_big_blocks_are_refused_by_the_16_lane_quantised_kernels
NO_G16_QUANT = lambda s, t, leg: leg in ("q2", "q3") and t == 16 and int(np.prod(s[0])) >= 1024

# (case, tiling, weight kind, late, option leg or None)
STEP_CASES = [(s, t, kind, late, None) for s, t in TILINGS for kind, late in KIND_STATES]
STEP_CASES += [(s, t, "pad", False, leg) for leg in sp.OPTION_LEGS for s in LEG_SHAPES for t in LEG_TILINGS[leg]
               if (s, t) in TILINGS and not NO_G16_QUANT(s, t, leg)]
# without weights the kernels accumulate the raw margin loss, (|diff| - eps)^2 per channel, in instantiations of their own
STEP_CASES += [(s, t, "none", True, leg) for leg in ("p10", "nodet") for s in LEG_SHAPES for t in (16, 64)]


def _name(s):
    return "x".join(map(str, s[0])) + f"-c{s[1]}-k" + "x".join(map(str, s[2]))


def _step_id(c):
    s, t, kind, late, leg = c
    return f"{_name(s)}-g{t}-{kind}-{'late' if late else 't7'}" + (f"-{leg}" if leg else "")


def expect_variant(name, tiling, N, weighted, graph=None, sample=False, unweighted=None):
    """Assert that ``name`` (smoe_last_fit_variant) is the kernel ``tiling`` asks for, with its marks.  Call it AFTER the
    case's own assertions: the one legitimate miss -- the duo / team tiling takes the block without weights (``unweighted``:
    what smoe_fit_variant, which asks without weights, names) but its LDS cannot hold the weighted one -- ends in a skip."""
    for t, mark, what in ((264, "duo64w2", "the joint scratch"), (816, "team16w8", "four blocks per workgroup")):
        if tiling == t and mark not in name:
            assert weighted and unweighted is not None and mark in unweighted, (name, unweighted)
            pytest.skip(f"tiling {t}: {what} + the weights of this block do not fit the LDS (without weights: {unweighted}); ran {name}")
    if tiling in (16, 32, 64):
        assert f"_g{tiling}" in name and "duo" not in name and "team" not in name and "_pair" not in name, name
    if tiling == 128:
        assert "_g64" in name and name.split("+")[0].endswith("_pair"), name
    assert ("+lw" in name) == weighted, name
    assert ("+sample" in name) == sample, name
    for g in ("ssim", "quant", "ic"):
        assert (("+" + g) in name) == (g == graph), name


_GRAPH = {"ic": "ic", "nodet_ic": "ic", "q2": "quant", "q3": "quant"}
WORST = {}


@pytest.mark.parametrize("case", STEP_CASES, ids=[_step_id(c) for c in STEP_CASES])
def test_teacher_forced_step(case):
    shape_case, tiling, kind, late, leg = case
    shape, C, kpd, yuv = shape_case
    opts = sp.OPTION_LEGS[leg] if leg else {}
    s = sp.build_state(shape_case, kind, late=late, **opts)
    assert 2 * s.clean.sum() >= s.clean.size                  # at most half of the blocks excluded
    if kind == "sample":
        assert s.flag_matters
    kw = sp.engine_kwargs(shape_case, **opts)
    eng = _engine(shape, C, s.K, **kw)
    eng0 = _engine(shape, C, s.K, **{**kw, "lr_expert": 0.0, "lr_pis": 0.0, "lr_steer": 0.0})
    try:
        eng.set_tiling(tiling)
        eng0.set_tiling(tiling)
        res = sp.check_step(eng, s, eng0=eng0)
        print(_step_id(case), res.variant, f"clean {res.clean}/{res.blocks} (dropped on a rounding tie: {res.dropped})", {k: f"{v:.3g}" for k, v in sp.worst(res.ratios).items()})
        res.require()
        assert 2 * res.clean >= res.blocks, (res.clean, res.blocks)          # the cap holds with the tie-pixel blocks taken out too
        assert eng0.last_fit_variant() == res.variant
        for k, v in sp.worst(res.ratios).items():
            WORST[k] = max(WORST.get(k, 0.0), v)
        WORST["blocks dropped on a rounding tie"] = WORST.get("blocks dropped on a rounding tie", 0) + res.dropped
        expect_variant(res.variant, tiling, int(np.prod(shape)), weighted=kind != "none", graph=_GRAPH.get(leg), sample=kind == "sample",
                       unweighted=eng.fit_variant(res.blocks))
    finally:
        eng.close()
        eng0.close()


@pytest.mark.parametrize("leg", ["q2", "q3"])
@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[3]], ids=_name)
def test_weighted_big_blocks_are_refused_by_the_16_lane_quantised_kernels(case, leg):
    """What the matrix above leaves out is refused with SMOE_ERR_UNSUPPORTED, not served by another kernel."""
    from steered_mixture_of_experts_amd import _lib
    shape, C, kpd, yuv = case
    opts = sp.OPTION_LEGS[leg]
    s = sp.build_state(case, "pad", **opts)
    eng = _engine(shape, C, s.K, **sp.engine_kwargs(case, **opts))
    eng.set_tiling(16)
    dp, st, act = sp.load_state(eng, s)
    T = torch.from_numpy(np.ascontiguousarray(np.transpose(s.tgt, (0, 2, 1)))).cuda()
    with pytest.raises(_lib.SmoeError) as e:
        eng.fit(T, dp, st, act, 1, loss_w=torch.from_numpy(s.lw).cuda())
    assert e.value.code == _lib.SMOE_ERR_UNSUPPORTED
    assert st.step == s.step and eng.last_fit_variant() == ""
    eng.close()


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module's tests: the worst error / tolerance ratio per comparison over the step cases that ran (shown with -s)."""
    yield
    if WORST:
        print("\nteacher-forced step, worst ratios:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------------------------------
# SSIM with weights passed: the loss ignores them, the LDS layout moves
# ------------------------------------------------------------------------------------------------------------------
SSIM_CASES = [(SHAPES[0], 16), (SHAPES[1], 16), (SHAPES[0], 64), (SHAPES[1], 64), (SHAPES[2], 64)]     # 16 lanes: 16x16 blocks only


@pytest.mark.parametrize("case,tiling", SSIM_CASES, ids=[f"{_name(s)}-g{t}" for s, t in SSIM_CASES])
def test_ssim_fit_ignores_the_weights_it_is_passed(case, tiling):
    """ssim_opt ignores loss_w (smoe.py:929), but off_qimg(N, has_lw, ...) moves the kernel's whole LDS layout when weights are
    passed: one step from the t = 7 state with and without them.  The same kernel: bit-identical.  Another kernel (the
    weighted block no longer fits the first choice's LDS): within the single-pass tolerance."""
    shape, C, kpd, yuv = case
    s = sp.build_state(case, "pad", ssim_opt=True)
    outs = []
    for weights in (False, True):
        eng = _engine(shape, C, s.K, **sp.engine_kwargs(case, ssim_opt=True))
        eng.set_tiling(tiling)
        dp, st, act = sp.load_state(eng, s)
        T = torch.from_numpy(np.ascontiguousarray(np.transpose(s.tgt, (0, 2, 1)))).cuda()
        LW = torch.from_numpy(s.lw).cuda() if weights else None
        loss, sse = torch.zeros(s.tgt.shape[0], device="cuda"), torch.zeros(s.tgt.shape[0], device="cuda")
        eng.fit(T, dp, st, act, 1, loss_w=LW, loss_out=loss, sse_out=sse)
        torch.cuda.synchronize()
        name = eng.last_fit_variant()
        expect_variant(name, tiling, int(np.prod(shape)), weighted=weights, graph="ssim")
        out = {"act": act.cpu().numpy(), "loss": loss.cpu().numpy(), "sse": sse.cpu().numpy()}
        for k in o.PARAM_NAMES:
            out["p:" + k], out["m:" + k], out["v:" + k] = dp[k].cpu().numpy(), st.m[k].cpu().numpy(), st.v[k].cpu().numpy()
        outs.append((name, out))
        eng.close()
    (n0, a), (n1, b) = outs
    assert (np.abs(s.lw - 1) > 0).any() and np.isfinite(a["loss"]).all()
    if n1 == n0 + "+lw":
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad
    else:
        assert np.array_equal(a["act"], b["act"])
        for k in ("loss", "sse"):
            assert (np.abs(a[k] - b[k]) <= 1e-6 + 2e-5 * np.abs(a[k])).all(), k
        for k in o.PARAM_NAMES:
            g0, g1 = (a["m:" + k] - 0.9 * s.m[k]) / 0.1, (b["m:" + k] - 0.9 * s.m[k]) / 0.1
            assert np.abs(g0 - g1).max() <= 2e-5 * np.abs(g0).max() + 10 * 2.0 ** -24 * np.abs(s.m[k]).max(), k


# ------------------------------------------------------------------------------------------------------------------
# (b) launch-split invariance
# ------------------------------------------------------------------------------------------------------------------
SPLIT_SHAPES = [SHAPES[0], SHAPES[2], SHAPES[3]]        # (16,16)/1/[2,2], (32,32)/3/[2,4], (16,16,4)/3/[2,2,1]
SPLIT_OPTS = {
    "plain": ({}, False), "pad": ({}, True), "qpis": (dict(quantize_pis=True), True),
    "q2": (sp.OPTION_LEGS["q2"], True), "q3": (sp.OPTION_LEGS["q3"], True), "ic": (dict(train_inverse_cov=True), True),
    "ssim": (dict(ssim_opt=True), True),
}
SPLIT_CASES = []
for _s in SPLIT_SHAPES:
    for _o in SPLIT_OPTS:
        if _o == "ssim" and len(_s[0]) == 3:
            continue                                     # 16x16x4: SYMMETRIC padding by 5 needs 5 frames
        for _t in (16, 64, 32, 128, 264, 816):
            if (_s, _t) not in TILINGS:
                continue
            if _o in ("q2", "q3", "ssim") and _t not in (16, 64):
                continue
            if _o == "ic" and _t not in (16, 64, 32):
                continue
            if _o == "ssim" and _t == 16 and tuple(_s[0]) != (16, 16):
                continue
            if NO_G16_QUANT(_s, _t, _o):
                continue
            SPLIT_CASES.append((_s, _t, _o))
SPLITS = ((6,), (2, 4), (1, 1, 1, 1, 1, 1))


@pytest.mark.parametrize("case,tiling,opt", SPLIT_CASES, ids=[f"{_name(s)}-g{t}-{op}" for s, t, op in SPLIT_CASES])
def test_result_does_not_depend_on_the_iterations_per_launch(case, tiling, opt):
    """6 iterations as 6, 2 + 4 and 6 x 1 launches from the same t = 7 state: bit-identical.  One block's loss0 is set so that
    its blow-up test (loss + 1 > (loss0 + 100) * 10) trips in iteration 3 exactly: it freezes in the middle of a launch in
    two of the splits, and its frozen flag crosses a launch boundary in two."""
    shape, C, kpd, yuv = case
    opts, weighted = SPLIT_OPTS[opt]
    s = sp.build_state(case, "pad", **opts)
    B = s.tgt.shape[0]
    # A few blocks get a momentum kick (a legitimate Adam state: large first moment, small second moment of their nu_e slots,
    # towards the far end of the value range): their expert levels move by ~0.03 per iteration, away from the fit, and their
    # loss rises from iteration to iteration -- candidates for the block that trips the blow-up test in iteration 3 and not
    # before (several, because a block whose kernels the warm-up has driven out of its pixels does not feel its experts)
    m, v = {k: a.copy() for k, a in s.m.items()}, {k: a.copy() for k, a in s.v.items()}
    for kick in (0, 2, 5, 6, 7, 8):           # (0: wholly valid under the padding mask)
        m["nu_e"][kick] = 0.2 if s.tgt[kick].mean() > 0.5 else -0.2          # (the step is -lr * m / sqrt(v))
        v["nu_e"][kick] = 1e-6
    s = dataclasses.replace(s, m=m, v=v)
    T = torch.from_numpy(np.ascontiguousarray(np.transpose(s.tgt, (0, 2, 1)))).cuda()
    LW = torch.from_numpy(s.lw).cuda() if weighted else None
    kw = sp.engine_kwargs(case, **opts)

    def run(split, loss0, trace=False):
        eng = _engine(shape, C, s.K, **kw)
        eng.set_tiling(tiling)
        dp, st, act = sp.load_state(eng, s)
        div = torch.zeros(B, dtype=torch.int32, device="cuda")
        loss, sse = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        l0 = None if loss0 is None else torch.from_numpy(loss0).cuda()
        per_iter = []
        for n in split:
            eng.fit(T, dp, st, act, n, loss_w=LW, diverged=div, loss0=l0, loss_out=loss, sse_out=sse)
            if trace:
                per_iter.append(loss.cpu().numpy().copy())
        torch.cuda.synchronize()
        name = (eng.last_fit_variant(), eng.fit_variant(B))
        out = {"div": div.cpu().numpy(), "act": act.cpu().numpy(), "loss": loss.cpu().numpy(), "sse": sse.cpu().numpy(),
               "b1p": np.float32(st.c.beta1_power), "b2p": np.float32(st.c.beta2_power), "step": st.step}
        for k in o.PARAM_NAMES:
            out["p:" + k], out["m:" + k], out["v:" + k] = dp[k].cpu().numpy(), st.m[k].cpu().numpy(), st.v[k].cpu().numpy()
        eng.close()
        return name, out, per_iter

    # One block has to trip the blow-up test in iteration 3 exactly.  The per-iteration losses of a run with one iteration per
    # launch and no stop test armed say which block can: one whose third loss is the largest of its first three, by more than
    # the fp32 resolution of the test's right-hand side; its loss0 goes just under the trip point of that loss.  The kernels'
    # expression is evaluated here in fp32 as they evaluate it.
    name, _, tr = run(SPLITS[2], None, trace=True)
    tr = np.stack(tr[:3]).astype(np.float32)             # (3, B)
    assert np.isfinite(tr).all()
    f1, f100, f10 = np.float32(1), np.float32(100), np.float32(10)
    trips = lambda l0, b: [bool(l + f1 > (l0 + f100) * f10) for l in tr[:, b]]
    pick = None
    for b in np.argsort(-(tr[2] - np.maximum(tr[0], tr[1]))):
        l0 = np.float32((np.float64(tr[2, b]) + 1.0) / 10.0 - 100.0)
        for _ in range(16):
            if trips(l0, b) == [False, False, True]:
                pick = (int(b), l0)
                break
            l0 = np.nextafter(l0, np.float32(-np.inf))
        if pick:
            break
    assert pick, ("no block whose loss peaks in iteration 3 by more than the resolution of the stop test",
                  tr[:, np.argsort(-(tr[2] - np.maximum(tr[0], tr[1])))[:4]])
    loss0 = np.full(B, 1e6, np.float32)
    loss0[pick[0]] = pick[1]
    runs = [run(sp_, loss0) for sp_ in SPLITS]
    ref = runs[0][1]
    assert ref["div"][pick[0]] == 1 and ref["div"].sum() == 1, ref["div"]
    assert ref["step"] == s.step + 6
    for (nm, out, _), split in zip(runs[1:], SPLITS[1:]):
        assert nm == runs[0][0]
        bad = [k for k in ref if not np.array_equal(ref[k], out[k], equal_nan=True)]
        assert not bad, (split, bad, {k: float(np.abs(ref[k].astype(np.float64) - out[k].astype(np.float64)).max()) for k in bad})
    assert runs[0][0] == name
    expect_variant(name[0], tiling, int(np.prod(shape)), weighted=weighted,
                   graph={"q2": "quant", "q3": "quant", "ic": "ic", "ssim": "ssim"}.get(opt), unweighted=name[1])
