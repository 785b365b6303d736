"""Teacher-forced step parity: ONE Adam step of an engine from a state with non-trivial slots, against the restatement.

TEST INFRASTRUCTURE, device-agnostic: ``check_step`` drives a ``BlockEngine`` (GPU) or the ``OracleEngine`` test double (CPU)
through the same interface; tensors go on ``eng.device``.

Why one step from a prepared state.  The first Adam step from zero slots is ``lr * g / (|g| + 3e-7)``: a sign, blind to
gradient magnitudes, to the bias correction and to the running beta powers.  Trajectories at the reference's learning rates are
chaotic and can only be judged by medians.  A step from a state the fp32 restatement reached after seven
iterations -- with its slots, beta powers and pruned kernel lists loaded into the engine -- has neither problem: every
element is compared, and nothing is amplified over iterations.

The pixel lattice (2^precision - 1 levels) makes loss and gradients discontinuous at rounding ties, so the engine's OWN
lattice (from its evaluation pass; a zero-learning-rate fit launch shows that the fit kernel's lattice is the same) is fed to
both restatements as ``q_override``.  The fp64 restatement's own lattice is never used: it differs from an fp32 one in a few
pixels per block, which alone moves gradients by 6e-4 of their scale.  What is fed to the restatements is itself compared
with the fp32 restatement's own lattice ("lattice" below): an engine that quantised to another number of levels would
otherwise agree with the restatement it was handed.

Bounds (all but the lattice on "clean" blocks: no gate value on the influence threshold, no blend on the clip edge):
  lattice     every pixel of every block: the engine's evaluation-pass reconstruction against the fp32 restatement's own
              lattice: equal (1e-7) off rounding ties of the quantiser, at most one level, 1 / (2^p - 1), where the fp64 blend
              times 2^p - 1 sits within 2e-4 of a half-integer (test_forward_parity's bound, generalised from 255 levels)
  loss, sse   rtol 2e-5, the single-pass tolerance of tests/test_gpu_parity.py, against the fp64 pass on the same lattice
  list        equal to the restatement's
  gradients   recovered from the slots, g = (m' - beta1 m) / (1 - beta1):  |g - g64| <= 2e-5 max|g64| per tensor (the bound
              of test_one_step_parity) + 10 * 2^-24 * max(|m|, |m'|), the fp32 rounding of m' that the recovery divides
              by 1 - beta1 = 0.1
  v'          against the fp32 restatement: 2 |g| dg (1 - beta2) + dg^2 (1 - beta2) + 4 ulp, dg = the gradient bound above
  parameters  against the fp32 restatement's adam_step.  The update is lr * bias * m' / (sqrt(v') + eps) with
              bias = sqrt(1 - beta2^t) / (1 - beta1^t); a gradient error dg moves m' by 0.1 dg and sqrt(v') by
              0.001 |g| dg / sqrt(v'):
              tol = 1e-6 (|p| + 1) + 2e-5 lr + lr bias [0.1 dg / (sqrt(v') + eps) + |m'| 0.001 |g| dg / (sqrt(v') (sqrt(v') + eps)^2)]
              (test_one_step_parity's tolerance generalised to t > 1)
  untrained   with lr == 0, radial_as (A_corr) or train_* = False the variable and both of its slots are bit-unchanged, on
              every block and every tiling (include/smoe_hip.h, smoe_fit)
"""
import dataclasses
import functools
import os
import sys

import numpy as np
import torch

from oracle import smoe_oracle as o
from test_gpu_parity import SHAPES, _bits_to_mask, _mask_to_bits, _setup

# One definition of the weight kinds, the quantisation ranges and the warm-up length, shared with the randomised sweep.  It
# lives in scripts/fuzz_parity.py because tests/test_gpu_fuzz.py imports that module and nothing else of this file's making.
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from fuzz_parity import QKW, WARMUP, make_weights          # noqa: E402


LATE = 150          # "late" state: the same slots with the beta powers of step 150 (bias correction nearly 1 for beta1, 0.37 for beta2)
KINDS = ("none", "pad", "frac", "sample")
CORNER_BLOCKS = (2, 5, 6, 7, 8, 9)   # "sample": candidates for the block whose kernel 0 only reaches pixels the sample did not draw

# lr_steer 1e-2 where the warm-up at the reference's 1.0 leaves a degenerate state: with gradient clipping every steering entry
# moves by ~1 per iteration whatever its gradient, the kernels collapse and most blocks get pixels no kernel reaches (y = 0
# exactly: on the clip edge, excluded); with the 14-bit steering lattice of QKW a diagonal entry that crosses 0 quantises to
# exactly 0, where the reference's own gradient (1 / A_ll of the determinant factor) is infinite
OPTION_LEGS = {
    "l1clip": dict(pis_l1=0.3, u_l1=0.002, grad_clip=2e-4, lr_steer=1e-2),
    "qpis": dict(quantize_pis=True),
    "ic": dict(train_inverse_cov=True),
    "q2": dict(quantization_mode=2, quantize_pis=True, lr_steer=1e-2, **QKW),
    "q3": dict(quantization_mode=3, quantize_pis=True, lr_steer=1e-2, **QKW),
    # the switches off their defaults, lr_steer at its default: the normaliser without the determinant factor (and the
    # su / A_ll term of the diagonal steering gradient gone with it), alone and on the inverse-covariance graph
    "nodet": dict(use_determinant=False),
    "nodet_ic": dict(use_determinant=False, train_inverse_cov=True),
    # one frozen tensor each; train_gammas=False also takes the slopes out of the forward graph
    "fz_pis": dict(train_pis=False),
    "fz_mus": dict(train_musx=False),
    "fz_gam": dict(train_gammas=False),
    # the lattice, the influence threshold and the margin follow the precision
    "p10": dict(precision=10),
    "p6": dict(precision=6),
    # 0.25: eps = margin / 2^p must stay clear of the lattice step 1 / (2^p - 1).  At margin 1.0 (1/256 against 1/255) pixels
    # one level off contribute a cancelled residue |d| - eps and the fp32 restatement alone uses 0.19 of the gradient
    # tolerance, at 1.5 more than half of it; at 0.25 it stays below 0.07
    "margin": dict(margin=0.25),
    # a normaliser of the l1 term that is no kernel count in use (4, 8, 36, 32, 272)
    "startpis": dict(pis_l1=0.3, start_pis=9),
}


def influence_threshold(cfg):
    """(tau, window): the influence threshold 0.5 / 2^precision of the gate and the half-width of the band around it in which a
    gate value makes its block's gradient discontinuous.  The band scales with the threshold, 1e-6 * 2^(8 - precision): 0.05 %
    of tau at every precision, and 0.5 / 256 with 1e-6 exactly at 8 bits."""
    return 0.5 / 2 ** cfg.precision, 1e-6 * 2.0 ** (8 - cfg.precision)


def lattice_check(judge, q, y32, y64, cfg):
    """The "lattice" comparison of the module docstring, shared with tests/shared_step_parity.py.  ``q``: the engine's
    reconstruction; ``y32`` / ``y64``: the blends of the fp32 / fp64 restatement."""
    own = o.fake_quant01(y32, cfg.precision, np.float32)
    levels = 2 ** cfg.precision - 1
    frac = (np.clip(y64, 0, 1) * levels + 0.5) % 1.0
    tie = (frac < 2e-4) | (frac > 1 - 2e-4)
    d = np.abs(q - own)
    judge("lattice", d[~tie], 1e-7)
    judge("lattice_tie", d, 1.0001 / levels)


def blocks_for(shape):
    """Batch sizes that are ragged for every tiling (not a multiple of 4 blocks per wavefront / workgroup) and for which the
    restatement alone keeps at least half of the blocks clean (checked by tests/test_step_parity_cpu.py)."""
    return 37 if int(np.prod(shape)) >= 1024 else 21


def _freeze(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))


@dataclasses.dataclass
class State:
    cfg: object
    K: int
    coords: np.ndarray
    tgt: np.ndarray          # (B,N,C)
    lw: object               # (B,N) or None
    fed: object              # (B,N) bool or None ("sample")
    p: dict
    m: dict
    v: dict
    b1p: np.float32
    b2p: np.float32
    step: int
    active: np.ndarray       # (B,K) bool
    clean: np.ndarray        # (B,) bool, from the fp64 restatement at this state
    corner: int              # "sample": the block whose kernel 0 only reaches pixels the sample did not draw
    flag_matters: bool       # "sample": the new list of that block differs with / without the sample flag


def _prepare_params(p, cfg, shape):
    d = len(shape)
    if cfg.quantization_mode == 3:          # mode 3 assumes A_corr zero on and above the diagonal (include/smoe_hip.h)
        p["A_corr"] = (p["A_corr"] * np.tril(np.ones((d, d), np.float32), -1)).astype(np.float32)
    if cfg.train_inverse_cov:               # A is the inverse covariance itself: positive diagonal, moderate correlations
        p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
        p["A_corr"] = (p["A_corr"] * 0.3).astype(np.float32)


def _ref_pass(st_p, s, dtype, q):
    """The restatement's pass at the state's parameters on the lattice ``q``.  With quantization_mode 2 / 3 the fp64 pass runs
    on the fp32-quantised parameters (the lattice points of an fp64 fake-quantiser are not those of the fp32 one the kernels and
    TF use) and routes the gradients back through the fp32 quantiser's masks, as scripts/fuzz_parity.py does."""
    cfg = s.cfg
    lw = None if cfg.ssim_opt else s.lw
    if dtype == np.float64 and cfg.quantization_mode >= 2:
        q32, back, _ = o.quantize_graph_params(st_p, cfg, np.float32)
        cfg0 = o.OracleConfig(**{**cfg.__dict__, "quantization_mode": 0, "quantize_pis": False})
        ref = o.forward(q32, s.tgt, s.coords, s.active, cfg0, lw, np.float64, want_grads=True, q_override=q, fed=s.fed)
        ref["grads"] = o.route_quant_grads(ref["grads"], back, np.float64)
        return ref
    return o.forward(st_p, s.tgt, s.coords, s.active, cfg, lw, dtype, want_grads=True, q_override=q, fed=s.fed)


@functools.lru_cache(maxsize=None)
def _build(shape, C, kpd, yuv, B, seed, opts, kind):
    if kind != "sample":
        return _build_one(shape, C, kpd, yuv, B, seed, opts, kind, CORNER_BLOCKS[0])
    for corner in CORNER_BLOCKS:        # the corner block has to be among the compared ones, or the flag would go unchecked
        s = _build_one(shape, C, kpd, yuv, B, seed, opts, kind, corner)
        if s.clean[corner] and s.flag_matters:
            return s
    raise AssertionError("no candidate corner block is clean and sensitive to the sample flag")


def _build_one(shape, C, kpd, yuv, B, seed, opts, kind, corner):
    kw = dict(opts)
    cfg, p, coords, tgt, K = _setup(shape, C, list(kpd), yuv, B, seed, **kw)
    _prepare_params(p, cfg, shape)
    rng = np.random.default_rng(seed + 17)
    active = rng.uniform(size=(B, K)) < 0.85               # a partial list: about 15 % of the bits cleared
    p["pis"][3, 0] = 0.0                                   # pis <= 0 kernels are absent (smoe.py:480)
    p["pis"][4, K - 1] = -0.1
    lw, fed = make_weights(kind, shape, B, rng, corner)
    if kind == "sample":
        p["A_diagonal"][corner, 0] *= 6.0            # kernel 0 of that block: narrow, around its centre
        active[corner, 0] = True
    st = o.new_adam_state(p)
    p = {k: v.astype(np.float32) for k, v in p.items()}
    for _ in range(WARMUP):
        f = o.forward(p, tgt, coords, active, cfg, None if cfg.ssim_opt else lw, np.float32, want_grads=True, fed=fed)
        active = f["active_new"]
        p = o.adam_step(p, f["grads"], st, cfg, np.float32)
    flag_matters = False
    if kind == "sample":
        # the warm-up pruned kernel 0 of the corner block (no fed pixel feels it; unlisted, it has not moved).  Re-admitted
        # -- as update_kernel_list does every val_iter iterations -- the step under test has to decide about it again
        active = active.copy()
        active[corner, 0] = True
        a_s = o.forward(p, tgt, coords, active, cfg, lw, np.float32, fed=fed)["active_new"]
        a_m = o.forward(p, tgt, coords, active, cfg, lw, np.float32)["active_new"]
        flag_matters = bool(a_m[corner, 0] and not a_s[corner, 0])
    r64 = o.forward(p, tgt, coords, active, cfg, None if cfg.ssim_opt else lw, np.float64, fed=fed)
    # blocks with a gate value on the influence threshold or a blend on the clip edge: discontinuous gradient there
    tau, window = influence_threshold(cfg)
    tie = (np.abs(r64["w"] - tau) < window).any(axis=(1, 2))
    edge = ((np.abs(r64["y"]) < 1e-6) | (np.abs(r64["y"] - 1) < 1e-6)).any(axis=(1, 2))
    for d in (p, st["m"], st["v"]):
        for a in d.values():
            a.setflags(write=False)
    return State(cfg=cfg, K=K, coords=coords, tgt=tgt, lw=lw, fed=fed, p=p, m=st["m"], v=st["v"],
                 b1p=np.float32(st["b1p"]), b2p=np.float32(st["b2p"]), step=WARMUP, active=active, clean=~(tie | edge),
                 corner=corner, flag_matters=flag_matters)


def build_state(case, kind, late=False, B=None, seed=None, **opts):
    """The state of ``case`` = (block_shape, C, kernels_per_dim, use_yuv) after WARMUP fp32 iterations with weight kind
    ``kind``; ``late``: the same parameters and slots with the beta powers (fp32 running products) of step LATE.  Cached: the
    tilings of a shape share one run of the restatement."""
    shape, C, kpd, yuv = case
    B = blocks_for(shape) if B is None else B
    seed = 300 + len(shape) + C if seed is None else seed
    s = _build(tuple(shape), C, tuple(kpd), bool(yuv), B, seed, _freeze(opts), kind)
    if late:
        b1, b2 = np.float32(s.cfg.beta1), np.float32(s.cfg.beta2)
        b1p, b2p = b1, b2
        for _ in range(LATE):
            b1p, b2p = np.float32(b1p * b1), np.float32(b2p * b2)
        s = dataclasses.replace(s, b1p=b1p, b2p=b2p, step=LATE)
    return s


def engine_kwargs(case, **opts):
    return dict(use_yuv=case[3], **opts)


def _dev(a, eng):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def load_state(eng, s):
    """(params, AdamState, active) of the engine at state ``s``."""
    dp = {k: _dev(v.astype(np.float32), eng) for k, v in s.p.items()}
    st = eng.new_adam_state(dp)
    for k in o.PARAM_NAMES:
        st.m[k].copy_(_dev(s.m[k].astype(np.float32), eng))
        st.v[k].copy_(_dev(s.v[k].astype(np.float32), eng))
    st.c.beta1_power, st.c.beta2_power, st.c.step = float(s.b1p), float(s.b2p), int(s.step)
    act = _dev(_mask_to_bits(s.active).view(np.int32), eng)
    return dp, st, act


def _host(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


@dataclasses.dataclass
class Result:
    ratios: dict             # comparison -> worst error / tolerance (<= 1 passes)
    failures: list
    clean: int
    blocks: int
    variant: str
    dropped: int = 0         # blocks left out because the fit kernel's lattice differs from the evaluation kernel's on a rounding tie

    def require(self):
        assert not self.failures, (self.failures, self.ratios, self.variant)
        return self


def _lr(cfg, name):
    return {"pis": cfg.lr_pis, "A_diagonal": cfg.lr_steer, "A_corr": cfg.lr_steer}.get(name, cfg.lr_expert)


def judge_adam(judge, name, cfg, lr, bias, g64, dg, m0, mn, mr, vr, vn, pr, pn):
    """The three comparisons of one tensor after one Adam step (module docstring), shared with tests/shared_step_parity.py.
    ``g64``: the UNCLIPPED fp64 gradient, ``dg``: its error bound; ``m0``: the first-moment slots before the step; ``mn``,
    ``vn``, ``pn``: the engine's slots and parameters after it; ``mr``, ``vr``, ``pr``: the fp32 restatement's."""
    b1, b2, eps = float(np.float32(cfg.beta1)), float(np.float32(cfg.beta2)), float(cfg.adam_eps)
    if cfg.grad_clip is not None:
        g64 = np.clip(g64, -cfg.grad_clip, cfg.grad_clip)
    m0, mn = m0.astype(np.float64), mn.astype(np.float64)
    g = (mn - b1 * m0) / (1.0 - b1)
    judge("grad:" + name, np.abs(g - g64), dg + 10 * 2.0 ** -24 * np.maximum(np.abs(m0), np.abs(mn)))
    vr, vn = vr.astype(np.float64), vn.astype(np.float64)
    judge("v:" + name, np.abs(vn - vr), (2 * np.abs(g64) * dg + dg * dg) * (1.0 - b2) + 4 * 2.0 ** -24 * np.abs(vr) + 1e-37)
    pr = pr.astype(np.float64)
    rv = np.sqrt(vr)
    with np.errstate(divide="ignore", invalid="ignore"):
        second = np.abs(mr.astype(np.float64)) * (1.0 - b2) * np.abs(g64) * dg / (rv * (rv + eps) ** 2)
    second = np.where(rv > 0, second, 0.0)
    tol = 1e-6 * (np.abs(pr) + 1.0) + 2e-5 * lr + lr * bias * ((1.0 - b1) * dg / (rv + eps) + second)
    judge("param:" + name, np.abs(pn.astype(np.float64) - pr), tol)


def check_step(eng, s, eng0=None):
    """Load ``s`` into ``eng``, run ONE fit iteration and compare with the restatement (module docstring).  ``eng0``: an engine
    of the same configuration and tiling with every learning rate 0, for the proof that the fit kernel's lattice is the
    evaluation kernel's.  Returns a ``Result``; nothing is asserted here but the facts about the launch itself."""
    cfg, B = s.cfg, s.tgt.shape[0]
    sample = s.fed is not None
    T = _dev(np.transpose(s.tgt, (0, 2, 1)), eng)
    LW = None if s.lw is None else _dev(s.lw, eng)
    fails, ratios = [], {}

    def judge(name, err, tol):
        r = float(np.max(err / tol)) if np.size(err) else 0.0          # (every tolerance is > 0; a NaN fails)
        ratios[name] = max(ratios.get(name, 0.0), r)
        if not r <= 1.0:
            fails.append((name, r))

    # the implementation's own lattice at these parameters (evaluation kernel)
    dp, st, act = load_state(eng, s)
    fw = eng.forward(T, dp, act, loss_w=LW, want_recon=True, update_active=False)
    q = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    fw_loss, fw_sse = fw["loss"].cpu().numpy(), fw["sse"].cpu().numpy()
    ref = _ref_pass(s.p, s, np.float32, q)
    ref64 = _ref_pass(s.p, s, np.float64, q)
    lattice_check(judge, q, ref["y"], ref64["y"], cfg)
    clean = s.clean
    dropped = 0
    if eng0 is not None:
        # A fit launch that moves nothing reports the loss / SSE of its own pass: a pixel an LSB apart moves a block's SSE or
        # loss by 2e-5 .. 1e-4 relative and more.  EVERY block, weights included.  The two kernels sum a block's N * C squared
        # errors in different orders: sqrt(N C) * 2^-24 is the random-walk size of one fp32 sum's rounding error, 4 x that the
        # tolerance for the difference of two (3.8e-6 for 256 values, 1.3e-5 for 3 072), never below the 2e-6 of
        # test_one_step_parity.  Why not its flat 2e-6: that test sums 21 blocks of fresh parameters and happens to stay under
        # it; from the t = 7 states the 3 072-value blocks of 16x16x4 RGB came out 4e-6 .. 5e-6 apart (quantize_pis on the duo
        # and team tilings, mode 2 on 64 lanes) in cases whose gradients, slots and parameters all sat below half of their
        # tolerances -- the same lattice, summed in another order.  The smallest difference seen from a real pixel an LSB
        # apart was 1.8e-5 on such a block; Result.dropped counts the blocks taken out, and the callers log it.
        # The fit kernels of the wide tilings hoist other terms than the evaluation kernel, so their blends can differ in the
        # last bit and a pixel ON a rounding tie of the quantiser may land one level apart (test_forward_parity allows the
        # evaluation kernel itself 1 LSB within 2e-4 of a tie).  A block whose lattices differ must have such a pixel -- anything
        # else is a failure -- and is not compared further: the lattice fed to the restatements is not the fit kernel's there.
        dp0, st0, act0 = load_state(eng0, s)
        l0 = torch.zeros(B, device=eng0.device)
        s0 = torch.zeros(B, device=eng0.device)
        eng0.fit(T, dp0, st0, act0, 1, loss_w=LW, loss_out=l0, sse_out=s0, loss_w_is_sample=sample)
        for k, v in _host(dp0).items():
            assert np.array_equal(v, s.p[k].astype(np.float32)), k          # zero learning rates: nothing moved,
        for k in o.PARAM_NAMES:                                             # the slots neither
            assert np.array_equal(st0.m[k].cpu().numpy(), s.m[k].astype(np.float32)), ("m", k)
            assert np.array_equal(st0.v[k].cpu().numpy(), s.v[k].astype(np.float32)), ("v", k)
        rt = max(2e-6, 4.0 * np.sqrt(s.tgt.shape[1] * s.tgt.shape[2]) * 2.0 ** -24)
        e_s, t_s = np.abs(s0.cpu().numpy() - fw_sse), 1e-9 + rt * np.abs(fw_sse)
        e_l, t_l = np.abs(l0.cpu().numpy() - fw_loss), 1e-12 + rt * np.abs(fw_loss)
        differs = ~((e_s <= t_s) & (e_l <= t_l))
        if differs.any():
            frac = (np.clip(ref64["y"], 0, 1) * (2 ** cfg.precision - 1) + 0.5) % 1.0
            on_tie = ((frac < 2e-4) | (frac > 1 - 2e-4)).any(axis=(1, 2))
            differs &= on_tie              # (what differs without a tie pixel stays in and fails below)
            clean = clean & ~differs
            dropped = int(differs.sum())
        judge("lattice_sse", e_s[~differs], t_s[~differs])
        judge("lattice_loss", e_l[~differs], t_l[~differs])
    ast = {"m": {k: v.copy() for k, v in s.m.items()}, "v": {k: v.copy() for k, v in s.v.items()}, "t": s.step,
           "b1p": s.b1p, "b2p": s.b2p}
    p_ref = o.adam_step({k: v.copy() for k, v in s.p.items()}, ref["grads"], ast, cfg, np.float32)

    loss = torch.zeros(B, device=eng.device)
    sse = torch.zeros(B, device=eng.device)
    eng.fit(T, dp, st, act, 1, loss_w=LW, loss_out=loss, sse_out=sse, loss_w_is_sample=sample)
    if eng.device.type == "cuda":
        torch.cuda.synchronize()
    assert st.step == s.step + 1
    variant = eng.last_fit_variant()
    c = clean

    lo, ss = loss.cpu().numpy(), sse.cpu().numpy()
    # (against the fp64 pass on the same lattice: an fp32 reference would add its own summation error to the comparison)
    judge("loss", np.abs(lo - ref64["loss"])[c], (1e-6 + 2e-5 * np.abs(ref64["loss"]))[c])
    judge("sse", np.abs(ss - ref64["sse"])[c], (1e-6 + 2e-5 * np.abs(ref64["sse"]))[c])
    new = _bits_to_mask(act.cpu().numpy().view(np.uint32), s.K)
    if not np.array_equal(new[c], ref["active_new"][c]):
        fails.append(("list", int((new[c] != ref["active_new"][c]).sum())))
    ratios["list"] = float((new[c] != ref["active_new"][c]).sum())

    m1, v1, got = _host(st.m), _host(st.v), _host(dp)
    bias = np.sqrt(1.0 - float(s.b2p)) / (1.0 - float(s.b1p))
    for name in o.PARAM_NAMES:
        lr = _lr(cfg, name)
        trainable = {"gamma_e": cfg.train_gammas, "musX": cfg.train_musx, "pis": cfg.train_pis,
                     "A_corr": not cfg.radial_as}.get(name, True)
        if not trainable or lr == 0:
            # (every block, clean or not: the variable and both slots bit-unchanged)
            moved = [w for w, a, a0 in (("p", got[name], s.p[name]), ("m", m1[name], s.m[name]), ("v", v1[name], s.v[name]))
                     if not np.array_equal(a, a0.astype(np.float32))]
            ratios["moved:" + name] = float(len(moved))
            if moved:
                fails.append(("moved:" + name, "/".join(moved)))
            continue
        g64 = ref64["grads"][name][c]
        # (with grad_clip the kernel clips a gradient whose rounding error is that of the UNCLIPPED tensor: its scale, as in
        # test_fit_with_loss_weights_regularisers_and_clipping)
        scale = float(np.abs(g64).max()) + 1e-30 if g64.size else 1e-30
        judge_adam(judge, name, cfg, lr, bias, g64, 2e-5 * scale, s.m[name][c], m1[name][c], ast["m"][name][c], ast["v"][name][c],
                   v1[name][c], p_ref[name][c], got[name][c])
    return Result(ratios=ratios, failures=fails, clean=int(c.sum()), blocks=B, variant=variant, dropped=dropped)


def worst(ratios):
    """{comparison kind: worst ratio} of a Result's per-tensor ratios (for logs)."""
    out = {}
    for k, r in ratios.items():
        kind = k.split(":")[0]
        out[kind] = max(out.get(kind, 0.0), r)
    return out


__all__ = ["SHAPES", "KINDS", "OPTION_LEGS", "QKW", "build_state", "check_step", "engine_kwargs", "judge_adam", "load_state", "worst",
           "blocks_for", "influence_threshold", "lattice_check", "WARMUP", "LATE"]
