"""Teacher-forced step parity of the shared-kernel whole-image fit: ONE Adam step of a ``SharedEngine`` (GPU) or of the
``OracleSharedEngine`` test double (CPU) from a state with non-trivial slots and sparse kernel lists, element by element
against the restatement.  TEST INFRASTRUCTURE, device-agnostic, the shared-mode sibling of tests/step_parity.py (read its
docstring first: why one step from a prepared state, why the engine's own pixel lattice is fed to both restatements).

What is different here.  One kernel set serves every batch: a pass leaves one gradient row per batch, the step sums the rows
of the batches visited since the last step (smoe_shared_accumulate promises exactly that sum) and takes ONE dense Adam step.
A gradient is discontinuous in a batch that has a gate value on the influence threshold or a blend on the clip edge, so
``check_shared_step`` accumulates the CLEAN batches only (one call per contiguous run of them) -- after a full pass whose rows
it discards, so that every row of a batch it does not revisit is stale -- and can then compare every element of every
tensor without loosening anything for the rest.

Bounds (tests/step_parity.judge_adam carries the Adam formulas for both modes):
  lattice     the engine's reconstruction against the fp32 restatement's: equal off rounding ties of the quantiser, at most
              one level, 1 / (2^precision - 1), on them (step_parity.lattice_check; test_shared_forward_parity's bound)
  loss, sse   per clean batch against the fp64 pass on the engine's lattice: 1e-6 + 2e-5 |ref|
  lists       the new lists of the clean batches equal the fp32 restatement's (with overlap: those of its halo pass); the
              lists of the batches that were not revisited are untouched
  gradients   recovered from the slots, against the fp64 SUM over the clean batches.  dg = 2e-5 max_elem sum_b |g64_b|: the
              single-pass bound of 2e-5 of the tensor scale holds per batch, and the errors of the batches add at worst
              linearly; + 10 * 2^-24 max(|m|, |m'|) for the recovery
  v', params  against the fp32 restatement's adam_step on that fp64 sum rounded to fp32, with the v and parameter tolerances
              of step_parity at this dg.  Why not on the fp32 pass's own gradients, as the block checker does: those
              tolerances allow the ENGINE's gradient an error of dg and the reference's none.  For the margin-loss graphs the
              fp32 numpy pass is within 0.03 dg of the fp64 one and it makes no difference; its SSIM graph is itself
              1.15 - 1.17 dg off (measured on the 64x80 / 16x16 / 3 state: grad:pis 1.15, grad:gamma_e 1.12, grad:nu_e 1.17),
              and with it as the reference v:pis of the MI355X kernel read 1.26 while the kernel's recovered gradient sat at
              0.18 dg from fp64 -- the reference's error charged to the engine.  Fed with the fp64 sum the same case reads
              0.39; the tolerances are unchanged and the recovered-gradient comparison runs against fp64 either way
  coasting    one kernel with non-zero slots is cleared from every list: TF's dense ApplyAdam still moves it with g = 0.  For
              it dg = 0: the recovered gradient is 0 within the recovery term, the slots are beta1 m and beta2 v as the fp32
              formula rounds them (4 ulp), and the parameters have moved wherever the restatement moved them
  untrained   with lr == 0, radial_as (A_corr) or train_* = False the variable and both slots are bit-unchanged
  bookkeeping step + 1, both beta powers one fp32 product further

``check_paths``: from the same state, smoe_shared_fit (the fused gather inside the step kernel; quantization_mode 3: gather
kernel + the one-workgroup routed step) equals accumulate + apply bit for bit, for 1 and for 3 iterations.  Both sum a kernel's
rows through gather_kernel_sums in the same order and step through the same kernel_apply.  With check_shared_step this
carries the element-wise result over to smoe_shared_fit, which can only run all batches.
"""
import dataclasses
import functools

import numpy as np
import torch

import step_parity as sp
from oracle import smoe_oracle as o
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.engine import SharedConfig
from test_gpu_shared import _bits, _mask, _setup

WARMUP, LATE = sp.WARMUP, sp.LATE

# id -> image shape, batch shape, C, kernels per dim, yuv: the smallest shapes that reach
CASES = {
    "A": ((136, 136), (8, 8), 1, (6, 6), False),        # 289 batches: a second gather trip of 33 live lanes + the clamped tail
    "B": ((72, 80), (8, 8), 3, (6, 6), True),           # 90 batches: the u = 1 rows of the first trip real for 26 lanes
    "C": ((48, 48), (16, 16), 1, (16, 17), False),      # 272 kernels: two compaction rounds, 9 list words (odd), lists over SH_KC
    "C3": ((32, 48), (16, 16), 3, (16, 17), True),      # the same with three-channel records
    "D": ((40, 40, 8), (8, 8, 2), 3, (4, 4, 2), True),  # 3-d, 100 batches
    "S": ((64, 80), (16, 16), 3, (6, 6), True),         # B-sized with 16x16 batches: the SSIM window needs them
}

# offsets of use_diff_center are quantised on their own range (as test_shared_fake_quantised_centre_offsets)
_DC = dict(bit_depths=(14, 10, 8, 10, 10), lower_bounds=(-60, -.03, -1, 0, -4), upper_bounds=(60, .04, 2, 2, 4))
# ``weights`` (a padding mask through set_loss_weights) and ``diff_center`` (set_center_grid) are this module's own switches,
# ``overlap`` is the engine's alone; everything else goes to the engine's and the restatement's configuration alike
OPTION_LEGS = {
    **sp.OPTION_LEGS,
    "startpis": dict(pis_l1=0.3, start_pis=50),                 # (the block leg's 9 with a count that is no K of CASES)
    "l1": dict(pis_l1=0.3, u_l1=0.002, lr_steer=1e-2),          # l1clip without the clipping, which leaves the step only the signs
    "radial": dict(radial_as=True),
    "dcq2": dict(diff_center=True, quantization_mode=2, quantize_pis=True, lr_steer=1e-2, **_DC),
    "lw": dict(weights=True),
    "ov3": dict(overlap=3),
    "ssim": dict(ssim_opt=True),
}
_OWN = ("weights", "diff_center", "overlap")
COAST_TENSORS = ("nu_e", "musX", "A_diagonal")          # the coasting kernel has non-zero slots in each of these that is trained


def trained(cfg, name):
    """Whether the configuration's optimiser moves tensor ``name`` at all (its group's rate, train_*, radial_as)."""
    return bool(sp._lr(cfg, name) != 0 and {"gamma_e": cfg.train_gammas, "musX": cfg.train_musx, "pis": cfg.train_pis,
                                            "A_corr": not cfg.radial_as}.get(name, True))


@dataclasses.dataclass
class SharedState:
    case: tuple
    opts: dict
    cfg: object
    K: int
    NB: int
    coords: np.ndarray       # (NB,Nb,d)
    halo: object             # (NB,Next,d) or None
    tgt: np.ndarray          # (NB,Nb,C)
    lw: object               # (NB,Nb) or None
    grid: object             # (K,d) or None (use_diff_center)
    p: dict                  # leading axis 1
    m: dict
    v: dict
    b1p: np.float32
    b2p: np.float32
    step: int
    lists: np.ndarray        # (NB,K) bool
    clean: np.ndarray        # (NB,) bool, from the fp64 restatement at this state
    coast: int               # the kernel cleared from every list
    absent: tuple            # the kernels with prior 0 and < 0: listed everywhere, trained nowhere


def _prepare(p, cfg, img, kpd, rng, diff_center):
    d = p["musX"].shape[-1]
    K = p["pis"].shape[1]
    if cfg.quantization_mode == 3:          # mode 3 assumes A_corr zero on and above the diagonal (include/smoe_hip.h)
        p["A_corr"] = (p["A_corr"] * np.tril(np.ones((d, d), np.float32), -1)).astype(np.float32)
    if cfg.train_inverse_cov:               # A is the inverse covariance itself: positive diagonal, moderate correlations
        p["A_diagonal"] = (p["A_diagonal"] ** 2).astype(np.float32)
        p["A_corr"] = (p["A_corr"] * 0.3).astype(np.float32)
    if cfg.radial_as:                       # one steering value per kernel, tiled over the diagonal; A_corr untrained
        a0 = np.abs(p["A_diagonal"][0, :, 0, 0])
        p["A_diagonal"] = (a0[None, :, None, None] * np.eye(d)).astype(np.float32)
        p["A_corr"] = np.zeros_like(p["A_corr"])
    grid = None
    if diff_center:
        grid = blk.init_block_params(img[None], list(kpd), True, False)["musX"][0].astype(np.float32)
        off = rng.uniform(-0.02, 0.02, size=grid.shape).astype(np.float32)
        off[5, 0] = 0.05                    # outside the fixed offset range: clamped, no gradient
        p["musX"] = (grid + off)[None].astype(np.float32)
    p["pis"][0, 3] = 0.0                    # pis <= 0 kernels are absent (smoe.py:480), listed or not
    p["pis"][0, K - 2] = -0.1
    return grid


def _pass(p, s_or, lists, dtype, want_grads=False):
    cfg, tgt, coords, halo, lw = s_or
    return o.shared_pass(p, tgt, coords, lists, cfg, dtype, want_grads=want_grads, halo_coords=halo,
                         loss_w=None if cfg.ssim_opt else lw)


@functools.lru_cache(maxsize=None)
def _build(case, seed, frozen):
    shape, bshape, C, kpd, yuv = case
    opts = dict(frozen)
    own = {k: opts.pop(k) for k in _OWN if k in opts}
    img, p, cfg, coords, tgt, K, NB = _setup(shape, bshape, C, list(kpd), yuv, seed=seed, **opts)
    rng = np.random.default_rng(seed + 17)
    grid = _prepare(p, cfg, img, kpd, rng, own.get("diff_center", False))
    if grid is not None:
        cfg = o.OracleConfig(**{**cfg.__dict__, "mus_grid": grid[None]})
    ov = int(own.get("overlap", 0))
    halo = o.global_halo_coords(shape, bshape, ov) if ov else None
    lw = None
    if own.get("weights"):                  # a padding mask: the last rows and columns of the image do not count
        lw = (~((coords[..., 0] > 0.9) | (coords[..., 1] > 0.88))).astype(np.float32)
        assert 0 < (lw == 0).all(axis=1).sum() and ((lw == 0).any(axis=1) & (lw == 1).any(axis=1)).any()
    env = (cfg, tgt, coords, halo, lw)
    p = {k: v.astype(np.float32) for k, v in p.items()}
    st = o.new_adam_state(p)
    lists = _pass(p, env, np.ones((NB, K), bool), np.float32)["lists_new"]          # the iteration-0 pass
    for _ in range(WARMUP):
        f = _pass(p, env, lists, np.float32, want_grads=True)
        lists = f["lists_new"]
        p = o.adam_step(p, f["grads"], st, cfg, np.float32)
    # the coasting kernel: non-zero slots, cleared from every list (of the candidates, the one the fewest batches lose)
    lists = lists.copy()
    # (of the tensors this configuration trains: the slots of a frozen one stay zero)
    moving = np.all([np.any(st["m"][k][0].reshape(K, -1) != 0, axis=1) for k in COAST_TENSORS if trained(cfg, k)], axis=0)
    cand = np.flatnonzero(moving & (p["pis"][0] > 0) & lists.any(axis=0))
    assert cand.size, "no kernel with non-zero slots to coast"
    coast = int(cand[np.argmin(lists[:, cand].sum(axis=0))])
    lists[:, coast] = False
    absent = (3, K - 2)
    lists[:, absent] = True                 # listed, but prior <= 0: the pass must not train them (nor count them in nact)
    r64 = o.forward(o._bcast(p, NB), tgt, coords, lists, cfg, None if cfg.ssim_opt else lw, np.float64)
    # batches with a gate value on the influence threshold or a blend on the clip edge: discontinuous gradient there
    tau, window = sp.influence_threshold(cfg)
    tie = (np.abs(r64["w"] - tau) < window).any(axis=(1, 2))
    edge = ((np.abs(r64["y"]) < 1e-6) | (np.abs(r64["y"] - 1) < 1e-6)).any(axis=(1, 2))
    if halo is not None:                    # ... or, for the new list, a gate value of the halo on the threshold
        h64 = o.forward(o._bcast(p, NB), np.zeros(halo.shape[:2] + (C,)), halo.astype(np.float64), lists, cfg, None, np.float64)
        tie |= (np.abs(h64["w"] - tau) < window).any(axis=(1, 2))
    for d in (p, st["m"], st["v"]):
        for a in d.values():
            a.setflags(write=False)
    lists.setflags(write=False)
    return SharedState(case=case, opts={**opts, **own}, cfg=cfg, K=K, NB=NB, coords=coords, halo=halo, tgt=tgt, lw=lw, grid=grid,
                       p=p, m=st["m"], v=st["v"], b1p=np.float32(st["b1p"]), b2p=np.float32(st["b2p"]), step=WARMUP, lists=lists,
                       clean=~(tie | edge), coast=coast, absent=absent)


def build_shared_state(case, late=False, seed=5, **opts):
    """The state of ``case`` (an id of CASES or its tuple) after WARMUP fp32 iterations of the restatement with pruned lists;
    ``late``: the same parameters and slots with the beta powers (fp32 running products) of step LATE.  Cached: the legs of
    one shape share the warm-up."""
    case = CASES[case] if isinstance(case, str) else case
    s = _build(case, seed, sp._freeze(opts))
    if late:
        b1, b2 = np.float32(s.cfg.beta1), np.float32(s.cfg.beta2)
        b1p, b2p = b1, b2
        for _ in range(LATE):
            b1p, b2p = np.float32(b1p * b1), np.float32(b2p * b2)
        s = dataclasses.replace(s, b1p=b1p, b2p=b2p, step=LATE)
    return s


def condition(s):
    """The precondition of a meaningful comparison, on the restatement alone: (clean batches, batches, kernels -- the
    coasting one aside -- that no clean batch lists).  The callers assert 2 * clean >= batches and no such kernel."""
    listed = s.lists[s.clean].any(axis=0)
    listed[s.coast] = True
    return int(s.clean.sum()), s.NB, [int(k) for k in np.flatnonzero(~listed)]


def shared_config(s, **override):
    shape, bshape, C, kpd, yuv = s.case
    kw = {k: v for k, v in s.opts.items() if k not in ("weights", "diff_center")}
    return SharedConfig(image_shape=shape, batch_shape=bshape, channels=C, kernels=s.K, use_yuv=yuv, **{**kw, **override})


def _dev(a, eng):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _sync(eng):
    if eng.device.type == "cuda":
        torch.cuda.synchronize()


def load_state(eng, s):
    """(target, params, AdamState, lists) of the engine at state ``s``; the loss weights and the centre grid are set."""
    dp = {k: _dev(v[0].astype(np.float32), eng) for k, v in s.p.items()}
    st = eng.new_adam_state(dp)
    for k in o.PARAM_NAMES:
        st.m[k].copy_(_dev(s.m[k][0].astype(np.float32), eng))
        st.v[k].copy_(_dev(s.v[k][0].astype(np.float32), eng))
    st.c.beta1_power, st.c.beta2_power, st.c.step = float(s.b1p), float(s.b2p), int(s.step)
    if hasattr(st, "_step"):
        st._step = int(s.step)
    lists = _dev(_bits(s.lists).view(np.int32), eng)
    T = _dev(np.transpose(s.tgt, (0, 2, 1)), eng)
    if s.lw is not None:
        eng.set_loss_weights(_dev(s.lw, eng))            # (both setters keep a reference to what they are given)
    if s.grid is not None:
        eng.set_center_grid(_dev(s.grid, eng))
    return T, dp, st, lists


def _host(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


def _ref_pass(s, dtype, q):
    """The restatement's per-batch pass at the state on the lattice ``q``.  With quantization_mode 2 / 3 the fp64 pass runs on
    the fp32-quantised parameters and routes the gradients back through the fp32 quantiser's masks (step_parity._ref_pass);
    the mode-3 ranges are image-wide -- the same in every batch -- and the routing is linear, so the sum of the routed
    per-batch gradients is the routed sum."""
    cfg = s.cfg
    lw = None if cfg.ssim_opt else s.lw
    pb = o._bcast(s.p, s.NB)
    if dtype == np.float64 and cfg.quantization_mode >= 2:
        q32, back, _ = o.quantize_graph_params(pb, cfg, np.float32)
        cfg0 = o.OracleConfig(**{**cfg.__dict__, "quantization_mode": 0, "quantize_pis": False})
        ref = o.forward(q32, s.tgt, s.coords, s.lists, cfg0, lw, np.float64, want_grads=True, q_override=q)
        ref["grads"] = o.route_quant_grads(ref["grads"], back, np.float64)
        return ref
    return o.forward(pb, s.tgt, s.coords, s.lists, cfg, lw, dtype, want_grads=True, q_override=q)


def _runs(mask):
    """[lo, hi) of every contiguous run of set entries."""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


@dataclasses.dataclass
class Result:
    ratios: dict             # comparison -> worst error / tolerance (<= 1 passes)
    failures: list
    clean: int
    batches: int
    runs: int                # accumulate calls the clean batches took

    def require(self):
        assert not self.failures, (self.failures, self.ratios)
        return self


def check_shared_step(eng, s):
    """Load ``s`` into ``eng``, take ONE step on the clean batches and compare with the restatement (module docstring).
    Returns a ``Result``; nothing is asserted here."""
    cfg, NB, K = s.cfg, s.NB, s.K
    fails, ratios = [], {}

    def judge(name, err, tol):
        r = float(np.max(err / tol)) if np.size(err) else 0.0          # (every tolerance is > 0; a NaN fails)
        ratios[name] = max(ratios.get(name, 0.0), r)
        if not r <= 1.0:
            fails.append((name, r))

    def count(name, n):
        ratios[name] = max(ratios.get(name, 0.0), float(n))
        if n:
            fails.append((name, int(n)))

    T, dp, st, lists = load_state(eng, s)
    c = s.clean

    # ---- the engine's own lattice --------------------------------------------------------------------------------
    fw = eng.forward(T, dp, lists.clone(), update_lists=False, want_recon=True)
    q = np.transpose(fw["recon"].cpu().numpy(), (0, 2, 1))
    ref = _ref_pass(s, np.float32, q)
    ref64 = _ref_pass(s, np.float64, q)
    sp.lattice_check(judge, q, ref["y"], ref64["y"], cfg)               # against the fp32 restatement's own lattice

    # ---- stale rows: a full pass, dropped ------------------------------------------------------------------------
    eng.accumulate(T, dp, lists.clone())
    eng.discard_gradients()

    # ---- the clean batches, one call per contiguous run; then the step -------------------------------------------
    work = lists.clone()
    loss = torch.zeros(NB, device=eng.device)
    sse = torch.zeros(NB, device=eng.device)
    runs = _runs(c)
    for lo, hi in runs:
        eng.accumulate(T[lo:hi].contiguous(), dp, work[lo:hi], first_batch=lo, loss_out=loss[lo:hi], sse_out=sse[lo:hi])
    eng.apply(dp, st)
    _sync(eng)

    lo_, ss_ = loss.cpu().numpy(), sse.cpu().numpy()
    judge("loss", np.abs(lo_ - ref64["loss"])[c], (1e-6 + 2e-5 * np.abs(ref64["loss"]))[c])
    judge("sse", np.abs(ss_ - ref64["sse"])[c], (1e-6 + 2e-5 * np.abs(ref64["sse"]))[c])
    want = ref["active_new"]
    if s.halo is not None:
        want = o.forward(o._bcast(s.p, NB), np.zeros(s.halo.shape[:2] + (s.tgt.shape[2],), np.float32), s.halo, s.lists, cfg,
                         None, np.float32)["active_new"]
    new = _mask(work.cpu().numpy().view(np.uint32), K)
    count("list", (new[c] != want[c]).sum())
    count("list_unvisited", (new[~c] != s.lists[~c]).sum())

    # ---- bookkeeping ---------------------------------------------------------------------------------------------
    count("step", int(st.step != s.step + 1))
    for name, got_p, p0, b in (("b1p", st.c.beta1_power, s.b1p, cfg.beta1), ("b2p", st.c.beta2_power, s.b2p, cfg.beta2)):
        adv = float(np.float32(p0) * np.float32(b))
        judge(name, np.abs(np.array([float(got_p) - adv])), 2.0 ** -22 * adv)

    # ---- gradients, slots, parameters ----------------------------------------------------------------------------
    ast = {"m": {k: v.copy() for k, v in s.m.items()}, "v": {k: v.copy() for k, v in s.v.items()}, "t": s.step,
           "b1p": s.b1p, "b2p": s.b2p}
    # The fp32 restatement's adam_step, fed with the fp64 sum of the clean batches' gradients rounded to fp32 once (the kernels
    # too sum the rows in fp64 and round the total once).  Not the fp32 pass's own gradients: the v' and parameter tolerances
    # allow the ENGINE's gradient an error of dg and the reference's none, and the fp32 numpy restatement of the SSIM graph is
    # itself up to 1.2 dg off the fp64 one (the margin-loss graphs: 0.03 dg), which the comparison would charge to the engine.
    g32 = {k: v[c].sum(axis=0, keepdims=True).astype(np.float32) for k, v in ref64["grads"].items()}
    p_ref = o.adam_step({k: v.copy() for k, v in s.p.items()}, g32, ast, cfg, np.float32)
    m1, v1, got = _host(st.m), _host(st.v), _host(dp)
    b1, b2 = np.float32(cfg.beta1), np.float32(cfg.beta2)
    bias = np.sqrt(1.0 - float(s.b2p)) / (1.0 - float(s.b1p))
    k_ = s.coast
    for name in o.PARAM_NAMES:
        lr = sp._lr(cfg, name)
        if not trained(cfg, name):
            count("moved:" + name, int(not (np.array_equal(got[name], s.p[name][0]) and np.array_equal(m1[name], s.m[name][0])
                                            and np.array_equal(v1[name], s.v[name][0]))))
            continue
        gb = ref64["grads"][name][c]
        g64 = gb.sum(axis=0)
        dg = 2e-5 * (float(np.abs(gb).sum(axis=0).max()) if gb.size else 0.0) + 1e-30
        sp.judge_adam(judge, name, cfg, lr, bias, g64, dg, s.m[name][0], m1[name], ast["m"][name][0], ast["v"][name][0], v1[name],
                      p_ref[name][0], got[name])
        # the coasting kernel: dense Adam with g = 0 exactly
        m0, v0, x0 = s.m[name][0][k_], s.v[name][0][k_], s.p[name][0][k_]
        count("coast:g64:" + name, int(np.any(g64[k_] != 0)))
        sp.judge_adam(lambda n, e, t: judge("coast_" + n, e, t), name, cfg, lr, bias, np.zeros_like(g64[k_]), 1e-30, m0, m1[name][k_],
                      ast["m"][name][0][k_], ast["v"][name][0][k_], v1[name][k_], p_ref[name][0][k_], got[name][k_])
        judge("coast_m:" + name, np.abs(m1[name][k_].astype(np.float64) - (m0 + (np.float32(0) - m0) * (np.float32(1) - b1))),
              4 * 2.0 ** -24 * np.abs(m0) + 1e-37)
        judge("coast_v2:" + name, np.abs(v1[name][k_].astype(np.float64) - (v0 + (np.float32(0) - v0) * (np.float32(1) - b2))),
              4 * 2.0 ** -24 * np.abs(v0) + 1e-37)
        ulp = 2.0 ** -23 * np.maximum(np.abs(x0), 2.0 ** -126)
        should = (m0 != 0) & (np.abs(p_ref[name][0][k_].astype(np.float64) - x0) > 4 * ulp)
        count("coast_still:" + name, (should & (got[name][k_] == x0)).sum())
        if name in COAST_TENSORS:
            count("coast_idle:" + name, int(not should.any()))          # (the scenario itself: something has to move)
    return Result(ratios=ratios, failures=fails, clean=int(c.sum()), batches=NB, runs=len(runs))


def _snapshot(eng, dp, st, lists, loss, sse):
    _sync(eng)
    out = {"lists": lists.cpu().numpy().copy(), "loss": loss.cpu().numpy().copy(), "sse": sse.cpu().numpy().copy(),
           "b1p": np.float32(st.c.beta1_power), "b2p": np.float32(st.c.beta2_power), "step": np.int64(st.step)}
    for k in o.PARAM_NAMES:
        out["p:" + k], out["m:" + k], out["v:" + k] = dp[k].cpu().numpy().copy(), st.m[k].cpu().numpy().copy(), st.v[k].cpu().numpy().copy()
    return out


def check_paths(eng_factory, s, iters=(1, 3)):
    """smoe_shared_fit against accumulate(all) + apply from the same loaded state, ``n`` iterations each: the names of
    everything that is not bit-identical, per ``n`` (empty: the two step paths agree)."""
    bad = {}
    for n in iters:
        outs = []
        for fused in (True, False):
            eng = eng_factory()
            try:
                T, dp, st, lists = load_state(eng, s)
                loss, sse = torch.zeros(s.NB, device=eng.device), torch.zeros(s.NB, device=eng.device)
                if fused:
                    eng.fit(T, dp, st, lists, n, loss_out=loss, sse_out=sse)
                else:
                    for _ in range(n):
                        eng.accumulate(T, dp, lists, loss_out=loss, sse_out=sse)
                        eng.apply(dp, st)
                outs.append(_snapshot(eng, dp, st, lists, loss, sse))
            finally:
                eng.close()
        a, b = outs
        diff = [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]
        if not (a["step"] == s.step + n and np.isfinite(a["loss"]).all()):
            diff.append("step/finite")
        if not any(np.any(a["p:" + k] != s.p[k][0]) for k in o.PARAM_NAMES):
            diff.append("nothing moved")
        if diff:
            bad[n] = diff
    return bad


worst = sp.worst

__all__ = ["CASES", "OPTION_LEGS", "build_shared_state", "check_shared_step", "check_paths", "condition", "shared_config", "load_state",
           "worst", "WARMUP", "LATE"]
