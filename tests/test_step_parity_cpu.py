"""The teacher-forced step checker (tests/step_parity.py) on the CPU: it accepts the restatement behind the ``BlockEngine``
interface (tests/fake_engine.OracleEngine: the plain-C oracle, the numpy one for the graphs the C one lacks), with a wide
margin, and rejects every mutant of it -- thin subclasses that alter what they hand the oracle.  Also checks, for every state
the GPU matrix (tests/test_gpu_step_parity.py) uses, that the restatement alone keeps at least half of the blocks clean."""
import numpy as np
import pytest
import torch

import step_parity as sp
from fake_engine import OracleEngine
from oracle import smoe_oracle as o
from steered_mixture_of_experts_amd.engine import EngineConfig

CPU_SHAPES = [sp.SHAPES[0], sp.SHAPES[2], sp.SHAPES[6]]        # (16,16)/1/[2,2], (32,32)/3/[2,4], (12,10,3)/3/[2,2,1]


def _ids(cases):
    return ["x".join(map(str, s[0])) + f"-c{s[1]}-k" + "x".join(map(str, s[2])) for s in cases]


def _engine(case, cls=OracleEngine, **opts):
    shape, C, kpd, yuv = case
    return cls(EngineConfig(block_shape=shape, channels=C, kernels=int(np.prod(kpd)), **sp.engine_kwargs(case, **opts)))


# ------------------------------------------------------------------------------------------------------------------
# mutants: each alters what the engine hands the oracle in fit()
# ------------------------------------------------------------------------------------------------------------------
class B2pAhead(OracleEngine):
    """beta2's running power one step ahead (a launch that advanced it before its first iteration)."""

    def fit(self, target, params, state, active, n_iters, **kw):
        state.c.beta2_power = float(np.float32(state.c.beta2_power) * np.float32(self.cfg.beta2))
        return super().fit(target, params, state, active, n_iters, **kw)


class VWithBeta1(OracleEngine):
    """v' = v + (g^2 - v)(1 - beta1)."""

    def fit(self, target, params, state, active, n_iters, **kw):
        self.ocfg.beta2 = self.ocfg.beta1
        return super().fit(target, params, state, active, n_iters, **kw)


class _WeightMutant(OracleEngine):
    def mutate(self, w):
        raise NotImplementedError

    def fit(self, target, params, state, active, n_iters, loss_w=None, **kw):
        w = torch.ones((target.shape[0], target.shape[2])) if loss_w is None else loss_w.clone()
        return super().fit(target, params, state, active, n_iters, loss_w=self.mutate(w).contiguous(), **kw)


class LastPixelIgnored(_WeightMutant):
    """the last pixel of every block does not count (a ragged tail guarded one pixel short)."""

    def mutate(self, w):
        w[:, -1] = 0.0
        return w


class OnePixelOffOnePercent(_WeightMutant):
    def mutate(self, w):
        w[:, w.shape[1] // 3] *= 1.01
        return w


class WeightsSquared(_WeightMutant):
    def mutate(self, w):
        return w * w


class ClearedBitSet(OracleEngine):
    """one cleared bit of one block's kernel list is treated as set."""

    def __init__(self, cfg, block, kernel):
        super().__init__(cfg)
        self.block, self.kernel = block, kernel

    def fit(self, target, params, state, active, n_iters, **kw):
        a = active.numpy().view(np.uint32)
        assert not (a[self.block] >> self.kernel) & 1
        a[self.block] |= np.uint32(1 << self.kernel)
        return super().fit(target, params, state, active, n_iters, **kw)


class SampleFlagIgnored(OracleEngine):
    """the weight-0 pixels of a sub-sample vote in the prune like loss-mask pixels."""

    def fit(self, target, params, state, active, n_iters, loss_w_is_sample=False, **kw):
        return super().fit(target, params, state, active, n_iters, loss_w_is_sample=False, **kw)


class NumpyOracleEngine(OracleEngine):
    """Every pass through the numpy restatement in fp32 (the plain OracleEngine takes the C one where it can): THE fp32
    reference of the margin check."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        self.numpy_only = True


# ---- one mutant per switch of the option legs: the engine ignores what it was configured with ----------------------
class DeterminantKept(OracleEngine):
    """use_determinant=False ignored: the normaliser keeps prod diag(A), the steering gradient its su / A_ll term."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert not self.ocfg.use_determinant
        self.ocfg.use_determinant = True


class FrozenTensorTrained(OracleEngine):
    """train_pis / train_musx = False ignored in the owner phase: the tensor's rate is not zeroed.  (Not for train_gammas:
    with the slopes out of the forward graph their gradient is 0, and Adam leaves a variable with zero gradient and zero slots
    where it is whatever its rate -- GammasKept.)"""

    def fit(self, target, params, state, active, n_iters, **kw):
        assert not (self.ocfg.train_pis and self.ocfg.train_musx and self.ocfg.train_gammas)
        real = o.adam_step
        o.adam_step = lambda p, g, st, cfg, *a, **k: real(p, g, st, o.OracleConfig(**{**cfg.__dict__, "train_pis": True,
                                                                                      "train_musx": True, "train_gammas": True}), *a, **k)
        self.numpy_only = True
        try:
            return super().fit(target, params, state, active, n_iters, **kw)
        finally:
            o.adam_step = real


class GammasKept(OracleEngine):
    """train_gammas=False ignored: the slopes stay in the forward graph and are trained."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert not self.ocfg.train_gammas
        self.ocfg.train_gammas = True


class FrozenSlotsAdvance(FrozenTensorTrained):
    """the frozen tensor stays where it is, but its slots take the step (the update masked on the variable alone)."""

    def fit(self, target, params, state, active, n_iters, **kw):
        keep = {k: v.clone() for k, v in params.items()}
        super().fit(target, params, state, active, n_iters, **kw)
        for k, on in (("pis", self.ocfg.train_pis), ("musX", self.ocfg.train_musx)):
            if not on:
                params[k].copy_(keep[k])


class Levels255(OracleEngine):
    """the pixel lattice has 255 levels whatever the precision; threshold and margin follow it.  Loss, list, gradients and
    the step all belong to that lattice, which the checker feeds to the restatements: only the lattice comparison can see it."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert self.ocfg.precision != 8
        self.numpy_only = True

    def _on_255(self, call, *a, **kw):
        real = o.fake_quant01
        o.fake_quant01 = lambda y, precision, T: real(y, 8, T)
        try:
            return call(*a, **kw)
        finally:
            o.fake_quant01 = real

    def forward(self, *a, **kw):
        return self._on_255(super().forward, *a, **kw)

    def fit(self, *a, **kw):
        return self._on_255(super().fit, *a, **kw)


class KernelsForStartPis(OracleEngine):
    """the l1 term of the priors normalised by the kernel count, start_pis ignored."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert self.ocfg.start_pis not in (None, cfg.kernels) and self.ocfg.pis_l1 > 0
        self.ocfg.start_pis = cfg.kernels


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("late", [False, True], ids=["t7", "late"])
@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("case", CPU_SHAPES, ids=_ids(CPU_SHAPES))
def test_checker_accepts_the_restatement_with_margin(case, kind, late):
    """The fp32 restatement against the fp64 one stays below a quarter of EVERY tolerance."""
    s = sp.build_state(case, kind, late=late)
    eng = _engine(case, cls=NumpyOracleEngine)
    res = sp.check_step(eng, s, eng0=_engine(case, cls=NumpyOracleEngine, lr_expert=0.0, lr_pis=0.0, lr_steer=0.0)).require()
    print(case[0], kind, "late" if late else "t7", f"clean {res.clean}/{res.blocks}", sp.worst(res.ratios))
    assert res.variant == "oracle"
    assert 2 * res.clean >= res.blocks
    for k, r in res.ratios.items():
        assert r <= 0.25, (k, r)
    if kind == "sample":
        assert s.flag_matters                          # the list of the corner block really depends on the sample flag


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("case", CPU_SHAPES, ids=_ids(CPU_SHAPES))
def test_checker_accepts_the_c_restatement(case, kind):
    """The double the mutants are built on (plain C where it can) is itself accepted: the derived tolerances with the same factor
    of four to spare; loss / SSE within the tolerance -- the C code sums a block's squared errors sequentially in fp32 (half of
    the 2e-5 over the 3 072 values of a 32x32 RGB block), which is that double's summation order and nothing a kernel shares.
    "lattice_tie" has no margin to keep: it reads 0 or 1 -- a pixel on a rounding tie of the quantiser, where the C code's blend
    and numpy's differ in the last bit, lands one level apart (the 32x32 states have such a pixel) or it does not; off the
    ties ("lattice") the two are equal."""
    s = sp.build_state(case, kind)
    res = sp.check_step(_engine(case), s).require()
    assert res.ratios["lattice"] == 0.0
    assert max(r for k, r in res.ratios.items() if k not in ("loss", "sse", "lattice_tie")) <= 0.25, res.ratios


@pytest.mark.parametrize("lr_steer", [1e-2])
@pytest.mark.parametrize("case", CPU_SHAPES, ids=_ids(CPU_SHAPES))
def test_checker_accepts_the_restatement_with_a_gentle_steering_step(case, lr_steer):
    s = sp.build_state(case, "frac", lr_steer=lr_steer)
    res = sp.check_step(_engine(case, cls=NumpyOracleEngine, lr_steer=lr_steer), s).require()
    assert max(res.ratios.values()) <= 0.25, res.ratios


SWITCH_LEGS = ("nodet", "nodet_ic", "fz_pis", "fz_mus", "fz_gam", "p10", "p6", "margin", "startpis")


def _accepts_leg(leg, case):
    opts = sp.OPTION_LEGS[leg]
    s = sp.build_state(case, "pad", **opts)
    res = sp.check_step(_engine(case, cls=NumpyOracleEngine, **opts), s).require()
    print(leg, case[0], f"clean {res.clean}/{res.blocks}", sp.worst(res.ratios))
    assert 2 * res.clean >= res.blocks
    assert max(res.ratios.values()) <= 0.25, res.ratios


@pytest.mark.parametrize("leg", list(sp.OPTION_LEGS))
def test_checker_accepts_the_option_legs(leg):
    _accepts_leg(leg, sp.SHAPES[1])


@pytest.mark.parametrize("case", [sp.SHAPES[2], sp.SHAPES[3]], ids=_ids([sp.SHAPES[2], sp.SHAPES[3]]))
@pytest.mark.parametrize("leg", SWITCH_LEGS)
def test_checker_accepts_the_switch_legs_on_the_other_shapes_of_the_gpu_matrix(leg, case):
    _accepts_leg(leg, case)


@pytest.mark.parametrize("leg", ["p10", "nodet"])
def test_checker_accepts_the_unweighted_late_legs(leg):
    case, opts = sp.SHAPES[1], sp.OPTION_LEGS[leg]
    s = sp.build_state(case, "none", late=True, **opts)
    res = sp.check_step(_engine(case, cls=NumpyOracleEngine, **opts), s,
                        eng0=_engine(case, cls=NumpyOracleEngine, **{**opts, "lr_expert": 0.0, "lr_pis": 0.0, "lr_steer": 0.0})).require()
    assert max(res.ratios.values()) <= 0.25, res.ratios


def test_switch_legs_leave_the_defaults():
    assert set(SWITCH_LEGS) <= set(sp.OPTION_LEGS)
    base = o.OracleConfig(block_shape=(16, 16), channels=3, kernels=4)
    for leg in SWITCH_LEGS:
        assert any(getattr(base, k) != v for k, v in sp.OPTION_LEGS[leg].items()), leg
        assert "lr_steer" not in sp.OPTION_LEGS[leg]                     # at its default: no leg needed a gentler steering step
    import shared_step_parity as ssp
    kernel_counts = {int(np.prod(c[2])) for c in sp.SHAPES} | {int(np.prod(c[3])) for c in ssp.CASES.values()}
    assert sp.OPTION_LEGS["startpis"]["start_pis"] not in kernel_counts and ssp.OPTION_LEGS["startpis"]["start_pis"] not in kernel_counts


def test_precision_8_masks_are_the_ones_of_the_fixed_threshold():
    """The influence threshold and its band now follow cfg.precision.  At 8 bits they are the constants every state was built
    with before, 0.5 / 256 and 1e-6, bit for bit -- and so are the clean masks of the GPU matrix's states, recomputed here with
    the old expression.  Off 8 bits the band keeps its share of the threshold."""
    base = o.OracleConfig(block_shape=(16, 16), channels=3, kernels=4)
    assert sp.influence_threshold(base) == (0.5 / 256, 1e-6)
    for prec in (6, 10, 12):
        tau, window = sp.influence_threshold(o.OracleConfig(block_shape=(16, 16), channels=3, kernels=4, precision=prec))
        assert tau == 0.5 / 2 ** prec and window / tau == 1e-6 / (0.5 / 256)
    n = 0
    for case, kind, leg in _gpu_matrix_states():
        s = sp.build_state(case, kind, **(sp.OPTION_LEGS[leg] if leg else {}))
        if s.cfg.precision != 8:
            continue
        r64 = o.forward(s.p, s.tgt, s.coords, s.active, s.cfg, None if s.cfg.ssim_opt else s.lw, np.float64, fed=s.fed)
        tie = (np.abs(r64["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
        edge = ((np.abs(r64["y"]) < 1e-6) | (np.abs(r64["y"] - 1) < 1e-6)).any(axis=(1, 2))
        assert np.array_equal(s.clean, ~(tie | edge)), (case, kind, leg)
        n += 1
    assert n >= 7 * 4 + 5 * 3


def _gpu_matrix_states():
    import test_gpu_step_parity as g
    seen = set()
    for case, _tiling, kind, late, leg in g.STEP_CASES:
        key = (case[0], case[1], tuple(case[2]), kind, leg)
        if key not in seen:
            seen.add(key)
            yield case, kind, leg


def test_every_gpu_matrix_state_keeps_half_of_its_blocks_clean():
    """The clean-block cap of the GPU matrix, on the restatement alone (the clean mask depends on the state only)."""
    low = (1.0, None)
    n = 0
    for case, kind, leg in _gpu_matrix_states():
        s = sp.build_state(case, kind, **(sp.OPTION_LEGS[leg] if leg else {}))
        share = s.clean.mean()
        assert 2 * s.clean.sum() >= s.clean.size, (case, kind, leg, int(s.clean.sum()), s.clean.size)
        if kind == "sample":
            assert s.flag_matters, (case, leg)
        low = min(low, (share, (case[0], kind, leg)))
        n += 1
    print(f"{n} states, lowest clean share {low}")
    assert n >= 7 * 4


MUTANTS = [
    # mutant, weight kind, late
    (B2pAhead, "frac", False), (B2pAhead, "pad", True),
    (VWithBeta1, "frac", False), (VWithBeta1, "none", True),
    (LastPixelIgnored, "none", True), (LastPixelIgnored, "frac", False),
    (OnePixelOffOnePercent, "none", True), (OnePixelOffOnePercent, "frac", False),
    (WeightsSquared, "frac", False),
    (SampleFlagIgnored, "sample", False),
]


@pytest.mark.parametrize("mutant,kind,late", MUTANTS, ids=[f"{m.__name__}-{k}-{'late' if l else 't7'}" for m, k, l in MUTANTS])
@pytest.mark.parametrize("case", CPU_SHAPES[:2], ids=_ids(CPU_SHAPES[:2]))
def test_checker_rejects_the_mutant(case, mutant, kind, late):
    s = sp.build_state(case, kind, late=late)
    res = sp.check_step(_engine(case, cls=mutant), s)
    print(mutant.__name__, case[0], kind, res.failures[:4])
    assert res.failures, res.ratios
    if mutant in (B2pAhead, VWithBeta1):
        # the Adam mutants leave loss, list and gradients alone: only the teacher-forced slots and parameters see them
        assert all(n.split(":")[0] in ("param", "v") for n, _ in res.failures), res.failures


SWITCH_MUTANTS = [
    # mutant, leg, weight kind, late, the comparisons that may (and at least one of which must) see it
    (DeterminantKept, "nodet", "pad", False, None), (DeterminantKept, "nodet", "none", True, None),
    (DeterminantKept, "nodet_ic", "pad", False, None),
    (FrozenTensorTrained, "fz_pis", "pad", False, {"moved"}), (FrozenTensorTrained, "fz_mus", "pad", False, {"moved"}),
    (GammasKept, "fz_gam", "pad", False, None),
    (FrozenSlotsAdvance, "fz_pis", "pad", False, {"moved"}), (FrozenSlotsAdvance, "fz_mus", "pad", False, {"moved"}),
    (Levels255, "p10", "pad", False, {"lattice", "lattice_tie"}), (Levels255, "p10", "none", True, {"lattice", "lattice_tie"}),
    (Levels255, "p6", "pad", False, {"lattice", "lattice_tie"}),
    (KernelsForStartPis, "startpis", "pad", False, {"loss", "grad", "v", "param"}),
]


@pytest.mark.parametrize("mutant,leg,kind,late,seen_by", SWITCH_MUTANTS,
                         ids=[f"{m.__name__}-{leg}-{k}-{'late' if l else 't7'}" for m, leg, k, l, _ in SWITCH_MUTANTS])
def test_checker_rejects_an_engine_that_ignores_the_switch(mutant, leg, kind, late, seen_by):
    """A leg is worth its GPU time only if the checker sees its switch ignored.  The state is the leg's own: the restatement
    obeys the switch, the mutant does not."""
    case, opts = sp.SHAPES[1], sp.OPTION_LEGS[leg]
    s = sp.build_state(case, kind, late=late, **opts)
    res = sp.check_step(_engine(case, cls=mutant, **opts), s)
    print(mutant.__name__, leg, kind, res.failures[:6])
    assert res.failures, res.ratios
    kinds = {str(n).split(":")[0] for n, _ in res.failures}
    if seen_by is not None:
        assert kinds <= seen_by, res.failures
    if mutant is FrozenSlotsAdvance:
        frozen = {"fz_pis": "pis", "fz_mus": "musX"}[leg]
        assert res.failures == [("moved:" + frozen, "m/v")], res.failures          # the variable itself has not moved


@pytest.mark.parametrize("case", CPU_SHAPES, ids=_ids(CPU_SHAPES))
def test_checker_rejects_a_cleared_list_bit_treated_as_set(case):
    s = sp.build_state(case, "pad")
    cand = np.argwhere(~s.active & (s.p["pis"] > 0) & s.clean[:, None])
    assert len(cand)
    block, kernel = (int(x) for x in cand[0])
    shape, C, kpd, yuv = case
    eng = ClearedBitSet(EngineConfig(block_shape=shape, channels=C, kernels=s.K, use_yuv=yuv), block, kernel)
    res = sp.check_step(eng, s)
    assert res.failures, res.ratios


def test_sample_scenario_is_what_it_claims():
    """Built like test_sub_sampled_pass_prunes_by_the_fed_pixels_only: with the flag the corner block drops kernel 0, without
    it keeps it -- on the restatement, at the state the step under test starts from."""
    for case in CPU_SHAPES:
        s = sp.build_state(case, "sample")
        a_s = o.forward(s.p, s.tgt, s.coords, s.active, s.cfg, s.lw, np.float32, fed=s.fed)["active_new"]
        a_m = o.forward(s.p, s.tgt, s.coords, s.active, s.cfg, s.lw, np.float32)["active_new"]
        assert s.active[s.corner, 0] and a_m[s.corner, 0] and not a_s[s.corner, 0]
        assert s.clean[s.corner], "the corner block must be among the compared ones"
