"""The shared-mode step checker (tests/shared_step_parity.py) on the CPU: it accepts the restatement behind the ``SharedEngine``
interface (tests/fake_engine.OracleSharedEngine) with a wide margin and rejects every mutant of it -- thin subclasses that get
the sum over the batches' rows, the lists or the Adam step wrong the ways the kernels could.  Also checks, for every state the
GPU matrix (tests/test_gpu_shared_step_parity.py) uses, the precondition of a meaningful comparison on the restatement alone."""
import numpy as np
import pytest

import shared_step_parity as ssp
import step_parity as sp
import test_gpu_shared_step_parity as g
from fake_engine import OracleSharedEngine
from oracle import smoe_oracle as o


def _engine(s, cls=OracleSharedEngine, *args):
    return cls(ssp.shared_config(s), *args)


def _slices(eng):
    out, off = {}, 0
    for k, shp in eng._shapes().items():
        n = int(np.prod(shp))
        out[k] = (off, off + n, shp)
        off += n
    return out


# ------------------------------------------------------------------------------------------------------------------
# mutants
# ------------------------------------------------------------------------------------------------------------------
class RegTimesNB(OracleSharedEngine):
    """the l1 terms counted once per batch of the image instead of once per batch that trains the kernel (nact)."""

    def apply(self, params, state):
        buf = self.grad_buffer().numpy()
        extra = self.num_batches - self._trained[self._seen].sum(axis=0).astype(np.float64)          # (K,)
        sl = _slices(self)
        buf[sl["pis"][0]:sl["pis"][1]] += extra * self.ocfg.pis_l1 / self.ocfg.k0
        a = buf[sl["A_diagonal"][0]:sl["A_diagonal"][1]].reshape(sl["A_diagonal"][2])
        a += (extra * self.ocfg.u_l1)[:, None, None] * np.eye(a.shape[-1])
        return super().apply(params, state)


class StaleRowsAdded(OracleSharedEngine):
    """the rows of the batches this step did not visit join the sum (no epoch filter)."""

    def apply(self, params, state):
        assert (~self._seen).any()
        self.grad_buffer().numpy()[:] += self._part[~self._seen].astype(np.float64).sum(axis=0)
        return super().apply(params, state)


class LastBatchTwice(OracleSharedEngine):
    """the last batch counted twice (the clamped tail of the gather not masked)."""

    def apply(self, params, state):
        assert self._seen[-1]
        self.grad_buffer().numpy()[:] += self._part[-1].astype(np.float64)
        return super().apply(params, state)


class SecondGroupBatchDropped(OracleSharedEngine):
    """one batch of the second group of 64 is left out of the sum."""

    def apply(self, params, state):
        b = 64 + int(np.flatnonzero(self._seen[64:128])[0])
        self.grad_buffer().numpy()[:] -= self._part[b].astype(np.float64)
        return super().apply(params, state)


class ClearedBitSet(OracleSharedEngine):
    """one cleared bit of one batch's kernel list is treated as set."""

    def __init__(self, cfg, batch, kernel):
        super().__init__(cfg)
        self.batch, self.kernel = batch, kernel

    def accumulate(self, target, params, lists, first_batch=0, **kw):
        r = self.batch - first_batch
        if 0 <= r < lists.shape[0]:
            w = lists.numpy().view(np.uint32)
            assert not (w[r, self.kernel >> 5] >> np.uint32(self.kernel & 31)) & 1
            w[r, self.kernel >> 5] |= np.uint32(1 << (self.kernel & 31))
        return super().accumulate(target, params, lists, first_batch, **kw)


class B2pAhead(OracleSharedEngine):
    """beta2's running power one step ahead."""

    def apply(self, params, state):
        state.c.beta2_power = float(np.float32(state.c.beta2_power) * np.float32(self.cfg.beta2))
        return super().apply(params, state)


class VWithBeta1(OracleSharedEngine):
    """v' = v + (g^2 - v)(1 - beta1)."""

    def apply(self, params, state):
        self.ocfg.beta2 = self.ocfg.beta1
        return super().apply(params, state)


class CoastingKernelLeft(OracleSharedEngine):
    """a kernel that no batch trained keeps its variables and slots (a sparse step where TF's ApplyAdam is dense)."""

    def apply(self, params, state):
        idle = self._trained[self._seen].sum(axis=0) == 0
        keep = [(d[k], d[k][idle].clone()) for d in (params, state.m, state.v) for k in d]
        super().apply(params, state)
        for t, old in keep:
            t[idle] = old


class KernelsPast255Skipped(OracleSharedEngine):
    """the list compaction stops after its first round of 256 kernels."""

    def accumulate(self, target, params, lists, first_batch=0, **kw):
        mask = self._mask(lists)
        mask[:, 256:] = False
        self._setbits(lists, mask)
        return super().accumulate(target, params, lists, first_batch, **kw)


# ---- one mutant per switch of the new option legs: the engine ignores what it was configured with ------------------
class DeterminantKept(OracleSharedEngine):
    """use_determinant=False ignored."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert not self.ocfg.use_determinant
        self.ocfg.use_determinant = True


class FrozenTensorTrained(OracleSharedEngine):
    """train_pis / train_musx = False ignored in the step: the tensor's rate is not zeroed."""

    def apply(self, params, state):
        assert not (self.ocfg.train_pis and self.ocfg.train_musx)
        keep = self.ocfg
        self.ocfg = o.OracleConfig(**{**keep.__dict__, "train_pis": True, "train_musx": True})
        try:
            return super().apply(params, state)
        finally:
            self.ocfg = keep


class FrozenSlotsAdvance(FrozenTensorTrained):
    """the frozen tensor stays where it is, but its slots take the step."""

    def apply(self, params, state):
        keep = {k: params[k].clone() for k in ("pis", "musX")}
        super().apply(params, state)
        for k, on in (("pis", self.ocfg.train_pis), ("musX", self.ocfg.train_musx)):
            if not on:
                params[k].copy_(keep[k])


class GammasKept(OracleSharedEngine):
    """train_gammas=False ignored: the slopes stay in the forward graph and are trained."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert not self.ocfg.train_gammas
        self.ocfg.train_gammas = True


class Levels255(OracleSharedEngine):
    """the pixel lattice has 255 levels whatever the precision; threshold and margin follow it.  Only the lattice comparison
    can see it: everything else belongs to the lattice the checker feeds to the restatements."""

    def _on_255(self, call, *a, **kw):
        assert self.ocfg.precision != 8
        real = o.fake_quant01
        o.fake_quant01 = lambda y, precision, T: real(y, 8, T)
        try:
            return call(*a, **kw)
        finally:
            o.fake_quant01 = real

    def forward(self, *a, **kw):
        return self._on_255(super().forward, *a, **kw)

    def accumulate(self, *a, **kw):
        return self._on_255(super().accumulate, *a, **kw)


class KernelsForStartPis(OracleSharedEngine):
    """the l1 term of the priors normalised by the kernel count, start_pis ignored."""

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device)
        assert self.ocfg.start_pis not in (None, cfg.kernels) and self.ocfg.pis_l1 > 0
        self.ocfg.start_pis = cfg.kernels


# ------------------------------------------------------------------------------------------------------------------
ACCEPT = [("B", False, None), ("C", False, None), ("B", True, "q3"), ("A", False, "l1clip"), ("A", False, "l1")]
ACCEPT += [("B", False, leg) for leg in g.NEW_LEGS] + [("D", False, "nodet"), ("D", False, "p10")]


@pytest.mark.parametrize("case", ACCEPT, ids=[g._id(c) for c in ACCEPT])
def test_checker_accepts_the_restatement_with_margin(case):
    """The fp32 restatement against the fp64 one stays below a quarter of every tolerance.  The one exception is by
    construction: the coasting kernel's recovered gradient is judged against the recovery term alone, 10 * 2^-24 max(|m|, |m'|)
    = 1.1 * 2^-24 |m'|, and the fp32 rounding of m' = 0.9 m alone is up to 2^-24 |m'|."""
    s = g.state_of(*case)
    res = ssp.check_shared_step(_engine(s), s).require()
    print(g._id(case), f"clean {res.clean}/{res.batches} in {res.runs} calls", {k: f"{v:.3g}" for k, v in ssp.worst(res.ratios).items() if v})
    assert res.runs >= 2 or res.clean == res.batches
    for k, r in res.ratios.items():
        assert r <= (1.0 if k.startswith("coast_grad:") else 0.25), (k, r)


def test_checker_accepts_the_two_step_paths_of_the_restatement():
    s = g.state_of("B", False, None)
    assert not ssp.check_paths(lambda: _engine(s), s)

    class FitDropsABatch(OracleSharedEngine):
        def fit(self, target, params, state, lists, n_iters, loss_out=None, sse_out=None):
            for _ in range(n_iters):
                self.accumulate(target, params, lists, 0, loss_out, sse_out)
                self.grad_buffer().numpy()[:] -= self._part[70].astype(np.float64)
                self.apply(params, state)
    bad = ssp.check_paths(lambda: _engine(s, FitDropsABatch), s)
    assert set(bad) == {1, 3} and "lists" not in bad[1] and any(k.startswith("m:") for k in bad[1]), bad


def test_every_gpu_matrix_state_meets_the_precondition():
    """At least half of the batches clean, and no kernel (the coasting one aside) without a clean batch that lists it: a
    condition on the restatement alone, asserted again by the GPU test."""
    seen = set()
    for cid, late, leg in g.STEP_CASES + [(c, False, leg) for c, leg in g.PATH_CASES]:
        if (cid, leg) in seen:
            continue
        seen.add((cid, leg))
        s = g.state_of(cid, False, leg)
        clean, batches, unlisted = ssp.condition(s)
        trained = s.lists & (s.p["pis"][0] > 0)[None, :]
        print(cid, leg, f"clean {clean}/{batches}, kernels per batch {trained.sum(1).min()}..{trained.sum(1).max()}, "
              f"batches per kernel up to {trained.sum(0).max()}, coasting kernel {s.coast}")
        assert 2 * clean >= batches and not unlisted, (cid, leg, clean, batches, unlisted)
        assert s.lists[:, list(s.absent)].all() and not trained[:, list(s.absent)].any() and not s.lists[:, s.coast].any()
        assert np.any(s.m["nu_e"][0, s.coast] != 0)
        assert trained.sum(0).max() < batches                      # nact < NB: the l1 terms can tell them apart
        assert len(ssp._runs(s.clean)) >= 2 or clean == batches    # (several accumulate calls, unless nothing is excluded)
    assert len(seen) == 17 + len(g.NEW_LEGS) + 2
    # the shapes reach what they are there for
    a, b, c = (g.state_of(x, False, None) for x in "ABC")
    assert a.NB == 289 and a.clean[256:].any() and a.clean[-1] and b.NB == 90 and b.clean[64:].any()
    kc = (c.lists & (c.p["pis"][0] > 0)[None, :]).sum(axis=1)
    assert c.K == 272 and (c.K + 31) // 32 == 9 and c.lists[:, 256:].any() and kc.min() < 64 < kc.max()


MUTANTS = [
    # mutant, case id, late, leg
    (RegTimesNB, "A", False, "l1clip"), (RegTimesNB, "A", False, "l1"),
    (StaleRowsAdded, "A", False, None), (StaleRowsAdded, "B", False, None),
    (LastBatchTwice, "A", False, None),
    (SecondGroupBatchDropped, "A", False, None), (SecondGroupBatchDropped, "B", False, None),
    (B2pAhead, "B", False, None), (B2pAhead, "B", True, "q3"),
    (VWithBeta1, "B", False, None),
    (CoastingKernelLeft, "B", False, None), (CoastingKernelLeft, "A", False, "l1clip"),
    (KernelsPast255Skipped, "C", False, None),
]


@pytest.mark.parametrize("mutant,cid,late,leg", MUTANTS, ids=[f"{m.__name__}-{g._id((c, l, leg))}" for m, c, l, leg in MUTANTS])
def test_checker_rejects_the_mutant(mutant, cid, late, leg):
    s = g.state_of(cid, late, leg)
    res = ssp.check_shared_step(_engine(s, mutant), s)
    print(mutant.__name__, cid, res.failures[:4])
    assert res.failures, res.ratios
    kinds = {n.split(":")[0] for n, _ in res.failures}
    if mutant in (B2pAhead, VWithBeta1):
        # the Adam mutants leave loss, lists and gradients alone: only the teacher-forced slots, parameters and powers see them
        assert kinds <= {"param", "v", "b2p", "coast_param", "coast_v", "coast_v2"}, res.failures
    if mutant is CoastingKernelLeft:
        # (it leaves every kernel that no batch trained, the two with a prior <= 0 included: the comparisons of the whole tensor
        # see those as well)
        assert {"coast_grad", "coast_m", "coast_v2", "coast_param", "coast_still"} <= kinds, res.failures


SWITCH_MUTANTS = [
    # mutant, case id, leg, the comparisons that may (and at least one of which must) see it
    (DeterminantKept, "B", "nodet", None), (DeterminantKept, "D", "nodet", None), (DeterminantKept, "B", "nodet_ic", None),
    (FrozenTensorTrained, "B", "fz_pis", {"moved"}), (FrozenTensorTrained, "B", "fz_mus", {"moved"}),
    (FrozenSlotsAdvance, "B", "fz_pis", {"moved"}), (FrozenSlotsAdvance, "B", "fz_mus", {"moved"}),
    (GammasKept, "B", "fz_gam", None),
    (Levels255, "B", "p10", {"lattice", "lattice_tie"}), (Levels255, "D", "p10", {"lattice", "lattice_tie"}),
    (Levels255, "B", "p6", {"lattice", "lattice_tie"}),
    (KernelsForStartPis, "B", "startpis", {"loss", "grad", "v", "param"}),
]


@pytest.mark.parametrize("mutant,cid,leg,seen_by", SWITCH_MUTANTS, ids=[f"{m.__name__}-{c}-{leg}" for m, c, leg, _ in SWITCH_MUTANTS])
def test_checker_rejects_an_engine_that_ignores_the_switch(mutant, cid, leg, seen_by):
    s = g.state_of(cid, False, leg)
    res = ssp.check_shared_step(_engine(s, mutant), s)
    print(mutant.__name__, cid, leg, res.failures[:6])
    assert res.failures, res.ratios
    if seen_by is not None:
        assert {n.split(":")[0] for n, _ in res.failures} <= seen_by, res.failures


def test_precision_8_masks_are_the_ones_of_the_fixed_threshold():
    """The influence threshold and its band follow cfg.precision (step_parity.influence_threshold); at 8 bits the clean masks
    of the GPU matrix's states are those of the constants they were built with before, 0.5 / 256 and 1e-6, bit for bit."""
    n = 0
    for cid, leg in [("A", None), ("B", None), ("C", None), ("D", None), ("A", "l1clip"), ("B", "ov3"), ("B", "lw"), ("B", "nodet")]:
        s = g.state_of(cid, False, leg)
        assert s.cfg.precision == 8 and sp.influence_threshold(s.cfg) == (0.5 / 256, 1e-6)
        r64 = o.forward(o._bcast(s.p, s.NB), s.tgt, s.coords, s.lists, s.cfg, s.lw, np.float64)
        tie = (np.abs(r64["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
        edge = ((np.abs(r64["y"]) < 1e-6) | (np.abs(r64["y"] - 1) < 1e-6)).any(axis=(1, 2))
        if s.halo is not None:
            h64 = o.forward(o._bcast(s.p, s.NB), np.zeros(s.halo.shape[:2] + (s.tgt.shape[2],)), s.halo.astype(np.float64), s.lists,
                            s.cfg, None, np.float64)
            tie |= (np.abs(h64["w"] - 0.5 / 256) < 1e-6).any(axis=(1, 2))
        assert np.array_equal(s.clean, ~(tie | edge)), (cid, leg)
        n += 1
    assert n == 8


def test_coasting_kernel_is_picked_among_the_trained_tensors():
    """With train_musx=False the musX slots stay zero: the picker looks at the tensors the configuration trains."""
    s = g.state_of("B", False, "fz_mus")
    assert not s.m["musX"].any() and not s.v["musX"].any()
    assert np.any(s.m["nu_e"][0, s.coast] != 0) and np.any(s.m["A_diagonal"][0, s.coast] != 0)
    assert ssp.trained(s.cfg, "nu_e") and not ssp.trained(s.cfg, "musX")


def test_checker_rejects_a_cleared_list_bit_treated_as_set():
    """The coasting kernel's bit, in the clean batch nearest to its centre."""
    s = g.state_of("B", False, None)
    centre = s.coords.mean(axis=1)                                               # (NB,d)
    dist = np.where(s.clean, np.linalg.norm(centre - s.p["musX"][0, s.coast][None, :], axis=1), np.inf)
    res = ssp.check_shared_step(_engine(s, ClearedBitSet, int(np.argmin(dist)), s.coast), s)
    assert res.failures, res.ratios
