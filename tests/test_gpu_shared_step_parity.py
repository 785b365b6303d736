"""GPU matrix of the teacher-forced step of the shared-kernel whole-image fit (tests/shared_step_parity.py).

(a) ONE Adam step of smoe_shared_accumulate (the clean batches only, after a discarded full pass) + smoe_shared_apply from a
    t = 7 state with sparse lists, element by element against the restatement, on the smallest shapes that reach what no other
    shared test does: more than 64 and more than 256 batches (the gather's second row per lane, its second trip, the clamped
    tail), more than 256 kernels (the second compaction round, an odd number of list words, lists longer than one LDS chunk),
    batches that a pass does not revisit (stale rows), nact < number of batches under the l1 terms, a kernel that coasts.
(b) smoe_shared_fit against accumulate + apply from the same state, bit for bit, for 1 and 3 iterations.
SMOE_SHARED_ONE_LAUNCH stays unset: the cooperative one-launch fit is pinned to the two-launch loop elsewhere.
"""
import pytest

import shared_step_parity as ssp

pytestmark = pytest.mark.gpu

# Seeds at which the restatement alone meets the precondition (tests/test_shared_step_parity_cpu.py): nine 16x16 batches of
# 272 kernels leave little room, one unclean batch takes the only listing of dozens of kernels with it.
SEEDS = {("C", None): 9, ("C3", None): 15, ("C", "q3"): 18}

# (case id, late, option leg or None)
STEP_CASES = [(c, False, None) for c in ("A", "B", "C", "C3", "D")] + [("A", True, None), ("C", True, None)]
STEP_CASES += [("A", False, "l1clip"), ("A", False, "l1")]
STEP_CASES += [("B", False, leg) for leg in ("qpis", "q2", "q3", "ic", "radial", "dcq2", "lw", "ov3")]
STEP_CASES += [("S", False, "ssim"), ("C", False, "q3")]
# the switches off their defaults; the determinant and the precision on the 3-d code as well
NEW_LEGS = ("nodet", "nodet_ic", "fz_pis", "fz_mus", "fz_gam", "p10", "p6", "margin", "startpis")
STEP_CASES += [("B", False, leg) for leg in NEW_LEGS] + [("D", False, "nodet"), ("D", False, "p10")]
# (smoe_shared_fit fills its kernel arguments -- use_det, reg_pi, the precision's constants -- apart from accumulate / apply)
PATH_CASES = [("A", None), ("B", None), ("C", None), ("D", None), ("B", "q3"), ("S", "ssim"), ("B", "p10"), ("B", "nodet")]


def state_of(cid, late, leg):
    return ssp.build_shared_state(cid, late=late, seed=SEEDS.get((cid, leg), 5), **(ssp.OPTION_LEGS[leg] if leg else {}))


def _id(c):
    cid, late, leg = c
    return f"{cid}-{'late' if late else 't7'}" + (f"-{leg}" if leg else "")


def _engine(s):
    from steered_mixture_of_experts_amd.engine import SharedEngine
    return SharedEngine(ssp.shared_config(s))


WORST = {}


@pytest.mark.parametrize("case", STEP_CASES, ids=[_id(c) for c in STEP_CASES])
def test_teacher_forced_shared_step(case, monkeypatch):
    monkeypatch.delenv("SMOE_SHARED_ONE_LAUNCH", raising=False)
    s = state_of(*case)
    clean, batches, unlisted = ssp.condition(s)
    assert 2 * clean >= batches and not unlisted, (clean, batches, unlisted)
    eng = _engine(s)
    try:
        assert eng.num_batches == s.NB
        res = ssp.check_shared_step(eng, s)
    finally:
        eng.close()
    print(_id(case), f"clean {res.clean}/{res.batches} in {res.runs} calls", {k: f"{v:.3g}" for k, v in ssp.worst(res.ratios).items() if v},
          *(["FAILS", [(n, float(f"{r:.3g}")) for n, r in res.failures[:4]]] if res.failures else []))
    for k, v in ssp.worst(res.ratios).items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    res.require()


@pytest.mark.parametrize("cid,leg", PATH_CASES, ids=[c + (f"-{leg}" if leg else "") for c, leg in PATH_CASES])
def test_fit_equals_accumulate_and_apply_bit_for_bit(cid, leg, monkeypatch):
    monkeypatch.delenv("SMOE_SHARED_ONE_LAUNCH", raising=False)
    s = state_of(cid, False, leg)
    bad = ssp.check_paths(lambda: _engine(s), s)
    assert not bad, bad


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module's tests: the worst error / tolerance ratio per comparison over the step cases that ran (shown with -s)."""
    yield
    if WORST:
        print("\nteacher-forced shared step, worst ratios:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})
