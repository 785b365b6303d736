"""The decoder cases of tests/triple_cases.py without a GPU: the case list is the non-FULL part of csrc/smoe_variants.def, the
fit parity lists of tests/test_gpu_parity.py name every triple of the file, and the restatements alone -- float32 against
float64 -- keep every case inside the caps the GPU suites put on their inputs (tests/test_gpu_sample.py, test_gpu_sample_grad.py,
test_gpu_sample_area.py: the conditions are theirs, imported)."""
import numpy as np
import pytest

import test_gpu_parity
import test_gpu_sample
import test_gpu_sample_area
import test_gpu_sample_grad
import triple_cases as tc
from sample_area_cases import LOOSE_CAP

CASES = [(t, name) for t in tc.TRIPLES for name, _, _ in tc.CONFIGS]
CASE_IDS = [f"{i}-{name}" for i in tc.TRIPLE_IDS for name, _, _ in tc.CONFIGS]


def test_the_parser_reads_the_file_as_the_build_does(tmp_path):
    triples = tc.parse_triples()
    assert len(triples) == 28 and sum(t[3] for t in triples) == 5
    assert (2, 3, 8, 1) in triples and (3, 1, 1, 0) in triples
    f = tmp_path / "v.def"
    f.write_text("// SMOE_TRIPLE(9, 9, 9, 1) in a comment\nSMOE_TRIPLE(2, 1, 4, 1)   // trailing\n\nSMOE_TRIPLE(3,3,16,0)\n")
    assert tc.parse_triples(str(f)) == [(2, 1, 4, 1), (3, 3, 16, 0)]
    f.write_text("SMOE_TRIPLE(2, 1, 4)\n")
    with pytest.raises(AssertionError):
        tc.parse_triples(str(f))
    f.write_text("SMOE_TRIPLE(2, 1, 4, 1)\nSMOE_TRIPLE(2, 1, 4, 0)\n")
    with pytest.raises(AssertionError):
        tc.parse_triples(str(f))


def test_the_case_list_is_the_non_full_triples_of_the_build():
    triples = tc.parse_triples()
    assert sorted(tc.TRIPLES) == sorted(t[:3] for t in triples if not t[3])
    assert len(tc.TRIPLES) == 23
    for t in tc.TRIPLES:
        c = tc.case_inputs(t, "plain")
        assert c["K"] == t[2] and c["C"] == t[1] and len(c["shape"]) == t[0] and int(np.prod(c["grid"])) == 12
        assert tuple(c["shape"]) == tc.BLOCK_SHAPE[t[0]] and 5000 <= len(c["pts"]) <= 10000


def test_the_fit_parity_lists_name_every_triple_of_the_build():
    triples = tc.parse_triples()
    named = {tc.parity_shape(s) for s in test_gpu_parity.SHAPES + test_gpu_parity.EXTRA_SHAPES}
    assert named == {t[:3] for t in triples}
    # ... and the train_inverse_cov lists every triple that is not FULL but was without a deterministic case (FULL ones: SHAPES)
    import test_gpu_invcov
    ic = {tc.parity_shape(s) for s in test_gpu_invcov.IC_SHAPES}
    assert {t[:3] for t in triples if t[3]} <= ic and {tc.parity_shape(s) for s in test_gpu_parity.LATE_SHAPES} <= ic


@pytest.mark.parametrize("triple,config", CASES, ids=CASE_IDS)
def test_the_restatements_alone_keep_the_caps(triple, config):
    c = tc.case_inputs(triple, config)
    # K <= 3: every block keeps a live kernel; the configurations are the two of the issue
    if triple[2] <= 3:
        assert (c["active"] & (c["p"]["pis"] > 0)).any(axis=1).all()
    assert bool(c["cfg"].train_inverse_cov) == (config == "ic-blend") and (c["beta"] is not None) == (config == "ic-blend")
    # smoe_sample
    ref, ref64 = tc.sample_case_reference(triple, config)
    loose, outside = test_gpu_sample.rotated_conditions(ref, ref64, c["n_out"], len(c["pts"]))
    assert ((ref["recon"] != 0).any(axis=1) | outside).mean() > 0.9              # the model decodes to something
    # smoe_sample_grad
    g, g64 = tc.grad_case_reference(triple, config)
    gl, gout, eJ, eV = test_gpu_sample_grad.rotated_conditions(g, g64, c["n_out"], len(c["pts"]))
    assert np.array_equal(g64["block"], ref64["block"])
    # smoe_sample_area
    a, a64 = tc.area_case_reference(triple, config)
    covered, al, tight, e32 = test_gpu_sample_area.rotated_conditions(a, a64)
    assert np.array_equal(a["block"], a64["block"]) and e32 > 0
    share = al[covered].mean()
    noted = tc.TRIPLE_CASES[triple][1][config]
    print(f"loose shares: sample {loose.mean():.2e}, sample_grad {gl.mean():.2e}, sample_area {share:.2e} (noted {noted:.1e}); "
          f"e32: J {eJ:.1e}, values {eV:.1e}, mean {e32:.1e}")
    assert share <= LOOSE_CAP and abs(share - noted) < 5e-4                       # the figure next to the case is the measured one
    assert (a64["count"] > 0).sum() > 2000 and ((a64["count"] > 0) & (a64["count"] < a64["inside"].shape[1])).any()
