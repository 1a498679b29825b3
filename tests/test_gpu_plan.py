"""-m gpu: the cases of tests/plan_cases.py on the GPU -- the smallest shapes at which the static plans take each branch of
PhaseBuilder::end (sub-job cap, combine tree at 11 / 12 / 13 / 16 / 17 pieces, window lanes with and without the pre-combine, the bucket
threshold, late combines), keyed plans, Toom-Cook on and off and Karatsuba, one case on each of the other curves: three generic proofs
per case byte for byte against the C++ oracle, honest and mutated batches under merged and per-equation verification word for word, with
one and four lanes per group operation where the case says so, and mp_plan_stats against the stand-alone checker's counts of the same
plan.  tests/test_plan_emu.py runs all but the two sub-job cap cases through the emulator; tests/test_plan_check.py keeps the list honest."""
import pytest

import plan_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return pc.build_checker()


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_plan_branch_matches_the_oracle(mp, coracle, checker, case):
    eng = mp._native.Engine(case.curve, 0)
    try:
        fails, checks = pc.run_case(eng, coracle, checker, case)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks == pc.checks_expected(case)
