"""CPU test of the static plans of layout.hpp, without a GPU and without the Python extension: tests/cpp/plan_check.cpp evaluates every phase
of the prover's and the verifier's job tables over formal sums and asserts, over a grid of shapes and work splits, that no slot is written
twice or read before it is written, that every slot lies inside its arena, that every final slot holds the sums of the unsplit plan, that
the unsplit per-equation phase and the merged phase (expanded through mjobs / mpairs) hold exactly what describe_verify describes, and that
the Karatsuba diagonals are the schoolbook bilinear form of the multi-exponentiation argument for m = 3 .. 40.  Toom-Cook's interpolation
is not checked here: its constants live in the engine (engine_core.hpp toom_constants), not in layout.hpp; the Toom-Cook cases of
tests/plan_cases.py compare it with the oracle on the GPU (tests/test_gpu_plan.py) and under the emulator (tests/test_plan_emu.py)."""
import subprocess

import pytest

import plan_cases as pc

# the grid: a copy of the lists in plan_check.cpp, from which the expected number of configurations is computed -- a grid that shrinks fails
M_VALUES = range(2, 19)
SMALL_N, LARGE_N = (2, 3, 8, 9), (63, 64, 65, 128, 129)              # the large n at m = 2 only
NAMED = 7 + 6                                                         # engine_core.hpp default PlanParams (both tiny_v), shuffle_edge_cases.PLAN_PARAMS
CHUNKS, LANES, CHUNKS_LARGE, LANES_LARGE = 8 + 4, 5, 4, 3             # chunk sizes 1, 2, 3, 4 .. 64 and four mixed pairs; lanes 1, 2, 3, 5, 16
BUCKET = 3 * 3 + 2 * 2                                                # three splits x (largest MSM - 1, the same, + 1); two x thresholds 2, 64
KEYED_TOOM = 4
CONFIGURATIONS = (len(M_VALUES) * len(SMALL_N) * (NAMED + CHUNKS * LANES + BUCKET) + len(LARGE_N) * (NAMED + CHUNKS_LARGE * LANES_LARGE + BUCKET)) * KEYED_TOOM
KARATSUBA_PLANS = len(range(3, 41)) * 2


@pytest.fixture(scope="module")
def checker():
    return pc.build_checker()


def test_every_work_split_evaluates_the_unsplit_sums(checker):
    r = subprocess.run([checker], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout
    out = dict(line.split() for line in r.stdout.splitlines())
    assert int(out["configurations"]) == CONFIGURATIONS == 24152
    assert int(out["karatsuba_plans"]) == KARATSUBA_PLANS


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_case_takes_the_branch_it_is_listed_for(checker, case):
    fails = pc.branch_failures(checker, case)
    assert not fails, "\n".join(fails)


def test_the_case_list_covers_every_branch():
    """what the issue of the case list asks for is in it: both caps, the tree edges, window lanes 2 / 3 / 16, both sides of the bucket
    threshold on two splits, two keyed cases, Toom-Cook on and off at m = 3 and 16, Karatsuba at 17, every curve, group lanes 1 and 4 on
    at least four cases"""
    keys = {(ph, key, op) + tuple(v) for c in pc.CASES for ph, key, op, *v in c.branch}
    for want in [("prove.A", "cap_fixed", ">0"), (pc.MERGED, "cap_var", ">0"), (pc.PER_EQ, "cap_var", ">0"), (pc.MERGED, "flat", "has", "11"),
                 ("prove.B", "late", ">0"), ("prove.B", "wsplit_single", ">0"), (pc.MERGED, "wsplit_multi", ">0"), (pc.MERGED, "bucket", "none")]:
        assert want in keys, want
    for pieces in ("12/4", "13/4", "16/4", "17/5"):
        assert (pc.MERGED, "tree", "has", pieces) in keys
    assert {2, 3, 16} <= {c.params[4] for c in pc.CASES}
    assert {(c.split == 3, c.bucket_min) for c in pc.CASES if c.bucket_min} == {(True, 54), (True, 55), (False, 54), (False, 55)}
    assert sum(1 for c in pc.CASES if c.keyed) >= 2
    assert {(c.m, c.toom) for c in pc.CASES if c.split in pc.TOOM_SPLITS and c.m in (3, 16)} == {(3, True), (3, False), (16, True), (16, False)}
    assert any(c.m == 17 for c in pc.CASES)
    assert {c.curve for c in pc.CASES} == {"stark", "bn254", "secp256k1", "bls12_377"}
    assert sum(1 for c in pc.CASES if c.group_lanes == (1, 4)) >= 4
    assert max(c.m * c.n for c in pc.CASES) == 258
