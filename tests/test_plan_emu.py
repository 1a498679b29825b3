"""CPU test (-m "not gpu") of the plan cases of tests/plan_cases.py with the kernel bodies under the development emulator (tools/hostemu):
every case of at most 12 cards -- the combine-tree edges, the window-lane cases, the bucket threshold, Toom-Cook on and off at m = 3, the
keyed cases and the three other curves, all at (2, 3), (3, 2) or (4, 3) -- and, since each takes the emulator only a few seconds, also
tree-and-late (2, 11), toom-16 and toom-off-16 (16, 2) and karatsuba-17 (17, 2).  GPU-only: the two sub-job cap cases, cap-fixed (2, 129)
and cap-var (2, 65), which take the emulator the longest; tests/test_gpu_plan.py runs every case."""
import ctypes
import os
import subprocess

import pytest

import plan_cases as pc
from conftest import ROOT

EMU_CASES = [c for c in pc.CASES if c.m * c.n <= pc.EMU_MAX_N]


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.fixture(scope="module")
def checker():
    return pc.build_checker()


def test_the_gpu_only_cases_are_the_documented_ones():
    assert sorted(c.name for c in pc.CASES if c not in EMU_CASES) == ["cap-fixed", "cap-var"]
    assert all(c in EMU_CASES for c in pc.CASES if c.m * c.n <= 12)


@pytest.mark.parametrize("case", EMU_CASES, ids=lambda c: c.name)
def test_plan_branch_matches_the_oracle(emu, coracle, checker, case):
    eng = emu(case.curve)
    try:
        fails, checks = pc.run_case(eng, coracle, checker, case)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks == pc.checks_expected(case)
