"""CPU tests (-m "not gpu") of the one-wave bucket kernel k_bucket_msm at mode, rank, share and item edges (tests/bucket_wave_cases.py)
with the kernel body under the development emulator (tools/hostemu): every family on STARK (8 .. 11 bits), secp256k1 (8, 11), bn254 (9)
and BLS12-377 (8, 10) against libmpemu.so, whose 2 'CUs' give 16 persistent waves, so that every call of more than 16 (MSM, window)
items reuses scratch rows and LDS.  Families A, D, E and G run once more against a further emulator library built with
-DMP_EXP_BK_BALANCED (make BALANCED=1), the hook that sends every window down the balanced walk: share boundaries at arbitrary places
of arbitrary bucket layouts, the expected points unchanged -- shipped code under a predicate that is not shipped, no GPU counterpart.
The group screen and the chain verifier run with 9 equations in a launch: 8 partitions, the first with two equations.
tests/test_gpu_bucket_wave.py runs the same cases on gfx950.

The construction check needs no engine: every case against the digit model, with the edge each case reaches printed (pytest -s).

Wall time of this module, measured with tests/test_bucket_split_emu.py in one session on one machine (both emulator libraries
built beforehand, 8 CPUs): 88 s against 141 s."""
import ctypes
import os
import subprocess

import pytest

import bucket_wave_cases as bwc
from conftest import ROOT

SLOTS = bwc.slots_of(bwc.EMU_CUS)


def _emu(mp, balanced):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d] + (["BALANCED=1"] if balanced else []))
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu_balanced.so" if balanced else "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.fixture(scope="module")
def emu(mp):
    return _emu(mp, False)


@pytest.fixture(scope="module")
def emu_balanced(mp):
    return _emu(mp, True)


def _run(fn, *args, **kw):
    fails, checks = fn(*args, **kw)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0
    return checks


def test_rules_are_the_engines():
    assert bwc.rules_are_the_engines() == []
    g = bwc.WaveGeo(8)
    assert (g.NBK, g.NB, g.LOGNB, g.lane(1), g.cls(1), g.lane(128), g.cls(128), g.bucket(37, 1)) == (128, 2, 1, 0, 0, 63, 1, 76)
    g = bwc.WaveGeo(11)
    assert (g.NBK, g.NB, g.LOGNB, g.lane(16), g.cls(16), g.lane(17), g.cls(17)) == (1024, 16, 4, 0, 15, 1, 0)
    assert [g.threshold(T) for T in (0, 63, 64, 127, 128, 4193)] == [32, 32, 33, 33, 35, 129]
    assert bwc.partition_sizes(7) == [7] and bwc.partition_sizes(8) == [1] * 8
    assert bwc.partition_sizes(9) == [2] + [1] * 7 and bwc.partition_sizes(17) == [3] + [2] * 7
    assert SLOTS == 16


def test_model_decisions_on_small_items():
    """decide() on layouts small enough to work out by hand (8 bits: 128 buckets, two classes)"""
    import numpy as np
    r = bwc.decide(np.full(33, 5), 8)                      # bucket 5: lane 2, class 0, rank 0 -> worker 0
    assert (r["mode"], r["maxn"], r["thr"], r["workers"], r["nonempty"], r["shares"]) == ("balanced", 33, 32, {0}, {5}, {0, 1})
    r = bwc.decide(np.array([6] * 20 + [8] * 20 + [10] * 3), 8)      # class 1, lanes 2, 3 (a tie: the lower lane first) and 4 -> workers 63, 62, 61
    assert r["mode"] == "ranked" and [int(r["n"][l]) for l in (63, 62, 61)] == [20, 20, 3] and r["workers"] == {61, 62, 63}
    r = bwc.decide(np.array([1] * 64 + [128] * 64), 8)
    assert (r["cuts_on"], r["cuts_inside"], r["span"], r["lo"][31], r["lo"][32]) == (1, 0, 0, 1, 128)
    r = bwc.decide(np.array([1] * 65 + [128] * 64), 8)
    assert (r["cuts_on"], r["cuts_inside"], r["span"]) == (0, 1, 127)


@pytest.mark.parametrize("curve", list(bwc.WIDTHS))
def test_constructions_reach_their_edges(curve):
    fails, checks, lines = bwc.self_check(curves=(curve,))
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:40])
    assert checks == len(lines) > 0


@pytest.mark.parametrize("fam", bwc.FAMILIES)
@pytest.mark.parametrize("curve", list(bwc.WIDTHS))
def test_wave_kernel_edges(emu, coracle, curve, fam):
    eng = emu(curve)
    try:
        _run(bwc.run_family, eng, coracle, curve, fam, SLOTS)
    finally:
        eng.close()


@pytest.mark.parametrize("fam", bwc.BALANCED_FAMILIES)
@pytest.mark.parametrize("curve", list(bwc.WIDTHS))
def test_every_layout_under_the_balanced_walk(emu_balanced, coracle, curve, fam):
    eng = emu_balanced(curve)
    try:
        _run(bwc.run_family, eng, coracle, curve, fam, SLOTS)
    finally:
        eng.close()


@pytest.mark.parametrize("bits", [8, 10])
def test_group_screen_of_nine_equations(emu, coracle, bits):
    eng = emu("stark")
    try:
        _run(bwc.run_group_screen, eng, coracle, bits)
    finally:
        eng.close()


def test_chain_of_nine_tables(emu, coracle):
    eng = emu("stark")
    try:
        _run(bwc.run_chain_nine, eng, coracle)
    finally:
        eng.close()
