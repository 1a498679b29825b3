"""CPU tests (-m "not gpu") of degenerate parameter sets (tests/param_edge_cases.py): the two oracles agree on every set, and the engine --
kernel bodies under the development emulator (tools/hostemu) -- builds its tables from them, proves the oracle's bytes under every plan
and gives the oracle's verdicts.  The same cases run on the gfx950 build in tests/test_gpu_param_edge.py."""
import ctypes
import os
import subprocess

import pytest

import param_edge_cases as pe
from conftest import ROOT


def _report(result):
    fails, count = result
    assert count > 0
    assert not fails, "\n" + "\n".join(fails[:9])


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.mark.parametrize("name", pe.SETS)
@pytest.mark.parametrize("m,n", pe.SHAPES)
@pytest.mark.parametrize("curve", pe.CURVES)
def test_oracles_agree_on_degenerate_parameters(coracle, curve, m, n, name):
    _report(pe.run_oracles_agree(coracle, curve, m, n, name))


@pytest.mark.parametrize("name", pe.SETS)
@pytest.mark.parametrize("m,n", pe.SHAPES)
@pytest.mark.parametrize("curve", pe.CURVES)
def test_degenerate_parameters_under_emulation(emu, coracle, curve, m, n, name):
    eng = emu(curve)
    try:
        _report(pe.run_engine(eng, coracle, curve, m, n, name))
    finally:
        eng.close()


@pytest.mark.parametrize("which", pe.INF_BASES)
@pytest.mark.parametrize("curve", pe.CURVES)
def test_a_base_at_infinity_is_refused_under_emulation(emu, coracle, curve, which):
    eng = emu(curve)
    try:
        _report(pe.run_infinite_base(eng, coracle, curve, 2, 2, which))
    finally:
        eng.close()
