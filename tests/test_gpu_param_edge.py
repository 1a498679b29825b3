"""Degenerate parameter sets (tests/param_edge_cases.py) on the gfx950 build: tables from commitment keys that coincide or cancel -- a whole
fixed-base table built from the point at infinity --, the prover's bytes under every plan, the verifier's verdicts under both strategies.
The same cases run under the emulator in tests/test_param_edge_emu.py, where the two oracles are also held to each other."""
import pytest

import param_edge_cases as pe

pytestmark = pytest.mark.gpu


def _report(result):
    fails, count = result
    assert count > 0
    assert not fails, "\n" + "\n".join(fails[:9])


@pytest.fixture(scope="module")
def engines(mp):
    cache = {}

    def get(curve):
        if curve not in cache:
            cache[curve] = mp._native.Engine(curve, 0)
        return cache[curve]
    yield get
    for eng in cache.values():
        eng.close()


@pytest.mark.parametrize("name", pe.SETS)
@pytest.mark.parametrize("m,n", pe.SHAPES)
@pytest.mark.parametrize("curve", pe.CURVES)
def test_degenerate_parameters(engines, coracle, curve, m, n, name):
    _report(pe.run_engine(engines(curve), coracle, curve, m, n, name))


@pytest.mark.parametrize("which", pe.INF_BASES)
@pytest.mark.parametrize("curve", pe.CURVES)
def test_a_base_at_infinity_is_refused(engines, coracle, curve, which):
    _report(pe.run_infinite_base(engines(curve), coracle, curve, 2, 2, which))
