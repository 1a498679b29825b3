"""The field and group-law primitives of the engine's headers, one operation per lane, against Python integers -- through the probe of
tools/primcheck built for the development emulator (kernel bodies as CPU loops).  Needs no GPU: it proves the cases, the reference and
the probe's plumbing, and checks the HOST forms of the arithmetic for all eight fields and four curves.  The same cases run on the
gfx950 build in tests/test_gpu_primitives.py; cases and checks: tests/prim_cases.py."""
import pytest

import prim_cases as pc


@pytest.fixture(scope="module")
def probe():
    p = pc.Probe(pc.build_emu_probe())
    assert "emulator" in p.rt_name
    return p


def _report(result):
    fails, count = result
    assert count > 0
    assert not fails, "\n" + "\n".join(fails[:9])


@pytest.mark.parametrize("family", list(pc.FIELD_FAMILIES))
@pytest.mark.parametrize("field", pc.FIELDS)
def test_field_operations_match_integers(probe, field, family):
    _report(pc.run_field(probe, field, family))


@pytest.mark.parametrize("op", list(pc.GROUP_OPS))
@pytest.mark.parametrize("curve", pc.CURVES)
def test_group_law_matches_oracle(probe, curve, op):
    _report(pc.run_group(probe, curve, op))


@pytest.mark.parametrize("launch", ["divergent", "uniform"])
@pytest.mark.parametrize("op", list(pc.QUAD_OPS))
@pytest.mark.parametrize("curve", pc.CURVES)
def test_four_lane_group_law_matches_oracle(probe, curve, op, launch):
    _report(pc.run_quad(probe, curve, op, launch))


def test_wave_helpers_match_numpy(probe):
    _report(pc.run_wave_helpers(probe))


def test_block_helpers_match_numpy(probe):
    _report(pc.run_block_helpers(probe))
