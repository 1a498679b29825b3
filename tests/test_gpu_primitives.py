"""The field and group-law primitives as the GPU runs them: one operation per lane through the gfx950 build of tools/primcheck (compiled
by the package's build() with the library's own flags), compared with Python integers and the Python oracle's group law.  This is the
only place where the device forms -- the product-scanning 8x32 product over fe_mac96, the pinned 29-bit multiply-add chains, the DPP
exchanges of the four-lane group law, the wave helpers of rt.hpp -- meet an integer.  A failure names the primitive and prints the first
operand tuples in hex.  Cases and checks: tests/prim_cases.py (the same run under the emulator in tests/test_primitives_emu.py)."""
import pytest

import prim_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(mp):      # (mp: the package is imported first, so that torch's HIP runtime is in the process before the probe's)
    p = pc.Probe(pc.GPU_LIB)      # a missing probe library is an error, not a skip
    assert p.rt_name == "hip-gfx950", p.rt_name
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
