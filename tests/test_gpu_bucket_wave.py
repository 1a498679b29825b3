"""-m gpu: the one-wave bucket kernel k_bucket_msm at mode, rank, share and item edges on the GPU -- the cases of
tests/bucket_wave_cases.py, which tests/test_bucket_wave_emu.py runs through the emulator: lengths around nq = 64, an item exactly at the
mode switch and its twin one term past it, balanced shares of 0, 1 and 2 terms that start on a bucket boundary or cross every empty
bucket, rank ties, empty leading classes, all the work on workers 0 and 63, exceptional points inside a bucket, 1 to 17 MSMs in a call
under both folds, more (MSM, window) items than persistent waves (8 per CU of this device), both modes in one launch, a small call after a
large one, windows whose results are at infinity -- through mp_msm, the result point byte for byte against the oracle's, every call
checked to have run on k_bucket_msm alone.  STARK: windows of 8 .. 11 bits; secp256k1 (256-bit order): 8 and 11; bn254: 9; BLS12-377
(14 limbs): 8 and 10.  The group screen and the chain verifier run with 9 equations in a launch."""
import pytest

import bucket_wave_cases as bwc

pytestmark = pytest.mark.gpu

CASES = [(curve, fam) for curve in bwc.WIDTHS for fam in bwc.FAMILIES]


def _slots():
    import torch
    return bwc.slots_of(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("curve,fam", CASES, ids=["%s-%s" % cf for cf in CASES])
def test_wave_kernel_edges(mp, coracle, curve, fam):
    eng = mp._native.Engine(curve, 0)
    try:
        fails, checks = bwc.run_family(eng, coracle, curve, fam, _slots())
    finally:
        eng.close()
    print("%s family %s: %d checks" % (curve, fam, checks))
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


@pytest.mark.parametrize("bits", [8, 10])
def test_group_screen_of_nine_equations(mp, coracle, bits):
    eng = mp._native.Engine("stark", 0)
    try:
        fails, checks = bwc.run_group_screen(eng, coracle, bits)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


def test_chain_of_nine_tables(mp, coracle):
    eng = mp._native.Engine("stark", 0)
    try:
        fails, checks = bwc.run_chain_nine(eng, coracle)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks > 0
