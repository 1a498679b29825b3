"""The scalar recodings and the tables and kernels behind them as the GPU runs them: the cases of tests/digit_cases.py through the gfx950
build of tools/digitcheck (compiled by the package's build() with the library's own flags) against the Python-integer models, exact
equality, and the cases of tests/fixed_base_cases.py through the C ABI against the C++ oracle -- every entry class of the 8-, 16-, 20- and
21-bit fixed-base tables, the key tables, and the recoders inside the Straus and bucket kernels on scalars that sit on a recoding boundary
in every window.  The same cases run under the emulator in tests/test_digit_emu.py (the wide tables excepted)."""
import pytest

import digit_cases as dc
import fixed_base_cases as fbc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(mp):      # (mp: the package is imported first, so that torch's HIP runtime is in the process before the probe's)
    p = dc.Probe(dc.GPU_LIB)      # a missing probe library is an error, not a skip
    assert p.rt_name == "hip-gfx950", p.rt_name
    return p


def _report(result):
    fails, count = result
    assert count > 0
    assert not fails, "\n" + "\n".join(fails[:9])


@pytest.mark.parametrize("bits", dc.FB_BITS)
@pytest.mark.parametrize("curve", dc.CURVES)
def test_fixed_base_digits_match_the_model(probe, curve, bits):
    _report(dc.run_digits(probe, curve, dc.KIND_FIXED, bits))


@pytest.mark.parametrize("curve", dc.CURVES)
def test_straus_digits_match_the_model(probe, curve):
    _report(dc.run_digits(probe, curve, dc.KIND_STRAUS, dc.STRAUS_BITS))


@pytest.mark.parametrize("c", dc.BUCKET_BITS)
@pytest.mark.parametrize("curve", dc.CURVES)
def test_bucket_digits_match_the_model(probe, curve, c):
    _report(dc.run_digits(probe, curve, dc.KIND_BUCKET, c))


def test_last_bucket_of_the_top_window_secp256k1_c8(probe):
    _report(dc.run_last_bucket(probe))


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


@pytest.mark.parametrize("curve,bits", [(c, b) for c in dc.CURVES for b in fbc.GPU_FB_BITS[c]])
def test_fixed_base_entries_match_oracle(engines, coracle, curve, bits):
    ft = fbc.FixedTable(engines(curve), coracle, curve, bits)      # (one table per (curve, width), all its cases on it)
    try:
        _report(fbc.run_fixed_entries(ft))
    finally:
        ft.close()


@pytest.mark.parametrize("path", fbc.MSM_PATHS, ids=fbc.path_id)
@pytest.mark.parametrize("curve", dc.CURVES)
def test_msm_recoders_match_oracle(engines, coracle, curve, path):
    _report(fbc.run_msm_families(engines(curve), coracle, curve, path))


@pytest.mark.parametrize("curve", dc.CURVES)
def test_keyed_and_keyset_remasking_match_oracle(engines, coracle, curve):
    import torch
    _report(fbc.run_keyed(engines(curve), coracle, curve, torch, torch.device("cuda", 0)))
