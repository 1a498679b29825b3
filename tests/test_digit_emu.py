"""CPU tests (-m "not gpu") of the scalar recodings and of the tables and kernels behind them, with the kernel bodies under the development
emulator (tools/hostemu): the probe tools/digitcheck/digit_check.hip built by g++ over the engine's headers, every case of
tests/digit_cases.py against the Python-integer models (exact equality), and the cases of tests/fixed_base_cases.py through the C ABI of
the emulator build against the C++ oracle.  The same cases run on the gfx950 build in tests/test_gpu_digit.py; the emulator leaves the
16-, 20- and 21-bit tables and the bucket windows of 11 bits and more to it (fixed_base_cases.EMU_*)."""
import ctypes
import os
import subprocess

import pytest

import digit_cases as dc
import fixed_base_cases as fbc
from conftest import ROOT


@pytest.fixture(scope="module")
def probe():
    p = dc.Probe(dc.build_emu_probe())
    assert p.rt_name.startswith("host-emulator"), p.rt_name
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


def test_window_counts_and_top_digits_of_the_four_orders():
    _report(fbc.check_order_table())


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.mark.parametrize("bits", fbc.EMU_FB_BITS)
@pytest.mark.parametrize("curve", dc.CURVES)
def test_fixed_base_entries_match_oracle(emu, coracle, curve, bits):
    eng = emu(curve)
    try:
        ft = fbc.FixedTable(eng, coracle, curve, bits)
        try:
            _report(fbc.run_fixed_entries(ft))
        finally:
            ft.close()
    finally:
        eng.close()


@pytest.mark.parametrize("path", fbc.EMU_MSM_PATHS, ids=fbc.path_id)
@pytest.mark.parametrize("curve", dc.CURVES)
def test_msm_recoders_match_oracle(emu, coracle, curve, path):
    eng = emu(curve)
    try:
        _report(fbc.run_msm_families(eng, coracle, curve, path))
    finally:
        eng.close()


@pytest.mark.parametrize("curve", dc.CURVES)
def test_keyed_and_keyset_remasking_match_oracle(emu, coracle, curve):
    import torch
    eng = emu(curve)
    try:
        _report(fbc.run_keyed(eng, coracle, curve, torch, "cpu"))
    finally:
        eng.close()
