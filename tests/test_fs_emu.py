"""CPU tests (-m "not gpu") of the device Fiat-Shamir layer with the kernel bodies under the development emulator (tools/hostemu): the probe
tools/fscheck/fs_check.hip built by g++ over the engine's headers, every case of tests/fs_cases.py against hashlib and the Python oracle
(exact equality), and the element-by-element tampering of a shuffle proof under both transcript kernels.  The same cases run on the
gfx950 build in tests/test_gpu_fs.py."""
import ctypes
import os
import subprocess

import pytest

import fs_cases as fc
from conftest import ROOT


@pytest.fixture(scope="module")
def probe():
    p = fc.Probe(fc.build_emu_probe())
    assert p.rt_name.startswith("host-emulator"), p.rt_name
    return p


def _report(result):
    fails, count = result
    assert count > 0
    assert not fails, "\n" + "\n".join(fails[:9])


def test_array_chacha_is_the_oracles():
    _report(fc.check_chacha_reference())


@pytest.mark.parametrize("mode", [0, 1], ids=["one-lane", "four-lane"])
def test_staged_blake2s_matches_hashlib(probe, mode):
    _report(fc.run_blake2s(probe, mode))


@pytest.mark.parametrize("lpp", fc.LPPS)
@pytest.mark.parametrize("curve", fc.CURVES)
def test_fsq_absorb_matches_hashlib(probe, curve, lpp):
    _report(fc.run_fsq_absorb(probe, curve, lpp))


def test_chacha20_block_matches_oracle(probe):
    _report(fc.run_chacha(probe))


@pytest.mark.parametrize("curve", fc.CURVES)
def test_rejection_classes_were_found(curve):
    _, found = fc.frstream_keys(curve)
    assert len(found) == (3 if curve in fc.REJECT_RUN else 0), found      # (secp256k1 rejects with probability ~2^-128: no such key exists)


@pytest.mark.parametrize("curve", fc.CURVES)
def test_fr_rand_matches_oracle(probe, curve):
    _report(fc.run_frstream(probe, curve))


@pytest.mark.parametrize("T", fc.CHAIN_T)
@pytest.mark.parametrize("curve", fc.CURVES)
def test_chain_weights_match_their_derivation(probe, curve, T):
    _report(fc.run_chain_weights(probe, curve, T))


@pytest.mark.parametrize("curve", fc.CURVES)
def test_chain_weights_depend_on_every_seed_of_their_table_only(probe, curve):
    _report(fc.run_chain_bit_flip(probe, curve))


@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("curve", fc.CURVES)
def test_screen_digests_and_weights(probe, curve, nw):
    _report(fc.run_screen_digest(probe, curve, nw))


@pytest.mark.parametrize("n", fc.MERGE_N)
@pytest.mark.parametrize("curve", fc.CURVES)
def test_merge_weights_match_on_one_and_four_lanes(probe, curve, n):
    _report(fc.run_merge_weights(probe, curve, n))


@pytest.mark.parametrize("mode,lpp", [(0, 0), (1, 4), (1, 16)], ids=["one-lane", "lpp4", "lpp16"])
@pytest.mark.parametrize("curve", fc.CURVES)
def test_merge_weights_depend_on_every_response_scalar(probe, curve, mode, lpp):
    _report(fc.run_merge_scalar_flips(probe, curve, mode, lpp))


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.mark.parametrize("curve,m,n", fc.ELEMENT_SHAPES)
def test_every_proof_element_is_enforced_under_both_transcript_kernels(emu, coracle, curve, m, n):
    eng = emu(curve)
    try:
        _report(fc.run_element_tamper(eng, coracle, curve, m, n))
    finally:
        eng.close()
