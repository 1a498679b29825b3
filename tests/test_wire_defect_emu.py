"""CPU tests (-m "not gpu") of malformed wire inputs to the shuffle calls (tests/wire_defect_cases.py) with the kernel bodies under the
development emulator (tools/hostemu): the verifier with a defect at every point and scalar of a proof, at every point of both decks
and in the per-proof key on STARK (2, 3) and, for the proof and the decks, BLS12-377 (2, 3); the strategies (merged and per equation,
group equations of 3, the pipelined lane, chains) on all of those STARK lanes; the prover's masking factors, deck points, permutations
and keys at N = 6.  Groups of 65, N = 64 / 65 / 130, the 32 769-proof call of k_prove_init, the other two curves and mp_set_validated
take the GPU: tests/test_gpu_wire_defect.py runs everything."""
import ctypes
import os
import subprocess

import pytest

import wire_defect_cases as wd
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


def _run(emu, curve, want, fn, *args, **kw):
    eng = emu(curve)
    try:
        fails, checks = fn(eng, *args, **kw)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks == want


STARK = ("stark", 2, 3)


@pytest.mark.parametrize("shape", [STARK, ("bls12_377", 2, 3)], ids=lambda s: "%s-%dx%d" % s)
def test_verifier_refuses_a_defect_at_every_position(emu, coracle, shape):
    _run(emu, shape[0], wd.positions_count(*shape), wd.run_verifier_positions, coracle, *shape)


def test_verifier_refuses_bad_keys(emu, coracle):
    import torch
    _run(emu, "stark", wd.keys_count("stark"), wd.run_verifier_keys, coracle, *STARK, torch, "cpu")


def test_strategies_keep_the_words(emu, coracle):
    import torch
    _run(emu, "stark", wd.strategies_count(*STARK, group_l=(3,)), wd.run_strategies, coracle, *STARK, torch, "cpu", group_l=(3,))


def test_chains_keep_the_words(emu, coracle):
    _run(emu, "stark", wd.chain_count(), wd.run_chain, coracle, *STARK)


def test_prover_refuses_malformed_witnesses_and_decks(emu, coracle):
    _run(emu, "stark", wd.prover_count(*STARK), wd.run_prover, coracle, *STARK)


def test_prover_refuses_bad_keys(emu, coracle):
    _run(emu, "stark", wd.prover_keys_count("stark"), wd.run_prover_keys, coracle, *STARK)
