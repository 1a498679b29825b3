"""CPU tests (-m "not gpu") of shuffle proofs on degenerate decks, witnesses and keys (tests/shuffle_edge_cases.py) with the kernel
bodies under the development emulator (tools/hostemu): the Python and the C++ oracle agree on every class on all four curves; the prover
under every plan and the verifier under every strategy on STARK (3, 2) (Toom-Cook on the large-batch splits, Karatsuba on the
small-batch ones).  The other shapes and curves of the case module -- reciprocal Toom-Cook points from (4, 3) on, (17, 2), BLS12-377 --
take minutes here and a second on the GPU: tests/test_gpu_shuffle_edge.py runs them all."""
import ctypes
import os
import subprocess

import pytest

import shuffle_edge_cases as sec
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


def _run(fn, *args):
    fails, checks = fn(*args)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


_ids = lambda s: "%s-%dx%d" % s


@pytest.mark.parametrize("curve", ["stark", "bn254", "secp256k1", "bls12_377"])
def test_shuffle_edge_oracles_agree(coracle, curve):
    _run(sec.run_oracles_agree, coracle, curve)


@pytest.mark.parametrize("shape", sec.EMU_SHAPES, ids=_ids)
def test_prover_matches_the_oracle_on_degenerate_inputs(emu, coracle, shape):
    import torch
    eng = emu(shape[0])
    try:
        _run(sec.run_prover, eng, coracle, *shape, torch, "cpu")
    finally:
        eng.close()


@pytest.mark.parametrize("shape", sec.EMU_SHAPES, ids=_ids)
def test_verifier_matches_the_oracle_on_degenerate_inputs(emu, coracle, shape):
    import torch
    eng = emu(shape[0])
    try:
        _run(sec.run_verifier, eng, coracle, *shape, torch, "cpu")
    finally:
        eng.close()
