"""CPU tests (-m "not gpu") of the opening phase -- mp_reveal_batch, mp_unmask_batch, mp_unmask_batch_dev -- with the kernel bodies under
the development emulator (tools/hostemu): the cases of tests/open_cases.py in full on the STARK curve, the honest shapes on BLS12-377
(the 14-limb field, and the only curve with a subgroup test)."""
import ctypes
import os
import subprocess

import pytest

import open_cases as oc
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


@pytest.mark.parametrize("shape", oc.shapes("stark"), ids=lambda s: "%dx%d" % s)
def test_reveal_and_unmask_match_the_oracle_stark(emu, coracle, shape):
    _run(oc.run_honest, emu("stark"), coracle, "stark", [shape])


@pytest.mark.parametrize("shape", oc.shapes("bls12_377"), ids=lambda s: "%dx%d" % s)
def test_reveal_and_unmask_match_the_oracle_bls12_377(emu, coracle, shape):
    _run(oc.run_honest, emu("bls12_377"), coracle, "bls12_377", [shape])


def test_tiny_batch_matches_the_python_oracle(emu, coracle):
    _run(oc.run_python_oracle, emu("stark"), coracle, "stark")


def test_one_defect_per_card_and_call_level_refusals(emu, coracle):
    _run(oc.run_defects, emu("stark"), coracle, "stark")


def test_agreement_with_the_sigma_calls(emu, coracle):
    _run(oc.run_agreement, emu("stark"), coracle, "stark")


def test_device_pointer_form_gives_the_same_outputs(emu, coracle):
    import torch
    _run(oc.run_dev, emu("stark"), coracle, "stark", torch, "cpu")
